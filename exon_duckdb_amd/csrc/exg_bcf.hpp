// exg_bcf.hpp — BCF records -> VCF lines on the device (exg_bcf.hip), for the reader's BCF producer (exg_rd_bcf.cpp) and
// the C-ABI (exg_bcf_to_vcf).
#pragma once
#include <stdint.h>

#include "../../include/exon_gpu.h"

namespace exg {
namespace bcf {

static constexpr uint32_t kMinRecordBytes = 32;  // l_shared, l_indiv and the 24 bytes of fixed fields
static constexpr uint32_t kNoEntry = 0xFFFFFFFFu;  // a dictionary table's length word: no such index

uint64_t workspace_bytes(uint64_t n_bytes);
// Checks the arguments, renders, and brings the result block back (*out).  Synchronises the stream.
int to_vcf(const exg_bcf_to_vcf_args *a, exg_bcf_to_vcf_result *out);

}  // namespace bcf
}  // namespace exg
