// exg_bam.hpp — the BAM record scan in two halves (exg_bam.hip), for the reader: the side buffer's size is known only when the
// records have been found and measured, and the reader wants a pinned block of exactly that size before the strings are
// written (their pointers address it).  exg_bam_scan is the two halves back to back.
#pragma once
#include <stdint.h>

#include "../../include/exon_gpu.h"

namespace exg {
namespace bam {

static constexpr uint32_t kTileBytes = 32768;  // (exg_chain.hpp's tile)
static constexpr uint32_t kMinRecordBytes = 36;  // block_size + the 32 bytes of fixed fields

uint64_t workspace_bytes(uint64_t n_bytes);

// Records found (speculate, stitch, index), validated and measured (rows, prefix sum of the side-buffer lengths); *out = the
// result so far: n_records, consumed_bytes, side_bytes, the first error, the tile counters.  No column is written.
// Synchronises the stream.  d_columns / d_side / capacity_records of `a` are not looked at.
int discover(const exg_bam_scan_args *a, exg_bam_scan_result *out);
// The columns of the first res->n_records rows, for the same args (same workspace, untouched in between) + d_columns,
// d_validity, d_side, side_base.  Asynchronous.
int emit(const exg_bam_scan_args *a, const exg_bam_scan_result *res);

}  // namespace bam
}  // namespace exg
