// exg_bam_header.hpp — host only: the header of a BAM file (SAM v1 §4.2: magic, l_text + SAM text, n_ref, and per reference
// l_name, name, l_ref) parsed from a prefix of the decoded stream.  No HIP call: runs under ASan in tests/bam_header_driver.cpp.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace exg_rd {

struct BamHeader {
    int32_t n_ref = 0;
    std::string names;              // the reference names closed up, without their NULs
    std::vector<uint64_t> offsets;  // n_ref + 1 offsets into `names`
    uint64_t end = 0;               // decoded offset of the first record
};

enum { kBamHeaderOk = 0, kBamHeaderMore = 1, kBamHeaderBad = -1 };
// p[0, n) = the first n decoded bytes; eof: the stream ends there.  kBamHeaderOk: *out is complete.  kBamHeaderMore: the
// header is longer than n (*need = bytes that are needed at least; never with eof).  kBamHeaderBad: *err says why.
int bam_parse_header(const uint8_t *p, uint64_t n, bool eof, BamHeader *out, uint64_t *need, std::string *err);

}  // namespace exg_rd
