// exg_bcf_header.hpp — host only: the header of a BCF 2.2 file (magic `BCF\2\2`, l_text, the VCF header text with its NUL) parsed
// from a prefix of the decoded stream, and the two dictionaries its records index.  No HIP call: runs under ASan in
// tests/bcf_header_driver.cpp.
//   string dictionary: the IDs of the ##FILTER / ##INFO / ##FORMAT lines — with IDX= at that index, without in order of first
//                      appearance; PASS is 0 whether it is declared or not; an ID used by INFO and FORMAT has one index
//   contig dictionary: the IDs of the ##contig lines, likewise (nothing is implied)
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace exg_rd {

static constexpr uint32_t kBcfNoEntry = 0xFFFFFFFFu;

struct BcfDict {
    std::string bytes;            // the names closed up
    std::vector<uint32_t> table;  // per index {offset, length}; length kBcfNoEntry: no ID has this index
    uint32_t size() const { return (uint32_t)(table.size() / 2); }
    int64_t find(const std::string &id) const;  // -1: not there
};

struct BcfHeader {
    std::string text;  // the header's text without its NULs, ended by LF: what the VCF path parses
    uint64_t end = 0;  // decoded offset of the first record
    uint32_t n_samples = 0;
    BcfDict strings, contigs;
    uint32_t gt_index = ~0u;  // the string dictionary's index of GT
};

enum { kBcfHeaderOk = 0, kBcfHeaderMore = 1, kBcfHeaderBad = -1 };
// p[0, n) = the first n decoded bytes; eof: the stream ends there.  kBcfHeaderOk: *out is complete.  kBcfHeaderMore: the
// header is longer than n (*need = bytes that are needed at least; never with eof).  kBcfHeaderBad: *err says why.
int bcf_parse_header(const uint8_t *p, uint64_t n, bool eof, BcfHeader *out, uint64_t *need, std::string *err);

}  // namespace exg_rd
