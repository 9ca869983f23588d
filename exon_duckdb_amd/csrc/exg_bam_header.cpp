// exg_bam_header.cpp — see exg_bam_header.hpp.  Every length is checked against what is there before a byte is read.
#include "exg_bam_header.hpp"

#include <string.h>

namespace exg_rd {

static uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

int bam_parse_header(const uint8_t *p, uint64_t n, bool eof, BamHeader *out, uint64_t *need, std::string *err) {
    *out = BamHeader();
    *need = 0;
    auto more = [&](uint64_t upto, const char *what) {
        if (eof) {
            *err = std::string("the BAM header is truncated (") + what + ")";
            return (int)kBamHeaderBad;
        }
        *need = upto;
        return (int)kBamHeaderMore;
    };
    if (n < 4) {
        if (n && memcmp(p, "BAM\1", (size_t)n) != 0) return *err = "not a BAM file (the decoded bytes do not begin with BAM\\1)", kBamHeaderBad;
        return eof ? (*err = "not a BAM file (the decoded bytes do not begin with BAM\\1)", (int)kBamHeaderBad) : more(12, "magic");
    }
    if (memcmp(p, "BAM\1", 4) != 0) return *err = "not a BAM file (the decoded bytes do not begin with BAM\\1)", kBamHeaderBad;
    if (n < 8) return more(12, "l_text");
    const uint64_t l_text = le32(p + 4);
    if (l_text > 0x7FFFFFFFull) return *err = "invalid BAM header: negative l_text", kBamHeaderBad;
    uint64_t pos = 8 + l_text;  // (the SAM text is skipped)
    if (n < pos + 4) return more(pos + 4, "n_ref");
    const uint32_t n_ref = le32(p + pos);
    if (n_ref > 0x7FFFFFFFu) return *err = "invalid BAM header: negative n_ref", kBamHeaderBad;
    pos += 4;
    // (n_ref may lie: nothing is reserved from it beyond what the bytes that are there can hold — 9 bytes a reference at least)
    if ((uint64_t)n_ref * 9 > n - pos && eof) return *err = "the BAM header is truncated (n_ref references do not fit)", kBamHeaderBad;
    out->offsets.reserve((size_t)((uint64_t)n_ref < (n - pos) / 9 ? n_ref : (n - pos) / 9) + 1);
    out->offsets.push_back(0);
    for (uint32_t i = 0; i < n_ref; i++) {
        if (n < pos + 4) return more(pos + 4 + (uint64_t)(n_ref - i - 1) * 9 + 5, "l_name");
        const uint32_t l_name = le32(p + pos);
        if (l_name == 0 || l_name > 0x7FFFFFFFu) return *err = "invalid BAM header: l_name of reference " + std::to_string(i) + " is not positive", kBamHeaderBad;
        if (n < pos + 4 + (uint64_t)l_name + 4) return more(pos + 4 + (uint64_t)l_name + 4 + (uint64_t)(n_ref - i - 1) * 9, "reference name");
        const uint8_t *name = p + pos + 4;
        if (name[l_name - 1] != 0) return *err = "invalid BAM header: the name of reference " + std::to_string(i) + " is not NUL-terminated", kBamHeaderBad;
        out->names.append((const char *)name, strnlen((const char *)name, l_name - 1));
        out->offsets.push_back(out->names.size());
        pos += 4 + (uint64_t)l_name + 4;  // (l_ref is not a column)
    }
    out->n_ref = (int32_t)n_ref;
    out->end = pos;
    return kBamHeaderOk;
}

}  // namespace exg_rd
