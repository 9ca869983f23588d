// bam_header_driver.cpp — the BAM header parser (csrc/exg_bam_header.cpp, host only) under ASan / UBSan: valid headers, every
// truncation, a header fed in two pieces split at every byte (what the reader does when a header is longer than a segment),
// an n_ref that lies, negative lengths.  Every input is copied into an allocation of exactly its size, so a read past the
// end is a sanitizer report.  Prints "ok" and exits 0.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "exg_bam_header.hpp"

using namespace exg_rd;

static void put32(std::string &s, int32_t v) {
    for (int i = 0; i < 4; i++) s.push_back((char)(((uint32_t)v >> (8 * i)) & 0xFF));
}
static std::string make(const std::vector<std::string> &refs, const std::string &text) {
    std::string s = std::string("BAM\1", 4);
    put32(s, (int32_t)text.size());
    s += text;
    put32(s, (int32_t)refs.size());
    for (const std::string &r : refs) {
        put32(s, (int32_t)r.size() + 1);
        s += r;
        s.push_back('\0');
        put32(s, 1000);
    }
    return s;
}
static int parse_exact(const std::string &s, size_t n, bool eof, BamHeader *h, uint64_t *need, std::string *err) {
    uint8_t *p = (uint8_t *)malloc(n ? n : 1);  // exactly n bytes: ASan sees any read behind them
    memcpy(p, s.data(), n);
    const int rc = bam_parse_header(p, n, eof, h, need, err);
    free(p);
    return rc;
}
#define CHECK(c)                                                 \
    do {                                                         \
        if (!(c)) {                                              \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                             \
        }                                                        \
    } while (0)

int main() {
    std::vector<std::string> refs = {"chr1", "a_reference_name_longer_than_twelve_bytes", "x"};
    for (int i = 0; i < 40; i++) refs.push_back("contig" + std::to_string(i * 7919));
    const std::string good = make(refs, "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000\n");
    const std::string tail = "records follow";
    BamHeader h;
    uint64_t need = 0;
    std::string err;
    CHECK(parse_exact(good + tail, good.size() + tail.size(), false, &h, &need, &err) == kBamHeaderOk);
    CHECK(h.n_ref == (int32_t)refs.size() && h.end == good.size() && h.offsets.size() == refs.size() + 1);
    for (size_t i = 0; i < refs.size(); i++) CHECK(h.names.substr(h.offsets[i], h.offsets[i + 1] - h.offsets[i]) == refs[i]);
    // a header split at every byte: "more" with a need beyond what is there, then complete with the rest; at the end of the
    // stream the same prefix is an error
    for (size_t cut = 0; cut < good.size(); cut++) {
        CHECK(parse_exact(good, cut, false, &h, &need, &err) == kBamHeaderMore);
        CHECK(need > cut && need <= good.size());
        CHECK(parse_exact(good, cut, true, &h, &need, &err) == kBamHeaderBad && !err.empty());
    }
    CHECK(parse_exact(good, good.size(), true, &h, &need, &err) == kBamHeaderOk);
    // no references, no text
    const std::string empty = make({}, "");
    CHECK(parse_exact(empty, empty.size(), true, &h, &need, &err) == kBamHeaderOk && h.n_ref == 0 && h.end == 12);
    // not BAM
    std::string bad = good;
    bad[3] = 2;
    CHECK(parse_exact(bad, bad.size(), false, &h, &need, &err) == kBamHeaderBad);
    CHECK(parse_exact("BA", 2, true, &h, &need, &err) == kBamHeaderBad);
    CHECK(parse_exact("@HD\tVN:1.6\n", 11, true, &h, &need, &err) == kBamHeaderBad);
    // n_ref lies (2^31 - 1 references in a header of a few bytes): no huge reservation, an error at the end of the stream
    std::string liar = make({"chr1"}, "");
    liar[8] = (char)0xFF, liar[9] = (char)0xFF, liar[10] = (char)0xFF, liar[11] = 0x7F;
    CHECK(parse_exact(liar, liar.size(), true, &h, &need, &err) == kBamHeaderBad);
    CHECK(parse_exact(liar, liar.size(), false, &h, &need, &err) == kBamHeaderMore && need > liar.size());
    liar[11] = (char)0xFF;  // negative n_ref
    CHECK(parse_exact(liar, liar.size(), false, &h, &need, &err) == kBamHeaderBad);
    // negative / zero l_name, negative l_text, a name without its NUL
    for (int32_t v : {-1, 0, (int32_t)0x80000000}) {
        std::string s = make({"chr1"}, "");
        for (int i = 0; i < 4; i++) s[12 + i] = (char)(((uint32_t)v >> (8 * i)) & 0xFF);
        CHECK(parse_exact(s, s.size(), false, &h, &need, &err) == kBamHeaderBad);
    }
    std::string s = make({"chr1"}, "");
    s[4] = s[5] = s[6] = s[7] = (char)0xFF;
    CHECK(parse_exact(s, s.size(), false, &h, &need, &err) == kBamHeaderBad);
    s = make({"chr1"}, "");
    s[16 + 4] = 'X';
    CHECK(parse_exact(s, s.size(), false, &h, &need, &err) == kBamHeaderBad);
    // random mutations of a valid header: any answer, no report
    uint64_t x = 88172645463325252ull;
    for (int it = 0; it < 20000; it++) {
        std::string m = good;
        for (int k = 0; k < 3; k++) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            m[x % m.size()] = (char)(x >> 32);
        }
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        (void)parse_exact(m, x % (m.size() + 1), (x >> 40) & 1, &h, &need, &err);
    }
    puts("ok");
    return 0;
}
