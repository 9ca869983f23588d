// bcf_header_driver.cpp — the BCF header parser and dictionary builder (csrc/exg_bcf_header.cpp: host only) as a program of its
// own, built with -fsanitize=address,undefined by tests/test_bcf_host.py.  Reads a BCF file's DECODED bytes from the file named
// on the command line and prints what the parser made of them, one item a line:
//   rc <0 ok | 1 more | -1 bad> need <bytes> end <offset> samples <n> gt <index or -1> err <text>
//   string <index> <id>    (or "string <index> -" for an index no ID has)
//   contig <index> <id>
// With a second argument "cuts": the same header cut at every length (eof = false) must ask for more and never read past the
// cut (each prefix is parsed from a heap copy of exactly its size), then, with eof = true, must be refused; prints "cuts ok".
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "exg_bcf_header.hpp"

static void dump(const char *what, const exg_rd::BcfDict &d) {
    for (uint32_t i = 0; i < d.size(); i++) {
        if (d.table[2 * i + 1] == exg_rd::kBcfNoEntry) printf("%s %u -\n", what, i);
        else printf("%s %u %.*s\n", what, i, (int)d.table[2 * i + 1], d.bytes.c_str() + d.table[2 * i]);
    }
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> all;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + k);
    fclose(f);
    if (argc > 2 && strcmp(argv[2], "cuts") == 0) {
        exg_rd::BcfHeader whole;
        uint64_t need = 0;
        std::string err;
        if (exg_rd::bcf_parse_header(all.data(), all.size(), true, &whole, &need, &err) != exg_rd::kBcfHeaderOk) return 3;
        for (uint64_t n = 0; n < whole.end; n++) {
            std::vector<uint8_t> part(all.begin(), all.begin() + (long)n);  // (its own allocation: a read past n is ASan's to find)
            exg_rd::BcfHeader h;
            err.clear();
            int rc = exg_rd::bcf_parse_header(part.data(), n, false, &h, &need, &err);
            if (rc != exg_rd::kBcfHeaderMore || need <= n || need > whole.end) {
                printf("cut %llu: rc %d need %llu\n", (unsigned long long)n, rc, (unsigned long long)need);
                return 4;
            }
            rc = exg_rd::bcf_parse_header(part.data(), n, true, &h, &need, &err);
            if (rc != exg_rd::kBcfHeaderBad || err.empty()) {
                printf("cut %llu at the end of the stream: rc %d\n", (unsigned long long)n, rc);
                return 5;
            }
        }
        printf("cuts ok\n");
        return 0;
    }
    exg_rd::BcfHeader h;
    uint64_t need = 0;
    std::string err;
    const int rc = exg_rd::bcf_parse_header(all.data(), all.size(), true, &h, &need, &err);
    printf("rc %d need %llu end %llu samples %u gt %d err %s\n", rc, (unsigned long long)need, (unsigned long long)h.end, h.n_samples, (int)h.gt_index, err.c_str());
    if (rc == exg_rd::kBcfHeaderOk) {
        dump("string", h.strings);
        dump("contig", h.contigs);
        printf("text %zu\n", h.text.size());
    }
    return 0;
}
