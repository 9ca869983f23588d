// sam_header_driver.cpp — the SAM header-end finder (exon_duckdb_amd/csrc/exg_sam_header.hpp) as a program of its own, built by
// tests/test_sam_host.py under AddressSanitizer + UBSan.  Every case copies its bytes into a heap block of exactly their
// size, so that a read one byte past them is caught.  Exit status 0 = every case as expected; else the case's number.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "exg_sam_header.hpp"

static size_t end_of(const std::string &s, char marker = '@') {
    char *p = (char *)malloc(s.size() ? s.size() : 1);
    memcpy(p, s.data(), s.size());
    const size_t r = exg_rd::leading_lines_end(s.size() ? p : p + 0, s.size(), marker);
    const size_t r2 = marker == '@' ? exg_rd::sam_header_end(p, s.size()) : r;
    free(p);
    return r == r2 ? r : (size_t)-1;
}

int main() {
    const std::string hd = "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:10\n", rec = "r\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*\n";
    int n = 0;
#define CASE(cond) \
    do {           \
        n++;       \
        if (!(cond)) return n; \
    } while (0)
    CASE(end_of(hd + rec) == hd.size());                       // 1: a header, then records
    CASE(end_of(hd) == hd.size());                             // 2: a header that ends exactly at the buffer's end (header only, or more to come)
    CASE(end_of(rec + rec) == 0);                              // 3: no header
    CASE(end_of("") == 0);                                     // 4: an empty file
    CASE(end_of("@HD\tVN:1.6\r\n@CO\tx\r\n" + rec) == 19);    // 5: a CR before the LF belongs to the header line
    CASE(end_of("@HD\tVN:1.6\n@CO\tno line feed") == 27);     // 6: an unterminated last header line reaches the end
    CASE(end_of("@") == 1 && end_of("@\n") == 2 && end_of("\n@HD\n") == 0);  // 7: the shortest ones; an empty first line is a record line
    CASE(end_of(hd + rec + "@CO\tbehind a record\n") == hd.size());          // 8: an '@' line behind a record is not header
    CASE(end_of(hd.substr(0, hd.size() - 1)) == hd.size() - 1);              // 9: cut in front of the last LF
    CASE(end_of("##a\n#CHROM\n1\t2\n", '#') == 11);                          // 10: the VCF reader's marker
    // 11: every cut of header + record: the end is min(cut, header size), except that a cut inside the header gives the cut
    for (size_t cut = 0; cut <= hd.size() + rec.size(); cut++) {
        const size_t want = cut < hd.size() ? cut : hd.size();
        if (end_of((hd + rec).substr(0, cut)) != want) return 11;
    }
    printf("sam header driver: %d cases ok\n", n + 1);
    return 0;
}
