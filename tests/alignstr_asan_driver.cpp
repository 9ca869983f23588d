// tests/alignstr_asan_driver.cpp — TEST INFRASTRUCTURE: a stand-alone program (its own main, no Python, no GPU) that drives the
// host side of the alignment strings — the backtrace of csrc/exg_alignfn.hpp and exon_scan::AlignmentString /
// AlignmentStringBindError of csrc/exon_table_function.hpp that the DuckDB shim registers — under AddressSanitizer + UBSan
// (tests/test_alignstr_host.py builds and runs it).  Both strings live in heap blocks of EXACTLY their length; every CIGAR is
// walked over the pair and its penalty compared with a plain three-matrix dynamic programme written here.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "exon_table_function.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                    \
        }                                                                \
    } while (0)

static long plain_penalty(const std::string &t, const std::string &p, long x, long o, long e) {
    const long inf = 1L << 50;
    const size_t n = t.size(), m = p.size();
    std::vector<long> H((n + 1) * (m + 1), inf), E(H), F(H);
    H[0] = 0;
    for (size_t i = 0; i <= m; i++)
        for (size_t j = 0; j <= n; j++) {
            if (!i && !j) continue;
            const size_t at = i * (n + 1) + j;
            if (j) E[at] = std::min(H[at - 1] + o + e, E[at - 1] + e);
            if (i) F[at] = std::min(H[at - (n + 1)] + o + e, F[at - (n + 1)] + e);
            const long d = i && j ? H[at - (n + 1) - 1] + (t[j - 1] == p[i - 1] ? 0 : x) : inf;
            H[at] = std::min(d, std::min(E[at], F[at]));
        }
    return H[m * (n + 1) + n];
}

// the penalty of a CIGAR over the pair, -1 when it is not an alignment of it in canonical run-length form
static long cigar_penalty(const std::string &t, const std::string &p, const std::string &c, long x, long o, long e) {
    size_t h = 0, v = 0, i = 0;
    long pen = 0;
    char last = 0;
    while (i < c.size()) {
        size_t count = 0, digits = 0;
        while (i < c.size() && c[i] >= '0' && c[i] <= '9') count = count * 10 + (size_t)(c[i++] - '0'), digits++;
        if (!digits || !count || i == c.size() || c[i] == last) return -1;
        last = c[i++];
        if (last == 'M' || last == 'X') {
            if (h + count > t.size() || v + count > p.size()) return -1;
            for (size_t q = 0; q < count; q++)
                if ((t[h + q] == p[v + q]) != (last == 'M')) return -1;
            h += count, v += count, pen += last == 'X' ? x * (long)count : 0;
        } else if (last == 'I') {
            h += count, pen += o + e * (long)count;
        } else if (last == 'D') {
            v += count, pen += o + e * (long)count;
        } else {
            return -1;
        }
    }
    return h == t.size() && v == p.size() ? pen : -1;
}

static int run(const std::string &t, const std::string &p, const exon_scan::AlignmentParams &prm, std::string *out) {
    char *a = (char *)malloc(t.size() ? t.size() : 1), *b = (char *)malloc(p.size() ? p.size() : 1);
    memcpy(a, t.data(), t.size());
    memcpy(b, p.data(), p.size());
    const int rc = exon_scan::AlignmentString(a, t.size(), b, p.size(), prm, out);
    free(a);
    free(b);
    return rc;
}

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33) % n;
}
static std::string random_seq(size_t n, const char *alphabet, uint32_t k) {
    std::string s(n, 'A');
    for (auto &c : s) c = alphabet[rnd(k)];
    return s;
}
static std::string mutate(const std::string &s) {
    std::string out;
    for (char c : s) {
        const uint32_t r = rnd(30);
        if (r == 0) continue;
        if (r == 1) out.push_back("ACGT"[rnd(4)]);
        out.push_back(r == 2 ? "ACGT"[rnd(4)] : c);
    }
    return out;
}

int main() {
    namespace af = exg::alignfn;
    exon_scan::AlignmentParams def;
    std::string c;
    // the pins
    CHECK(run("AACC", "AAACC", def, &c) == EXG_OK && c == "2M1D2M");
    CHECK(run("AAA", "AAAA", def, &c) == EXG_OK && c == "3M1D");
    CHECK(run("", "ACG", def, &c) == EXG_OK && c == "3D");
    CHECK(run("ACG", "", def, &c) == EXG_OK && c == "3I");
    CHECK(run("ACGT", "AGGT", def, &c) == EXG_OK && c == "1M1X2M");
    CHECK(run("", "", def, &c) == EXG_OK && c.empty());
    exon_scan::AlignmentParams prm;
    CHECK(exon_scan::AlignmentStringBindError(false, 0, 1, 1, 1, "memory_low", 10, &prm).empty());
    CHECK(run("AACC", "AAACC", prm, &c) == EXG_OK && c == "2M1D2M");
    CHECK(exon_scan::AlignmentStringBindError(true, -1, 1, 2, 3, "memory_low", 10, &prm).empty());
    CHECK(prm.mismatch == 4 && prm.gap_opening == 4 && prm.gap_extension == 7);
    CHECK(run("AACC", "AAACC", prm, &c) == EXG_OK && c == "2M1D2M");
    // every CIGAR is an alignment of its pair with the optimum's penalty: low-complexity pairs, every parameter set
    const int sets[][3] = {{4, 6, 2}, {1, 1, 1}, {2, 3, 1}, {20, 2, 1}, {3, 0, 2}, {5, 40, 1}, {1023, 1023, 1023}, {1, 0, 1}, {2, 0, 1}};
    for (const auto &ps : sets) {
        prm.mismatch = ps[0], prm.gap_opening = ps[1], prm.gap_extension = ps[2];
        for (int it = 0; it < 150; it++) {
            const std::string t = random_seq(rnd(41), it % 3 ? "ACGT" : "AC", it % 3 ? 4 : 2);
            const std::string p = it % 2 ? mutate(t) : random_seq(rnd(41), it % 3 ? "AC" : "ACGT", it % 3 ? 2 : 4);
            CHECK(run(t, p, prm, &c) == EXG_OK);
            CHECK(cigar_penalty(t, p, c, ps[0], ps[1], ps[2]) == plain_penalty(t, p, ps[0], ps[1], ps[2]));
            CHECK(c.size() <= 2 * (t.size() + p.size()));
        }
    }
    // a long pair, and the longest text a pair can have for its length: every column its own run
    {
        const std::string t = random_seq(1200, "ACGT", 4), p = mutate(t);
        CHECK(run(t, p, def, &c) == EXG_OK && cigar_penalty(t, p, c, 4, 6, 2) == plain_penalty(t, p, 4, 6, 2));
        std::string a, b;
        for (int i = 0; i < 40; i++) a += i % 2 ? "A" : "C", b += i % 2 ? "A" : "G";
        prm.mismatch = 1, prm.gap_opening = 40, prm.gap_extension = 40;
        CHECK(run(a, b, prm, &c) == EXG_OK && c.size() == 80 && cigar_penalty(a, b, c, 1, 40, 40) == 20);
    }
    // the run writer on its own: backwards, merging, counts of several digits
    {
        uint8_t buf[32];
        af::RunWriter rw{buf + sizeof buf, buf, 0, 0, false};
        rw.add('M', 7), rw.add('M', 5), rw.add('X', 1), rw.add('M', 0), rw.add('X', 1), rw.add('D', 1000000);
        const uint8_t *begin = rw.finish();
        CHECK(std::string(reinterpret_cast<const char *>(begin), (size_t)(buf + sizeof buf - begin)) == "1000000D2X12M" && !rw.overflow);
        for (int i = 0; i < 20; i++) rw.add(i % 2 ? 'I' : 'D', 7);  // 40 bytes more do not fit 32: refused, nothing below buf
        rw.finish();
        CHECK(rw.overflow);
    }
    // the sizing of the device's history: the closed form against the sum it stands for
    for (uint32_t e : {1u, 2u, 3u, 7u})
        for (uint64_t mpb : {0ull, 1ull, 2ull, 10ull, 320ull})
            for (uint64_t P : {0ull, 1ull, 5ull, 9ull, 100ull, 652ull, 2000ull}) {
                uint64_t sum = 0;
                for (uint64_t s = 0; s <= P; s++) sum += af::step_width_bound(s, e, mpb);
                CHECK(af::history_entries(e, mpb, P) == sum);
            }
    CHECK(af::history_steps(6, 2, 320, 0) == 652 && af::history_steps(6, 2, 320, 100) == 100 && af::history_steps(6, 2, 320, 1000) == 652);
    // limits and bind-time errors
    exon_scan::AlignmentParams bad;
    bad.mismatch = 0;
    CHECK(run("A", "A", bad, &c) == EXG_E_INVALID_ARG && c.empty());
    CHECK(exon_scan::AlignmentStringBindError(true, 1, 4, 6, 2, "memory_high", 11, &prm) == "Match score must be negative or zero.");
    CHECK(exon_scan::AlignmentStringBindError(true, -1, 511, 6, 2, "memory_high", 11, &prm) == af::kStringParamRangeText);
    CHECK(exon_scan::AlignmentStringBindError(true, INT64_MIN, 4, 6, 2, "memory_high", 11, &prm) == af::kStringParamRangeText);
    CHECK(exon_scan::AlignmentStringBindError(false, 0, 4, 6, 2, "memory", 6, &prm) == "Invalid memory model: memory");
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("alignstr host functions ok\n");
    return 0;
}
