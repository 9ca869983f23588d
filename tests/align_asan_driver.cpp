// tests/align_asan_driver.cpp — TEST INFRASTRUCTURE: a stand-alone program (its own main, no Python, no GPU) that drives the host
// side of the alignment scores — the rules of csrc/exg_alignfn.hpp and exon_scan::AlignmentScore / AlignmentBindError of
// csrc/exon_table_function.hpp that the DuckDB shim registers — under AddressSanitizer + UBSan (tests/test_alignfn_host.py builds
// and runs it).  Both strings live in heap blocks of EXACTLY their length, so an extend that reads one byte past either end is a
// report; the expected penalties come from a plain three-matrix dynamic programme written here.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
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

static int run(const std::string &t, const std::string &p, const exon_scan::AlignmentParams &prm, float *score) {
    char *a = (char *)malloc(t.size() ? t.size() : 1), *b = (char *)malloc(p.size() ? p.size() : 1);
    memcpy(a, t.data(), t.size());
    memcpy(b, p.data(), p.size());
    const int rc = exon_scan::AlignmentScore(a, t.size(), b, p.size(), prm, score);
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
    float f = 1;
    // the pins
    CHECK(run("AACC", "AACC", def, &f) == EXG_OK && f == 0.0f && !std::signbit(f));
    CHECK(run("AACC", "AAACC", def, &f) == EXG_OK && f == -8.0f);
    CHECK(run("", "ACG", def, &f) == EXG_OK && f == -12.0f);
    CHECK(run("", "", def, &f) == EXG_OK && f == 0.0f && !std::signbit(f));
    exon_scan::AlignmentParams ones;
    ones.mismatch = ones.gap_opening = ones.gap_extension = 1;
    CHECK(run("AACC", "AAACC", ones, &f) == EXG_OK && f == -2.0f);
    // against the plain programme: lengths around the 8-byte steps of extend, equal tails, every parameter set
    const int sets[][3] = {{4, 6, 2}, {1, 1, 1}, {2, 3, 1}, {20, 2, 1}, {3, 0, 2}, {5, 40, 1}, {1023, 1023, 1023}, {1, 0, 1}};
    for (const auto &ps : sets) {
        exon_scan::AlignmentParams prm;
        prm.mismatch = ps[0], prm.gap_opening = ps[1], prm.gap_extension = ps[2];
        for (int it = 0; it < 150; it++) {
            const std::string t = random_seq(rnd(41), it % 3 ? "ACGT" : "AC", it % 3 ? 4 : 2);
            const std::string p = it % 2 ? mutate(t) : random_seq(rnd(41), "ACGT", 4);
            CHECK(run(t, p, prm, &f) == EXG_OK);
            CHECK(f == (float)-plain_penalty(t, p, ps[0], ps[1], ps[2]));
            float g = 0;
            CHECK(run(p, t, prm, &g) == EXG_OK && g == f);  // the roles are symmetric
        }
        for (size_t n : {7u, 8u, 9u, 15u, 16u, 17u, 64u}) {
            const std::string t = random_seq(n, "ACGT", 4);
            CHECK(run(t, t, prm, &f) == EXG_OK && f == 0.0f);
            std::string q = t;
            q[n - 1] ^= 6;
            CHECK(run(t, q, prm, &f) == EXG_OK && f == (float)-plain_penalty(t, q, ps[0], ps[1], ps[2]));
        }
    }
    // a long pair: whole 8-byte steps, wavefronts of hundreds of diagonals
    {
        const std::string t = random_seq(1200, "ACGT", 4), p = mutate(t);
        CHECK(run(t, p, def, &f) == EXG_OK && f == (float)-plain_penalty(t, p, 4, 6, 2));
    }
    // limits and bind-time errors
    exon_scan::AlignmentParams bad;
    bad.mismatch = 0;
    CHECK(run("A", "A", bad, &f) == EXG_E_INVALID_ARG);
    bad.mismatch = 4, bad.gap_extension = 1024;
    CHECK(run("A", "A", bad, &f) == EXG_E_INVALID_ARG);
    CHECK(!af::params_ok(1, -1, 1) && af::params_ok(1, 0, 1) && af::params_ok(1023, 1023, 1023) && !af::params_ok(1024, 0, 1));
    CHECK(exon_scan::AlignmentBindError(true, 1, 4, 6, 2, "memory_high", 11) == "Match score must be negative or zero.");
    CHECK(exon_scan::AlignmentBindError(true, -1, 4, 6, 2, "memory_high", 11).find("not supported") != std::string::npos);
    CHECK(exon_scan::AlignmentBindError(true, 0, 4, 6, 2, "memory_low", 10).empty());
    CHECK(exon_scan::AlignmentBindError(false, 99, 4, 6, 2, "memory_med", 10).empty());
    CHECK(exon_scan::AlignmentBindError(false, 0, 4, 6, 2, "memory", 6) == "Invalid memory model: memory");
    CHECK(exon_scan::AlignmentBindError(false, 0, 4, 6, 2, "", 0) == "Invalid memory model: ");
    CHECK(af::penalty_bound(1023, 1023, af::kMaxPairBytes, 0) < 0x80000000u);
    char text[96];
    const size_t k = af::format_error(EXG_PE_ALIGN_TOO_LONG, 301, 300, text, sizeof text);
    CHECK(std::string(text, k) == "Alignment pair too long: 301 bytes (at most 300)");
    CHECK(af::format_error(0, 301, 300, text, sizeof text) == 0 && text[0] == 0);
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("alignfn host functions ok\n");
    return 0;
}
