// tests/cigar_asan_driver.cpp — TEST INFRASTRUCTURE: a stand-alone program (its own main, no Python, no GPU) that drives the host
// side of the CIGAR scalars — the rules of csrc/exg_cigarfn.hpp and exon_scan::ParseCigar / ExtractFromCigar of
// csrc/exon_table_function.hpp that the DuckDB shim registers — under AddressSanitizer + UBSan (tests/test_cigarfn_host.py builds
// and runs it).  Every row lives in a heap block of EXACTLY its length, so a parser or a backward walker that reads one byte in
// front of a row or behind it is a report.  run_before() — the walker of the device's tiles — is held against next_op() at every
// run of every row.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "exon_table_function.hpp"

namespace cf = exg::cigarfn;

static int g_fail = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                    \
        }                                                                \
    } while (0)

struct Exact {  // a heap copy of exactly the string's length
    char *p;
    size_t n;
    explicit Exact(const std::string &s) : p((char *)malloc(s.size() ? s.size() : 1)), n(s.size()) { memcpy(p, s.data(), s.size()); }
    ~Exact() { free(p); }
    const uint8_t *u() const { return reinterpret_cast<const uint8_t *>(p); }
};

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33) % n;
}

// the parse of s, and every digit run of it through the backward walker
static exon_scan::CigarStatus parse(const std::string &s, std::vector<exon_scan::CigarOp> *ops) {
    const Exact e(s);
    const exon_scan::CigarStatus st = exon_scan::ParseCigar(e.p, e.n, ops);
    const cf::Check ck = cf::check(e.u(), e.n);
    CHECK(ck.ok == !st.code && (ck.ok ? ck.n_ops == ops->size() : ck.offset == st.offset));
    for (size_t k = 1; k <= e.n; k++) {
        if (!cf::is_digit(e.u()[k - 1]) || (k < e.n && cf::is_digit(e.u()[k]))) continue;
        size_t first = k;  // the run is [first, k)
        while (first > 0 && cf::is_digit(e.u()[first - 1])) first--;
        const cf::Run rn = cf::run_before(e.u(), k);
        uint32_t v = 0;
        size_t bad = k;
        for (size_t i = first; i < k && bad == k; i++)
            if (!cf::push_digit(v, e.u()[i])) bad = i;
        CHECK(rn.ok == (bad == k) && (rn.ok ? rn.len == v : rn.bad == bad));
    }
    return st;
}

static void expect_ops(const std::string &s, const std::vector<exon_scan::CigarOp> &want) {
    std::vector<exon_scan::CigarOp> got;
    CHECK(parse(s, &got).code == 0 && got.size() == want.size());
    for (size_t k = 0; k < want.size() && k < got.size(); k++) CHECK(got[k].op == want[k].op && got[k].len == want[k].len);
}
static void expect_error(const std::string &s, uint64_t offset) {
    std::vector<exon_scan::CigarOp> got;
    const exon_scan::CigarStatus st = parse(s, &got);
    CHECK(st.code == EXG_PE_CIGAR_INVALID && st.offset == offset);
}
static exon_scan::CigarStatus extract(size_t seq_len, const std::string &cigar, int32_t *start, int32_t *end) {
    const Exact e(cigar);
    return exon_scan::ExtractFromCigar(seq_len, e.p, e.n, start, end);
}

int main() {
    // the pins (test_scalar_functions.test:91-116) and the decided corners
    expect_ops("1M2M123S", {{'M', 1}, {'M', 2}, {'S', 123}});
    expect_ops("100M", {{'M', 100}});
    expect_ops("", {});
    expect_ops("*", {});
    expect_ops("268435455M", {{'M', 268435455}});
    expect_ops("0000000000001M", {{'M', 1}});
    expect_ops("1M2I3D4N5S6H7P8=9X", {{'M', 1}, {'I', 2}, {'D', 3}, {'N', 4}, {'S', 5}, {'H', 6}, {'P', 7}, {'=', 8}, {'X', 9}});
    expect_error("MMM", 0);
    expect_error("268435456M", 8);
    expect_error("2684354550M", 9);
    expect_error("99999999999999999999M", 8);
    expect_error("12", 2);
    expect_error("5M12", 4);
    expect_error("5M*", 2);
    expect_error("**", 0);
    expect_error("5MM", 2);
    expect_error("5m", 1);
    expect_error("5M 3I", 2);
    expect_error(std::string("5M\0003I", 5), 2);
    expect_error(std::string(5000, '0'), 5000);
    expect_ops(std::string(5000, '0') + "1M", {{'M', 1}});
    CHECK(exon_scan::ParseCigarErrorText("MMM", 3) == "Invalid CIGAR string: MMM");
    // every byte value alone and behind a digit
    for (int c = 0; c < 256; c++) {
        const std::string one(1, (char)c), two = std::string("7") + one;
        std::vector<exon_scan::CigarOp> got;
        const bool letter = strchr("MIDNSHP=X", c) != nullptr && c != 0;
        CHECK(cf::is_op((uint32_t)c) == letter && cf::is_digit((uint32_t)c) == (c >= '0' && c <= '9'));
        CHECK((parse(two, &got).code == 0) == letter);
        if (c != '*') CHECK(parse(one, &got).code == EXG_PE_CIGAR_INVALID);
    }
    // random rows, valid and broken
    for (int it = 0; it < 4000; it++) {
        std::string s;
        std::vector<exon_scan::CigarOp> want, got;
        const uint32_t n_ops = 1 + rnd(12);
        for (uint32_t k = 0; k < n_ops; k++) {
            const uint32_t v = rnd(4) ? rnd(300) : rnd(1u << 28);
            const char op = "MIDNSHP=X"[rnd(9)];
            s += std::string(rnd(4) ? 0 : rnd(12), '0') + std::to_string(v) + op;
            want.push_back({op, (int32_t)v});
        }
        expect_ops(s, want);
        if (it % 2) {
            s[rnd((uint32_t)s.size())] = "MI0 9*x"[rnd(7)];
            parse(s, &got);  // (whatever it is: the walker and the parser agree, and nothing reads outside the row)
        }
    }
    // extract_from_cigar
    int32_t a = -1, b = -1;
    CHECK(extract(6, "2I2M2I", &a, &b).code == 0 && a == 2 && b == 4);
    CHECK(extract(7, "2I2M2I1M", &a, &b).code == 0 && a == 2 && b == 7);
    CHECK(extract(6, "", &a, &b).code == 0 && a == 0 && b == 6);
    CHECK(extract(6, "*", &a, &b).code == 0 && a == 0 && b == 6);
    CHECK(extract(6, "3I", &a, &b).code == 0 && a == 3 && b == 3);
    CHECK(extract(6, "6M", &a, &b).code == 0 && a == 0 && b == 6);
    CHECK(extract(0, "1M", &a, &b).code == 0 && a == 0 && b == 0);
    CHECK(extract(6, "4I", &a, &b).code == EXG_PE_CIGAR_RANGE);
    CHECK(extract(6, "4I1M3I", &a, &b).code == EXG_PE_CIGAR_RANGE);
    CHECK(extract((size_t)1 << 31, "1M", &a, &b).code == EXG_PE_CIGAR_RANGE);
    CHECK(extract(((size_t)1 << 31) - 1, "1M", &a, &b).code == 0 && b == 0x7FFFFFFF);
    const exon_scan::CigarStatus st = extract(6, "9I1M9I5", &a, &b);  // a syntax error comes before the range error
    CHECK(st.code == EXG_PE_CIGAR_INVALID && st.offset == 7);
    CHECK(exon_scan::ExtractFromCigarErrorText(st) == "Invalid CIGAR string");
    char text[96];
    CHECK(std::string(text, cf::format_error(EXG_PE_CIGAR_INVALID, 3, 7, text, sizeof text)) == "Invalid CIGAR string in row 3 at byte 7");
    CHECK(std::string(text, cf::format_error(EXG_PE_CIGAR_RANGE, 3, 0, text, sizeof text)) == "CIGAR insertions exceed the sequence in row 3");
    if (g_fail) return 1;
    printf("cigarfn host functions ok\n");
    return 0;
}
