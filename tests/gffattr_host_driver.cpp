// tests/gffattr_host_driver.cpp — TEST INFRASTRUCTURE: a stand-alone program (its own main, no Python, no GPU) over the host side
// of gff_parse_attributes — the rules of csrc/exg_gffattr.hpp and exon_scan::GffParseAttributes of csrc/exon_table_function.hpp
// that the DuckDB shim registers — built with AddressSanitizer + UBSan (tests/test_gffattr_host.py builds and runs it).  Every field
// lives in a heap block of EXACTLY its length, so a parser that reads one byte in front of a field or behind it is a report.
// walk_words() — the word walk a wavefront of the device op performs, its masks built by a loop — is held against the
// left-to-right parser on every field.
//
// usage: gffattr_host_driver [file ...]   each file: one field a line (a GFF3 line's ninth field, or the whole line when it has
// no tabs); every field must parse the same way by both statements of the rules
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <string>
#include <utility>
#include <vector>

#include "exon_table_function.hpp"

namespace ga = exg::gffattr;

static int g_fail = 0;
#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                         \
        }                                                                     \
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

using Pairs = std::vector<std::pair<std::string, std::string>>;

// the host scalar on s, with the word walk held against it: the same entries, or the same offset and length
static exon_scan::GffAttributeStatus parse(const std::string &s, Pairs *pairs) {
    const Exact e(s);
    std::vector<exon_scan::GffAttribute> list;
    const exon_scan::GffAttributeStatus st = exon_scan::GffParseAttributes(e.p, e.n, &list);
    std::vector<exon_scan::GffAttribute> walked;
    const ga::Verdict v = ga::walk_words(e.u(), (uint32_t)e.n, [&walked](uint32_t k, uint32_t kn, uint32_t val, uint32_t vn) {
        walked.push_back(exon_scan::GffAttribute{k, kn, val, vn});
    });
    if (st.code) {
        CHECK(v.kind == ga::kError && v.a == st.offset && v.b == st.length);
        if (!(v.kind == ga::kError && v.a == st.offset && v.b == st.length))
            fprintf(stderr, "  field '%s': parser (%llu, %llu), walk kind %u (%u, %u)\n", s.c_str(), (unsigned long long)st.offset,
                    (unsigned long long)st.length, v.kind, v.a, v.b);
    } else {
        CHECK(v.kind == ga::kEntry && v.a == list.size() && walked.size() == list.size());
        for (size_t k = 0; k < list.size() && k < walked.size(); k++)
            CHECK(walked[k].key_start == list[k].key_start && walked[k].key_len == list[k].key_len && walked[k].value_start == list[k].value_start &&
                  walked[k].value_len == list[k].value_len);
        if (!(v.kind == ga::kEntry && walked.size() == list.size())) fprintf(stderr, "  field '%s'\n", s.c_str());
    }
    pairs->clear();
    for (const exon_scan::GffAttribute &a : list) {
        CHECK(a.key_len && a.value_len && a.key_start + a.key_len < a.value_start && a.value_start + a.value_len <= e.n);
        pairs->emplace_back(std::string(e.p + a.key_start, a.key_len), std::string(e.p + a.value_start, a.value_len));
    }
    return st;
}

static void expect_pairs(const std::string &s, const Pairs &want) {
    Pairs got;
    CHECK(parse(s, &got).code == 0);
    CHECK(got == want);
}
static void expect_error(const std::string &s, uint64_t offset, uint64_t length) {
    Pairs got;
    const exon_scan::GffAttributeStatus st = parse(s, &got);
    CHECK(st.code == EXG_PE_GFF_ATTRIBUTES && st.offset == offset && st.length == length);
    const Exact e(s);
    CHECK(exon_scan::GffAttributeErrorText(e.p, st) == "Invalid attribute: '" + s.substr(offset, length) + "' expected 'key=value;key2=value2'");
}

int main(int argc, char **argv) {
    // the pins (test_gff_scan.test:79-99) and every rule's examples
    expect_pairs("key=value", {{"key", "value"}});
    expect_pairs("key=value;", {{"key", "value"}});
    expect_pairs("key=value;key2=value2", {{"key", "value"}, {"key2", "value2"}});
    expect_error("ID", 0, 2);
    expect_pairs(";;a=b;;;c=d;;", {{"a", "b"}, {"c", "d"}});
    expect_pairs(" a=b ;\tc=d\r\n", {{"a", "b"}, {"c", "d"}});
    expect_pairs(" \t\n\v\f\ra=b\r\f\v\n\t ", {{"a", "b"}});
    expect_pairs("a = b", {{"a ", " b"}});
    expect_pairs("a==b", {{"a", "b"}});
    expect_pairs("=a=b", {{"a", "b"}});
    expect_pairs("a=b=", {{"a", "b"}});
    expect_pairs("a= =", {{"a", " "}});
    expect_pairs("a=b= ", {{"a", "b"}});
    expect_pairs("a=b;a=c", {{"a", "b"}, {"a", "c"}});
    expect_pairs("a\xE9=\xE9 ;", {{"a\xE9", "\xE9"}});
    expect_pairs("\xA0" "a=b\x85", {{"\xA0" "a", "b\x85"}});
    expect_pairs("ID=gene%3B1;Name=x y", {{"ID", "gene%3B1"}, {"Name", "x y"}});
    expect_error("a", 0, 1);
    expect_error("a=", 0, 2);
    expect_error("=a", 0, 2);
    expect_error("a= ", 0, 2);
    expect_error("a=b=c", 0, 5);
    expect_error("a= =b", 0, 5);
    expect_error("   ", 0, 0);
    expect_error("a=b;  ;c=d", 4, 0);
    expect_error("", 0, 0);
    expect_error(";", 0, 1);
    expect_error(";;;", 0, 3);
    expect_error("===", 0, 3);
    expect_error("a=b;  x  ;c", 6, 1);
    expect_error("a=b; x ;y", 5, 1);  // the leftmost failing segment
    expect_pairs(std::string("a=b;\0=c", 7), {{"a", "b"}, {std::string(1, '\0'), "c"}});  // (NUL is a byte like any other)
    // seventy entries, and segments astride every word seam
    {
        std::string s;
        Pairs want;
        for (int k = 0; k < 70; k++) s += "a=b;", want.emplace_back("a", "b");
        expect_pairs(s, want);
    }
    for (size_t pad = 50; pad < 80; pad++) {
        const std::string k(pad, 'k');
        expect_pairs(k + "=v", {{k, "v"}});
        expect_pairs(k + "==v;", {{k, "v"}});
        expect_pairs("x=" + k + "  \t  ;  y=z", {{"x", k}, {"y", "z"}});
        expect_pairs("x=" + k + "=  \t  ;  y=z", {{"x", k}, {"y", "z"}});
        expect_pairs("x=" + std::string(pad, ' ') + "=", {{"x", std::string(pad, ' ')}});
        expect_error("x=" + std::string(pad, ' '), 0, 2);
        expect_error("x=y;" + std::string(pad, ' ') + ";", 4, 0);
        expect_error("x=y;" + std::string(pad, ' ') + "z ;", 4 + pad, 1);
        expect_error(k + "=v=" + std::string(pad, ' ') + "w", 0, 2 * pad + 4);
    }
    // every prefix of a field of 200 bytes
    {
        std::string f;
        while (f.size() < 200) f += "ID=cds-" + std::to_string(f.size()) + " ; Parent = rna\t;;Dbxref=GeneID:1==x;";
        f.resize(200);
        Pairs got;
        for (size_t n = 0; n <= f.size(); n++) parse(f.substr(0, n), &got);
    }
    // every byte value as the key, and around an entry: only the six blanks are trimmed
    for (int c = 1; c < 256; c++) {
        const std::string one(1, (char)c);
        Pairs got;
        const bool blank = c == ' ' || (c >= 9 && c <= 13);
        CHECK(ga::is_blank((uint32_t)c) == blank);
        if (c == ';' || c == '=') continue;
        if (blank) expect_pairs(one + "a=b" + one, {{"a", "b"}});
        else expect_pairs(one + "a=b" + one, {{one + "a", "b" + one}});
    }
    // random fields, most of them broken: both statements agree, and nothing reads outside the field
    for (int it = 0; it < 20000; it++) {
        std::string s;
        const uint32_t n = rnd(201);
        for (uint32_t k = 0; k < n; k++) s += "ab=;; \t\r\xE9" "aaab=="[rnd(15)];
        Pairs got;
        parse(s, &got);
    }
    // the files: every field by both
    size_t fields = 0, entries = 0;
    for (int a = 1; a < argc; a++) {
        std::ifstream in(argv[a], std::ios::binary);
        CHECK(in.good());
        std::string line;
        while (std::getline(in, line)) {
            if (line.empty() || line[0] == '#') continue;
            size_t tab = 0, at = 0;
            for (int k = 0; k < 8 && tab != std::string::npos; k++) tab = line.find('\t', at), at = tab + 1;
            const std::string field = tab == std::string::npos ? line : line.substr(at);
            Pairs got;
            CHECK(parse(field, &got).code == 0);
            fields++, entries += got.size();
        }
    }
    if (g_fail) return 1;
    printf("gffattr host functions ok: %zu fields, %zu entries from files\n", fields, entries);
    return 0;
}
