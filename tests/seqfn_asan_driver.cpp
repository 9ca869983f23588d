// tests/seqfn_asan_driver.cpp — TEST INFRASTRUCTURE: a stand-alone program (its own main, no Python, no GPU) that drives the host
// side of the sequence scalars — the tables and the error formatter of csrc/exg_seqfn.hpp and the per-row functions of
// csrc/exon_table_function.hpp that the DuckDB shim registers — under AddressSanitizer + UBSan (tests/test_seqfn_host.py
// builds and runs it).  Outputs go to heap buffers of EXACTLY the size the functions are documented to write, so one byte too
// many is a report; the expected values are computed here by plain switch statements.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

static char plain_map(uint32_t op, char c) {
    switch (op) {
        case EXG_SEQ_COMPLEMENT: return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : 0;
        case EXG_SEQ_REVERSE_COMPLEMENT: return c == 'A' ? 'C' : c == 'T' ? 'G' : c == 'C' ? 'A' : c == 'G' ? 'T' : 0;
        case EXG_SEQ_TRANSCRIBE: return c == 'T' ? 'U' : (c == 'A' || c == 'C' || c == 'G') ? c : 0;
        case EXG_SEQ_REVERSE_TRANSCRIBE: return c == 'U' ? 'T' : (c == 'A' || c == 'C' || c == 'G') ? c : 0;
        default: return 0;
    }
}

// one row through SequenceMap with an exactly-sized heap output; returns the status, the output in *out
static exon_scan::SequenceStatus run(uint32_t op, const std::string &s, std::string *out) {
    // the input on the heap too, without a terminator behind it
    char *in = (char *)malloc(s.size() ? s.size() : 1);
    memcpy(in, s.data(), s.size());
    const size_t n_out = exon_scan::SequenceOutputLength(op, s.size());
    char *o = (char *)malloc(n_out ? n_out : 1);
    const exon_scan::SequenceStatus st = exon_scan::SequenceMap(op, in, s.size(), o);
    out->assign(o, st.code ? 0 : n_out);
    free(o);
    free(in);
    return st;
}

static float run_gc(const std::string &s) {
    char *in = (char *)malloc(s.size() ? s.size() : 1);
    memcpy(in, s.data(), s.size());
    const float f = exon_scan::GcContent(in, s.size());
    free(in);
    return f;
}

static std::string dna(size_t n, uint32_t seed, const char *alphabet) {
    std::string s(n, 'A');
    for (size_t i = 0; i < n; i++) {
        seed = seed * 1664525u + 1013904223u;
        s[i] = alphabet[(seed >> 24) & 3];
    }
    return s;
}

int main() {
    const size_t sizes[] = {0, 1, 2, 3, 11, 12, 13, 36, 39, 4095, 4096, 1u << 20, (1u << 20) + 1, (1u << 20) + 2};
    for (uint32_t op = EXG_SEQ_COMPLEMENT; op <= EXG_SEQ_REVERSE_TRANSCRIBE; op++) {
        const char *alphabet = op == EXG_SEQ_REVERSE_TRANSCRIBE ? "ACGU" : "ACGT";
        for (size_t n : sizes) {
            const std::string s = dna(n, (uint32_t)n + op, alphabet);
            std::string out;
            const exon_scan::SequenceStatus st = run(op, s, &out);
            CHECK(st.code == 0 && out.size() == n);
            bool same = true;
            for (size_t i = 0; i < n; i++) same = same && out[i] == plain_map(op, s[i]);
            CHECK(same);
            // every position of a short row, and the ends and the middle of a long one, made invalid
            for (size_t at : {(size_t)0, n / 2, n ? n - 1 : 0}) {
                if (!n) break;
                std::string bad = s;
                bad[at] = op == EXG_SEQ_REVERSE_TRANSCRIBE ? 'T' : 'U';
                const exon_scan::SequenceStatus e = run(op, bad, &out);
                CHECK(e.code == EXG_PE_SEQ_INVALID_CHARACTER && e.offset == at && e.length == n && e.bytes[0] == (uint8_t)bad[at]);
                CHECK(exon_scan::SequenceErrorText(e) == std::string("Invalid character in sequence: ") + bad[at]);
            }
        }
        for (int c = 0; c < 256; c++) {
            std::string out;
            const exon_scan::SequenceStatus st = run(op, std::string(1, (char)c), &out);
            const char want = plain_map(op, (char)c);
            CHECK(want ? (st.code == 0 && out.size() == 1 && out[0] == want) : (st.code == EXG_PE_SEQ_INVALID_CHARACTER && st.bytes[0] == c));
        }
    }
    for (size_t n : sizes) {
        const std::string s = dna(n, (uint32_t)n, "ACGT");
        std::string out;
        const exon_scan::SequenceStatus st = run(EXG_SEQ_TRANSLATE, s, &out);
        if (n % 3) {
            CHECK(st.code == EXG_PE_SEQ_LENGTH && st.offset == 0 && st.length == n);
            CHECK(exon_scan::SequenceErrorText(st) == "Invalid sequence length: " + std::to_string(n));
            continue;
        }
        CHECK(st.code == 0 && out.size() == n / 3);
        if (n >= 3) {
            std::string bad = s;
            bad[n - 2] = 'N';
            const exon_scan::SequenceStatus e = run(EXG_SEQ_TRANSLATE, bad, &out);
            CHECK(e.code == EXG_PE_SEQ_CODON && e.offset == n - 3 && e.length == n && !memcmp(e.bytes, bad.data() + n - 3, 3));
            CHECK(exon_scan::SequenceErrorText(e) == "Invalid codon: " + bad.substr(n - 3));
        }
    }
    {
        std::string out;
        CHECK(run(EXG_SEQ_TRANSLATE, "ATGCGC", &out).code == 0 && out == "MR");
        CHECK(run(EXG_SEQ_TRANSLATE, "TAATAGTGA", &out).code == 0 && out == "***");
        CHECK(run(EXG_SEQ_TRANSLATE, "NNNN", &out).code == EXG_PE_SEQ_LENGTH);  // the length before any codon
        // every three-byte string over a 7-letter alphabet: a codon exactly when all three letters are A, C, G or T
        const char letters[] = "ACGTUNa";
        for (char a : std::string(letters))
            for (char b : std::string(letters))
                for (char c : std::string(letters)) {
                    const std::string codon{a, b, c};
                    const bool ok = codon.find_first_not_of("ACGT") == std::string::npos;
                    CHECK((run(EXG_SEQ_TRANSLATE, codon, &out).code == 0) == ok);
                }
    }
    for (size_t n : sizes) {
        std::string s = dna(n, 77, "ACGT");
        size_t count = 0;
        for (char c : s) count += c == 'G' || c == 'C';
        const float want = n ? (float)count / (float)n : 0.0f;
        CHECK(run_gc(s) == want);
        for (size_t i = 0; i < n; i += 2) s[i] = (char)(i % 3 ? 'g' : 0xC7);  // lower case and bytes >= 0x80 never count
        count = 0;
        for (char c : s) count += c == 'G' || c == 'C';
        CHECK(run_gc(s) == (n ? (float)count / (float)n : 0.0f));
    }
    // the error formatter into buffers of every size: truncated, always terminated, never past the end
    for (size_t cap = 0; cap <= 48; cap++) {
        char *buf = (char *)malloc(cap ? cap : 1);
        const uint8_t bytes[4] = {'N', 'N', 'N', 0};
        for (uint32_t code : {(uint32_t)EXG_PE_SEQ_INVALID_CHARACTER, (uint32_t)EXG_PE_SEQ_LENGTH, (uint32_t)EXG_PE_SEQ_CODON, 0u}) {
            const size_t k = exg::seqfn::format_error(code, bytes, 18446744073709551615ull, buf, cap);
            CHECK(cap ? (k < cap && buf[k] == 0) : k == 0);
        }
        free(buf);
    }
    for (uint32_t which = 0; which < (uint32_t)exg::seqfn::kSamFlagCount; which++) {
        for (int32_t flag : {0, 1, 4095, 65535, 65536, 65537, -1, -2147483647 - 1, 2147483647})
            CHECK(exon_scan::SamFlag(which, flag) == (((uint32_t)flag & 0xFFFFu & (1u << which)) != 0));
        CHECK(exg::seqfn::kSamFlagNames[which][0] == 'i');
    }
    if (g_fail) return 1;
    printf("seqfn host functions ok\n");
    return 0;
}
