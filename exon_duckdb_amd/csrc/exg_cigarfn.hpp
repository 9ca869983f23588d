// exg_cigarfn.hpp — the rules of parse_cigar / extract_from_cigar, stated ONCE for the device op (exg_cigarfn.hip), the host
// scalars (exon_table_function.hpp, which the DuckDB shim registers) and the C-ABI's error text.
// Plain C++: no HIP, no DuckDB; usable from host and device code.
//
// Reference: exon/src/exon/sam_functions/module.cpp:32-131 and rust/src/sam_functions.rs:114-200.  INTEGRATION.md, "CIGAR
// scalars", carries the same rules.
//   grammar      one or more of [one or more ASCII digits, one of MIDNSHP=X] — exactly what the SAM scan accepts
//                (exg_sam.hip: sam_cigar); a length is at most 2^28 - 1 in VALUE: leading zeros are allowed and the number of
//                digits is not bounded
//   absent       the empty string and the text `*` are the CIGAR without operations (the scans hand `*` over as the empty string)
//   parse_cigar  the operations in order: (letter, length)
//   extract_from_cigar(sequence, cigar)
//                start = the first operation's length if it is I, else 0; end = |sequence| - the last operation's length if it
//                is I, else |sequence|; the slice is the bytes [start, end).  A CIGAR of one operation is both first and last;
//                the absent CIGAR gives {0, |sequence|}.  The whole CIGAR is validated.  start > end, or |sequence| > 2^31 - 1:
//                EXG_PE_CIGAR_RANGE
// Where an invalid CIGAR is reported: the offset at which a left-to-right parser (next_op below) stops —
//   a byte that is neither a digit nor an operation     that byte's offset
//   an operation letter with no digit in front of it    the letter's offset
//   digits that run to the end of the row               the row's length
//   a length above the bound                            the digit at which the value first exceeds it
// The leftmost such offset of a row is the row's error; in extract_from_cigar a syntax error comes before the range error.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "exon_gpu.h"

#if defined(__HIPCC__)
#define EXG_CIG_HD __host__ __device__ inline
#else
#define EXG_CIG_HD inline
#endif

namespace exg {
namespace cigarfn {

static constexpr uint32_t kMaxLen = (1u << 28) - 1;
static constexpr const char *kInvalidText = "Invalid CIGAR string";  // sam_functions.rs:122 / test_scalar_functions.test:97
static constexpr const char *kRangeText = "CIGAR insertions exceed the sequence";

EXG_CIG_HD constexpr bool is_digit(uint32_t c) { return c - (uint32_t)'0' <= 9u; }
// MIDNSHP=X: '=' (0x3D) is the lowest, 'X' (0x58) the highest — bit (c - '=') of one word
constexpr uint32_t op_bit(char c) { return 1u << ((uint32_t)(uint8_t)c - (uint32_t)'='); }
static constexpr uint32_t kOpMask =
    op_bit('M') | op_bit('I') | op_bit('D') | op_bit('N') | op_bit('S') | op_bit('H') | op_bit('P') | op_bit('=') | op_bit('X');
EXG_CIG_HD constexpr bool is_op(uint32_t c) { return c - (uint32_t)'=' <= (uint32_t)('X' - '=') && ((kOpMask >> (c - (uint32_t)'=')) & 1u); }
EXG_CIG_HD constexpr bool is_absent(const uint8_t *s, uint64_t n) { return n == 0 || (n == 1 && s[0] == '*'); }

// v * 10 + d, or false when that exceeds kMaxLen (v <= kMaxLen: nothing wraps)
EXG_CIG_HD constexpr bool push_digit(uint32_t &v, uint32_t c) {
    if (v > kMaxLen / 10u) return false;
    v = v * 10u + (c - (uint32_t)'0');
    return v <= kMaxLen;
}

// The left-to-right parser: one operation of s[0, n) from offset i < n.  ok: the operation, next = the offset behind its
// letter.  !ok: next = the offset the error is reported at.
struct Step {
    uint64_t next;
    uint32_t len;
    uint8_t op;
    bool ok;
};
EXG_CIG_HD constexpr Step next_op(const uint8_t *s, uint64_t n, uint64_t i) {
    const uint64_t first = i;
    uint32_t v = 0;
    for (; i < n && is_digit(s[i]); i++)
        if (!push_digit(v, s[i])) return Step{i, 0, 0, false};
    if (i >= n) return Step{n, 0, 0, false};                                // digits (or nothing) up to the end of the row
    if (i == first || !is_op(s[i])) return Step{i, 0, 0, false};            // a letter without digits, or a bad byte
    return Step{i + 1, v, s[i], true};
}

// The same length read from its END: the digit run in front of offset e (s[e - 1] is a digit), walked back to its first digit
// and never in front of the row.  What a terminator — the operation letter, a bad byte or the row's end — does where the row
// is cut among many lanes: one walker a run, linear in the run.  Up to nine digits are summed on the way back (< 2^32); a
// longer run, or a value above the bound, is read once more from its first digit as next_op reads it.
struct Run {
    uint64_t bad;  // !ok: the digit at which the value first exceeds the bound
    uint32_t len;
    bool ok;
};
EXG_CIG_HD constexpr Run run_before(const uint8_t *s, uint64_t e) {
    uint64_t k = e;
    uint32_t v = 0, pw = 1;
    for (int nd = 0; nd < 9 && k > 0 && is_digit(s[k - 1]); nd++, k--, pw *= 10u) v += (s[k - 1] - (uint32_t)'0') * pw;
    const bool whole = !(k > 0 && is_digit(s[k - 1]));
    if (whole && v <= kMaxLen) return Run{0, v, true};
    while (k > 0 && is_digit(s[k - 1])) k--;
    v = 0;
    for (; k < e; k++)
        if (!push_digit(v, s[k])) return Run{k, 0, false};
    return Run{0, v, true};
}

// the whole row: the number of operations, or where the first error is
struct Check {
    uint64_t offset;  // !ok
    uint64_t n_ops;
    bool ok;
};
EXG_CIG_HD constexpr Check check(const uint8_t *s, uint64_t n) {
    Check c{0, 0, true};
    if (is_absent(s, n)) return c;
    for (uint64_t i = 0; i < n;) {
        const Step st = next_op(s, n, i);
        if (!st.ok) return Check{st.next, c.n_ops, false};
        i = st.next, c.n_ops++;
    }
    return c;
}

// extract_from_cigar's two numbers from the first and the last operation of a valid CIGAR (absent: neither is read)
EXG_CIG_HD constexpr bool extract_range(bool absent, uint32_t first_op, uint32_t first_len, uint32_t last_op, uint32_t last_len,
                                        uint64_t sequence_length, int32_t *start, int32_t *end) {
    if (sequence_length > 0x7FFFFFFFull) return false;
    const int64_t s = !absent && first_op == 'I' ? (int64_t)first_len : 0;
    const int64_t e = (int64_t)sequence_length - (!absent && last_op == 'I' ? (int64_t)last_len : 0);
    if (s > e) return false;
    *start = (int32_t)s, *end = (int32_t)e;
    return true;
}

// the text of an EXG_PE_CIGAR_* of row `row`; returns the number of bytes written (no terminator counted)
inline size_t format_error(uint32_t code, uint64_t row, uint64_t offset, char *out, size_t cap) {
    if (!cap) return 0;
    int n = 0;
    if (code == EXG_PE_CIGAR_INVALID)
        n = snprintf(out, cap, "%s in row %llu at byte %llu", kInvalidText, (unsigned long long)row, (unsigned long long)offset);
    else if (code == EXG_PE_CIGAR_RANGE)
        n = snprintf(out, cap, "%s in row %llu", kRangeText, (unsigned long long)row);
    else
        out[0] = 0;
    return n < 0 ? 0 : ((size_t)n < cap ? (size_t)n : cap - 1);
}

}  // namespace cigarfn
}  // namespace exg
