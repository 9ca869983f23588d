// exg_alignfn.hpp — the rules of alignment_score / alignment_score_wfa_gap_affine and of alignment_string /
// alignment_string_wfa_gap_affine, stated ONCE for the device ops (exg_alignfn.hip, exg_alignstr.hip), the host scalars
// (exon_table_function.hpp, which the DuckDB shim registers) and the C-ABI's error text.
// Plain C++: no HIP, no DuckDB; usable from host and device code.
//
// Reference: exon/src/exon/alignment_functions/module.cpp:264-329 (WFAligner::alignEnd2End + getAlignmentScore of WFA2-lib, an
// absent submodule) and module.hpp:48 (the default bind data).  INTEGRATION.md, "Alignment scores", carries the same rules.
//   penalty(text, pattern; x, o, e)   the minimum over global (end-to-end) alignments of 0 per equal byte pair, x per unequal
//                                     pair and o + L * e per gap of L bytes on either side (WFA's convention: opening is
//                                     charged on top of the first extension)
//   score                             (float)(-(int32_t)penalty); the empty pair scores +0.0f
//   bytes                             compared as bytes: case-sensitive, any value, N equals N; text and pattern are symmetric
//   defaults                          x = 4, o = 6, e = 2
//   limits                            1 <= x <= 1023, 0 <= o <= 1023, 1 <= e <= 1023, |text| + |pattern| <= 2^21
//   memory_model                      memory_high, memory_med or memory_low; no effect on the result
//   match                             0 only: > 0 is the reference's error, < 0 is refused (WFA2's conversion is unknown here)
// The wavefront recurrences (offsets h = text position per diagonal k = h - v, kNone = no alignment ends there):
//   I[s,k] = max(M[s-o-e,k-1], I[s-e,k-1]) + 1      D[s,k] = max(M[s-o-e,k+1], D[s-e,k+1])
//   M[s,k] = extend(max(M[s-x,k] + 1, I[s,k], D[s,k]))     offsets that leave the n x m rectangle are discarded
//   penalty = the first s with M[s, n - m] >= n; never more than 2o + e(n + m) (delete one string, insert the other)
//
// alignment_string(text, pattern[, [match,] mismatch, gap_opening, gap_extension, memory_model]) -> VARCHAR
// Reference: module.cpp:150-247 (alignEndsFree(pattern, 0, 0, text, 0, 0): every free end is 0, so the alignment is global;
// getAlignmentCigar + compressCigarString), module.hpp:31-38 (the two-argument form: 4 / 6 / 2).  INTEGRATION.md, "Alignment
// strings", carries the same rules.
//   axes      argument 0 is `text` (offset h), argument 1 is `pattern` (offset v)
//   letters   one per alignment column: M an equal pair, X an unequal pair, I consumes a text byte (the I state: k-1 -> k,
//             h + 1), D consumes a pattern byte (the D state: k+1 -> k)
//   result    the run-length form <count><letter>...; the empty pair gives the empty string; only M, X, I and D appear
//   optimum   optimal alignments are not unique and WFA2-lib is not in the reference tree: the rule is OURS and deterministic,
//             the backtrace over the furthest-reaching wavefronts of cell(), from M at (s = penalty, k = n - m, h = n):
//     in M at (s, k) with offset h   sub = in_rect(M[s-x,k] + 1), ins = I[s,k], del = D[s,k], pre = max of the three; emit
//                                    h - pre matches (at s = 0: h matches, stop); the first candidate that equals pre, in the
//                                    order  sub: emit X, s -= x, h = pre - 1, stay in M   del: go to D   ins: go to I
//     in D at (s, k, h)              emit D; candidates D[s-e,k+1] (extend) and M[s-o-e,k+1] (open), extend first; k += 1;
//                                    D and s -= e on extend, M and s -= o + e on open
//     in I at (s, k, h)              emit I; candidates I[s-e,k-1] + 1 (extend) and M[s-o-e,k-1] + 1 (open), extend first;
//                                    k -= 1, h -= 1; I and s -= e on extend, M and s -= o + e on open
//             the emitted letters are reversed and run-length encoded.  An entry outside a step's visited diagonals is kNone.
//   match     <= 0 is supported (> 0 is the reference's error): with a = match, minimising a #M + x #X + o #gaps + e gaplen
//             under n + m = 2 #M + 2 #X + gaplen is minimising with x' = 2x - 2a, o' = 2o, e' = 2e - a and match 0; the rule
//             runs on (x', o', e'), and both (x, o, e) and (x', o', e') must pass params_ok
//   limits    those of the score; the host scalar keeps every wavefront over its visited diagonals and refuses a history above
//             1 GiB (kHistoryLimitText)
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "exon_gpu.h"

#if defined(__HIPCC__)
#define EXG_ALN_HD __host__ __device__ inline
#else
#define EXG_ALN_HD inline
#endif

namespace exg {
namespace alignfn {

static constexpr int32_t kDefaultMismatch = 4, kDefaultGapOpening = 6, kDefaultGapExtension = 2;  // module.hpp:48
static constexpr int32_t kMaxParam = 1023;
static constexpr uint64_t kMaxPairBytes = 1ull << 21;  // 2o + e(n + m) stays below 2^31 for every allowed o and e

EXG_ALN_HD constexpr bool params_ok(int64_t x, int64_t o, int64_t e) {
    return x >= 1 && x <= kMaxParam && o >= 0 && o <= kMaxParam && e >= 1 && e <= kMaxParam;
}
// wavefronts kept: M of the scores s - max(x, o + e) .. s, I and D of s - e .. s
EXG_ALN_HD constexpr uint32_t m_ring_depth(uint32_t x, uint32_t o, uint32_t e) { return (x > o + e ? x : o + e) + 1; }
EXG_ALN_HD constexpr uint32_t gap_ring_depth(uint32_t e) { return e + 1; }
// the penalty of deleting one string and inserting the other: no optimum is larger, so no score loop runs past it
EXG_ALN_HD constexpr uint32_t penalty_bound(uint32_t o, uint32_t e, uint64_t n, uint64_t m) {
    return n + m ? (uint32_t)(2 * o + e * (n + m)) : 0u;
}
EXG_ALN_HD float score_of(uint32_t penalty) { return (float)(-(int32_t)penalty); }

// one cell of a wavefront.  Offsets are text positions h on diagonal k = h - v; kNone marks "nothing ends here" and stays
// below 0 under the + 1 of the recurrences because every stored offset went through in_rect.
static constexpr int32_t kNone = -30000;
EXG_ALN_HD constexpr int32_t in_rect(int32_t h, int32_t k, int32_t n, int32_t m) {
    return (h >= 0 && h <= n && h - k >= 0 && h - k <= m) ? h : kNone;
}
EXG_ALN_HD constexpr int32_t max2(int32_t a, int32_t b) { return a > b ? a : b; }
struct Cell {
    int32_t i, d, m;  // m: before extend
};
// m_open_* = M[s-o-e] at k-1 / k+1, i_left = I[s-e,k-1], d_right = D[s-e,k+1], m_sub = M[s-x,k]
EXG_ALN_HD constexpr Cell cell(int32_t m_open_left, int32_t i_left, int32_t m_open_right, int32_t d_right, int32_t m_sub, int32_t k,
                               int32_t n, int32_t m) {
    const int32_t i = in_rect(max2(m_open_left, i_left) + 1, k, n, m);
    const int32_t d = in_rect(max2(m_open_right, d_right), k, n, m);
    const int32_t sub = in_rect(m_sub + 1, k, n, m);
    return Cell{i, d, max2(sub, max2(i, d))};
}
// how many of the 8 bytes of a and b (little endian: byte 0 first) are equal from the front
EXG_ALN_HD uint32_t equal_prefix8(uint64_t a, uint64_t b) {
    const uint64_t x = a ^ b;
    return x ? (uint32_t)__builtin_ctzll(x) >> 3 : 8u;
}

// ---- the SQL surface's argument rules (module.cpp:53-133, by position as the signatures name them) ----
static constexpr const char *kMatchPositiveText = "Match score must be negative or zero.";  // module.cpp:101
static constexpr const char *kMatchNegativeText =
    "alignment_score: a match score below 0 is not supported here (only match = 0: WFA2's conversion of penalties and of the "
    "returned score cannot be read in the reference tree)";
static constexpr const char *kParamRangeText =
    "alignment_score: mismatch must be in 1..1023, gap_opening in 0..1023 and gap_extension in 1..1023";
inline bool memory_model_ok(const char *s, size_t n) {
    return (n == 11 && !memcmp(s, "memory_high", 11)) || (n == 10 && (!memcmp(s, "memory_med", 10) || !memcmp(s, "memory_low", 10)));
}
static constexpr const char *kMemoryModelPrefix = "Invalid memory model: ";  // module.cpp:91, :130

// the text of EXG_PE_ALIGN_TOO_LONG; returns the number of bytes written (no terminator counted)
inline size_t format_error(uint32_t code, uint64_t length, uint64_t limit, char *out, size_t cap) {
    if (!cap) return 0;
    int n = 0;
    if (code == EXG_PE_ALIGN_TOO_LONG)
        n = snprintf(out, cap, "Alignment pair too long: %llu bytes (at most %llu)", (unsigned long long)length, (unsigned long long)limit);
    else
        out[0] = 0;
    return n < 0 ? 0 : ((size_t)n < cap ? (size_t)n : cap - 1);
}


// ---- alignment_string: the backtrace, shared by the host scalar and the kernel the way they share cell() ----
static constexpr const char *kStringParamRangeText =
    "alignment_string: mismatch must be in 1..1023, gap_opening in 0..1023 and gap_extension in 1..1023, also after a match "
    "score below 0 is folded in (2 * mismatch - 2 * match, 2 * gap_opening, 2 * gap_extension - match)";
static constexpr const char *kHistoryLimitText = "alignment_string: the alignment's wavefronts exceed 1 GiB";
static constexpr uint64_t kHostHistoryBytes = 1ull << 30;
// a match score a <= 0 folded into the penalties (header comment: match)
EXG_ALN_HD constexpr int64_t fold_mismatch(int64_t a, int64_t x) { return 2 * x - 2 * a; }
EXG_ALN_HD constexpr int64_t fold_gap_opening(int64_t, int64_t o) { return 2 * o; }
EXG_ALN_HD constexpr int64_t fold_gap_extension(int64_t a, int64_t e) { return 2 * e - a; }

// the diagonals a step at score s visits, at most: diagonal k needs s >= o + |k| e, and a step looks one beyond either side
EXG_ALN_HD constexpr uint64_t step_width_bound(uint64_t s, uint32_t e, uint64_t max_pair_bytes) {
    return 2 * (s / e) + 3 < max_pair_bytes + 1 ? 2 * (s / e) + 3 : max_pair_bytes + 1;
}
// the sum of step_width_bound over s = 0 .. P in closed form: what one of M, I, D takes in a history that never overflows
EXG_ALN_HD constexpr uint64_t history_entries(uint32_t e, uint64_t max_pair_bytes, uint64_t P) {
    const uint64_t W = max_pair_bytes + 1, Q = P / e;
    const uint64_t under = W >= 3 ? (W - 3) / 2 + 1 : 0;  // the q = s / e with 2q + 3 <= W
    const uint64_t a = Q < under ? Q : under;             // of the Q whole groups of e steps
    const uint64_t whole = a * a + 2 * a + (Q - a) * W;   // sum over q < Q of min(W, 2q + 3)
    const uint64_t last = 2 * Q + 3 < W ? 2 * Q + 3 : W;
    return e * whole + (P - Q * e + 1) * last;
}
// the largest penalty a row of a call can reach: the cap, or the bound of the longest admissible pair
EXG_ALN_HD constexpr uint32_t history_steps(uint32_t o, uint32_t e, uint64_t max_pair_bytes, uint32_t max_penalty) {
    const uint32_t bound = penalty_bound(o, e, max_pair_bytes, 0);
    return max_penalty && max_penalty < bound ? max_penalty : bound;
}

enum : uint32_t { kBtM = 0, kBtI = 1, kBtD = 2, kBtDone = 3, kBtBad = 4 };
struct BtState {
    int32_t s, k, h;
    uint32_t st;
};
struct BtStep {
    BtState next;
    int32_t matches;  // emitted first (they lie behind the operation in the alignment)
    char op;          // then this letter, 0 = none
};
// One step of the rule.  W gives the stored wavefronts: w.m(s, k), w.i(s, k), w.d(s, k), kNone for s < 0 and outside a step's
// visited diagonals.  kBtBad: the history contradicts itself (a defect, never expected).
template <class W>
EXG_ALN_HD BtStep backtrace_step(const W &w, const BtState &z, int32_t x, int32_t o, int32_t e, int32_t n, int32_t m) {
    BtStep r{z, 0, 0};
    if (z.st == kBtM) {
        if (z.s == 0) {
            r.matches = z.h, r.next.st = kBtDone;
            return r;
        }
        const int32_t sub = in_rect(w.m(z.s - x, z.k) + 1, z.k, n, m), ins = w.i(z.s, z.k), del = w.d(z.s, z.k);
        const int32_t pre = max2(sub, max2(ins, del));
        if (pre < 0 || pre > z.h) {
            r.next.st = kBtBad;
            return r;
        }
        r.matches = z.h - pre, r.next.h = pre;
        if (sub == pre)
            r.op = 'X', r.next.s -= x, r.next.h = pre - 1;
        else
            r.next.st = del == pre ? kBtD : kBtI;
        return r;
    }
    const bool del = z.st == kBtD;
    const int32_t k = del ? z.k + 1 : z.k - 1, step = del ? 0 : 1;
    const int32_t ext = (del ? w.d(z.s - e, k) : w.i(z.s - e, k)) + step, opn = w.m(z.s - o - e, k) + step;
    r.op = del ? 'D' : 'I', r.next.k = k, r.next.h = z.h - step;
    if (ext == z.h)
        r.next.s -= e;
    else if (opn == z.h)
        r.next.s -= o + e, r.next.st = kBtM;
    else
        r.next.st = kBtBad;
    return r;
}
// The run-length text, written backwards from `end` (the backtrace emits the alignment's last column first): add() takes the
// letters in emission order, finish() returns where the text begins.  At most 2 (n + m) bytes: a run's text is at most twice
// the bytes it covers; the area must hold ten bytes more (flush wants room for the longest run before it writes any).
struct RunWriter {
    uint8_t *at, *floor;  // the text begins at `at`; nothing is written below `floor`
    uint32_t count;
    char letter;
    bool overflow;
    EXG_ALN_HD void flush() {
        if (!count) return;
        if (at - floor < 11) {  // a letter and ten digits: a defect (the area holds 2 (n + m) bytes), never expected
            overflow = true;
            return;
        }
        *--at = (uint8_t)letter;
        for (uint32_t c = count; c; c /= 10) *--at = (uint8_t)('0' + c % 10);
    }
    EXG_ALN_HD void add(char op, uint32_t times) {
        if (!times) return;
        if (op != letter) flush(), letter = op, count = 0;
        count += times;
    }
    EXG_ALN_HD uint8_t *finish() {
        flush(), count = 0;
        return at;
    }
};
// the whole backtrace of a pair of penalty s into rw; false: kBtBad
template <class W>
EXG_ALN_HD bool backtrace(const W &w, int32_t s, int32_t x, int32_t o, int32_t e, int32_t n, int32_t m, RunWriter *rw) {
    BtState z{s, n - m, n, kBtM};
    while (z.st < kBtDone) {
        const BtStep step = backtrace_step(w, z, x, o, e, n, m);
        if (step.next.st == kBtBad) return false;
        rw->add('M', (uint32_t)step.matches);
        if (step.op) rw->add(step.op, 1);
        z = step.next;
    }
    rw->finish();
    return !rw->overflow;
}

}  // namespace alignfn
}  // namespace exg
