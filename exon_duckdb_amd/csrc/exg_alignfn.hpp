// exg_alignfn.hpp — the rules of alignment_score / alignment_score_wfa_gap_affine, stated ONCE for the device op
// (exg_alignfn.hip), the host scalar (exon_table_function.hpp, which the DuckDB shim registers) and the C-ABI's error text.
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

}  // namespace alignfn
}  // namespace exg
