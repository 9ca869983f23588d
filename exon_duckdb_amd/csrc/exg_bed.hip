// exg_bed.hip — BED record scan (read_bed_file): one row per line, twelve columns — reference_sequence_name, start, end,
// name, score, strand, thick_start, thick_end, color, block_count, block_sizes, block_starts — the strings as
// duckdb::string_t slices of the input, the integers parsed to int64 (start and thick_start + 1: BED is 0-based, the
// reference's rows are 1-based).
//
// Replaces the tokenising the reference gets from noodles-bed 0.10.0 through exon 0.2.6 (registered at
// exon/src/exon_extension.cpp:47-58; column order pinned by test_bed_io.test:4-18; the value rules are INTEGRATION.md's).
//
// The driver around the row function (BedRows::line<Src>) is exg_line_rows.hpp's: the fused any-shape scan — a half with more lines
// than its list holds is emitted in passes (the shortest line, "c\t1\t2\n", gives 2 730 lines per 16 KiB half) — and the
// general path, its differential partner.
// Every line of the input is a record: there is no header, so `lead` is only a shard's halo.
#include "exg_line_rows.hpp"

#include "exg_parse.hpp"

namespace exg {

// d_col: exg_string_t[] (0, 3, 5, 8, 10, 11) / int64_t[] (1, 2, 4, 6, 7, 9); RowInfo::valid bit c - 3: column c (3 .. 11) is not NULL
using BedRowsDev = LineRowsDev<EXG_BED_COLUMNS>;

// ---- the format, for the driver (exg_line_rows.hpp) ----------------------------------------------------------
#ifndef EXG_BED_HALVES_FULL
#define EXG_BED_HALVES_FULL 2
#endif
#ifndef EXG_BED_WAVES_FULL
#define EXG_BED_WAVES_FULL 4
#endif
#ifndef EXG_BED_NL_CAP
#define EXG_BED_NL_CAP 1024
#endif
struct BedRows {
    static constexpr const char *kName = "exg_bed_scan", *kLabel = "BED";
    static constexpr int kColumns = EXG_BED_COLUMNS;
    static constexpr int kValidBits = 9;
    static constexpr int kKeepBit = -1;  // every line is a row
    __host__ __device__ static __forceinline__ constexpr int valid_col(int bit) { return 3 + bit; }
    static constexpr uint32_t kGeneralBytesPerLine = 32;
    static constexpr int kNlCap = EXG_BED_NL_CAP;  // BED3 lines of ~25 bytes: 650 per half; denser halves go in passes
    static constexpr int kHalvesFull = EXG_BED_HALVES_FULL, kWavesFull = EXG_BED_WAVES_FULL;
    template <class Src>
    __device__ static RowInfo line(const Src &src, int s, int e, const BedRowsDev &a, unsigned long long out, bool store);  // the row function, below
};

static constexpr unsigned long long kBedIntMax = 0x7FFFFFFFFFFFFFFFull;  // usize as BIGINT: 2^63 - 1

// usize::from_str (optional '+', digits) with an upper bound
template <class Src>
__device__ __forceinline__ bool bed_uint(const Src &src, int s, int e, unsigned long long max, long long *out) {
    long long v = 0;
    if (!parse_pos(src, s, e, &v) || (unsigned long long)v > max) return false;
    *out = v;
    return true;
}

// r,g,b: three u8::from_str
template <class Src>
__device__ inline bool bed_color(const Src &src, int s, int e) {
    int i = s;
    for (int k = 0; k < 3; k++) {
        if (i < e && src.b(i) == '+') i++;
        const int d0 = i;
        uint32_t v = 0;
        for (; i < e; i++) {
            const uint32_t d = src.b(i) - '0';
            if (d > 9u) break;
            v = v * 10u + d;
            if (v > 255u) return false;
        }
        if (i == d0) return false;
        if (k < 2) {
            if (i >= e || src.b(i) != ',') return false;
            i++;
        }
    }
    return i == e;
}

// block_sizes / block_starts: the first `count` comma-separated items of [s, e), each a usize; *end = where the last of
// them ends (before the separator of item count + 1, or before a trailing comma).  false: fewer items, or one is no integer
template <class Src>
__device__ inline bool bed_block_list(const Src &src, int s, int e, unsigned long long count, int *end) {
    *end = s;
    if (count == 0) return true;
    unsigned long long taken = 0;
    for (int i = s;;) {
        if (i < e && src.b(i) == '+') i++;
        const int d0 = i;
        unsigned long long v = 0;
        for (; i < e; i++) {
            const uint32_t d = src.b(i) - '0';
            if (d > 9u) break;
            if (v > 0x0CCCCCCCCCCCCCCCull || (v == 0x0CCCCCCCCCCCCCCCull && d > 7u)) return false;  // above 2^63 - 1
            v = v * 10 + d;
        }
        if (i == d0) return false;
        if (i < e && src.b(i) != ',') return false;
        if (++taken == count) {
            *end = i;
            return true;
        }
        if (i >= e) return false;
        i++;
    }
}

// One line [s, e) (CR already stripped), stored straight to row `out` (store == false: validate only).  Precedence of the
// errors: the field count, then the fields left to right (the caller checks UTF-8 behind them).
// Everything is statically indexed (runtime-indexed arrays would live in scratch memory).
template <class Src>
__device__ __forceinline__ RowInfo BedRows::line(const Src &src, int s, int e, const BedRowsDev &a, unsigned long long out, bool store) {
    RowInfo r;
    r.code = 0;
    r.valid = 0;
    // positions of the first 12 tabs (e when there are fewer): field k = [fs_k, t[k]), fs_0 = s, fs_k = t[k - 1] + 1
    int t[12];
#pragma unroll
    for (int k = 0; k < 12; k++) t[k] = e;
    int found = 0;
    const int len = e - s;
    {
        // the usual line — up to 128 bytes, or twelve tabs within its first 128 — out of two 64-byte tab masks: twelve pops
        unsigned long long tb0 = 0, tb1 = 0;
        if (len > 0) {
            tb0 = src.tabs64(s);
            if (len < 64) tb0 &= (1ull << len) - 1ull;
        }
        bool have = len <= 64 || __popcll(tb0) >= 12;
        if (!have) {
            tb1 = src.tabs64(s + 64);
            if (len < 128) tb1 &= (1ull << (len - 64)) - 1ull;
            have = len <= 128 || __popcll(tb0) + __popcll(tb1) >= 12;
        }
        if (have) {
#pragma unroll
            for (int k = 0; k < 12; k++) {
                const bool lo = tb0 != 0;
                unsigned long long w = lo ? tb0 : tb1;
                if (w) {
                    t[k] = s + (lo ? 0 : 64) + __ffsll((long long)w) - 1;
                    w &= w - 1;
                    tb0 = lo ? w : tb0;
                    tb1 = lo ? tb1 : w;
                    found++;
                }
            }
        } else {
            // a long line with few tabs in front (an oversized name): 64 bytes at a time
            for (int base = s; base < e && found < 12; base += 64) {
                unsigned long long bits = src.tabs64(base);
                const int rem = e - base;
                if (rem < 64) bits &= (1ull << rem) - 1ull;
                while (bits && found < 12) {
                    const int pos = base + __ffsll((long long)bits) - 1;
                    bits &= bits - 1;
#pragma unroll
                    for (int k = 0; k < 12; k++)
                        if (k == found) t[k] = pos;
                    found++;
                }
            }
        }
    }
    const int nf = found + 1;  // (found == 12: thirteen fields or more)
    if (nf < 3 || nf == 10 || nf == 11 || nf > 12) {
        r.code = EXG_PE_BED_FIELD_COUNT;
        return r;
    }
    if (t[0] == s) {
        r.code = EXG_PE_BED_REFERENCE_NAME;
        return r;
    }
    long long start_v = 0, end_v = 0, score_v = 0, ts_v = 0, te_v = 0, bc_v = 0;
    int bs_end = 0, bt_end = 0;
    if (!bed_uint(src, t[0] + 1, t[1], kBedIntMax - 1, &start_v) || !bed_uint(src, t[1] + 1, t[2], kBedIntMax, &end_v) || end_v < 1) {
        r.code = EXG_PE_BED_POSITION;
        return r;
    }
    uint32_t valid = 0;
    if (nf >= 4 && !(t[3] - t[2] == 2 && src.b(t[2] + 1) == '.')) valid |= 1u;
    if (nf >= 5 && !(t[4] - t[3] == 2 && src.b(t[3] + 1) == '0')) {
        if (!bed_uint(src, t[3] + 1, t[4], 1000, &score_v) || score_v < 1) {
            r.code = EXG_PE_BED_SCORE;
            return r;
        }
        valid |= 2u;
    }
    if (nf >= 6) {
        const uint32_t c = t[5] - t[4] == 2 ? src.b(t[4] + 1) : 0u;
        if (c == '+' || c == '-') valid |= 4u;
        else if (c != '.') {
            r.code = EXG_PE_BED_STRAND;
            return r;
        }
    }
    if (nf >= 7) {
        if (!bed_uint(src, t[5] + 1, t[6], kBedIntMax - 1, &ts_v)) {
            r.code = EXG_PE_BED_POSITION;
            return r;
        }
        valid |= 8u;
    }
    if (nf >= 8) {
        if (!bed_uint(src, t[6] + 1, t[7], kBedIntMax, &te_v) || te_v < 1) {
            r.code = EXG_PE_BED_POSITION;
            return r;
        }
        valid |= 16u;
    }
    if (nf >= 9 && !(t[8] - t[7] == 2 && src.b(t[7] + 1) == '0')) {
        if (!bed_color(src, t[7] + 1, t[8])) {
            r.code = EXG_PE_BED_COLOR;
            return r;
        }
        valid |= 32u;
    }
    if (nf == 12) {
        if (!bed_uint(src, t[8] + 1, t[9], kBedIntMax, &bc_v)) {
            r.code = EXG_PE_BED_POSITION;
            return r;
        }
        if (!bed_block_list(src, t[9] + 1, t[10], (unsigned long long)bc_v, &bs_end) ||
            !bed_block_list(src, t[10] + 1, t[11], (unsigned long long)bc_v, &bt_end)) {
            r.code = EXG_PE_BED_BLOCKS;
            return r;
        }
        valid |= 64u | 128u | 256u;
    }
    r.valid = valid;
    if (store) {
        const uint4 z = make_uint4(0, 0, 0, 0);
        put_str(a.d_col[0], out, src.str(s, (uint32_t)(t[0] - s)));
        put_i64(a.d_col[1], out, start_v + 1);
        put_i64(a.d_col[2], out, end_v);
        if (a.d_col[3]) put_str(a.d_col[3], out, (valid & 1u) ? src.str(t[2] + 1, (uint32_t)(t[3] - t[2] - 1)) : z);
        put_i64(a.d_col[4], out, score_v);
        if (a.d_col[5]) put_str(a.d_col[5], out, (valid & 4u) ? src.str(t[4] + 1, 1u) : z);
        put_i64(a.d_col[6], out, (valid & 8u) ? ts_v + 1 : 0);
        put_i64(a.d_col[7], out, te_v);
        if (a.d_col[8]) put_str(a.d_col[8], out, (valid & 32u) ? src.str(t[7] + 1, (uint32_t)(t[8] - t[7] - 1)) : z);
        put_i64(a.d_col[9], out, bc_v);
        if (a.d_col[10]) put_str(a.d_col[10], out, (valid & 128u) ? src.str(t[9] + 1, (uint32_t)(bs_end - t[9] - 1)) : z);
        if (a.d_col[11]) put_str(a.d_col[11], out, (valid & 256u) ? src.str(t[10] + 1, (uint32_t)(bt_end - t[10] - 1)) : z);
    }
    return r;
}

}  // namespace exg

extern "C" int exg_bed_scan(const exg_bed_scan_args *a) { return exg::line_rows_scan<exg::BedRows>(a); }
