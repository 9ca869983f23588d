// exg_bed.hip — BED record scan (read_bed_file): one row per line, twelve columns — reference_sequence_name, start, end,
// name, score, strand, thick_start, thick_end, color, block_count, block_sizes, block_starts — the strings as
// duckdb::string_t slices of the input, the integers parsed to int64 (start and thick_start + 1: BED is 0-based, the
// reference's rows are 1-based).
//
// Replaces the tokenising the reference gets from noodles-bed 0.10.0 through exon 0.2.6 (registered at
// exon/src/exon_extension.cpp:47-58; column order pinned by test_bed_io.test:4-18; the value rules are INTEGRATION.md's).
//
// Two implementations behind exg_bed_scan, one row function (bed_line<Src>):
//   * fused (exg_fused_core.hpp skeleton, the any-shape instance only): thread = line, fields cut out of LDS; a half with more
//     lines than its list holds is emitted in passes (the shortest line, "c\t1\t2\n", gives 2 730 lines per 16 KiB half); the one
//     line per half that begins in front of the 1 KiB window is left to k_bed_far behind the kernel (FarRec);
//   * general: line index (exg_lines.hip) + thread = line reading global memory — the differential partner.
// Every line of the input is a record: there is no header, so `lead` is only a shard's halo.
#include "exg_fused_core.hpp"
#include "exg_line_src.hpp"
#include "exg_lines.hpp"

#include "exg_parse.hpp"

namespace exg {

struct BedDev {
    const uint8_t *d_in;
    uint64_t n_bytes;
    uint64_t lead;
    uint64_t first_line_index;  // unused (kept for the core's EOF arithmetic): 0
    uint64_t payload_base;
    uint32_t flags;
    uint32_t pad;
    void *d_col[EXG_BED_COLUMNS];  // exg_string_t[] (0, 3, 5, 8, 10, 11) / int64_t[] (1, 2, 4, 6, 7, 9); NULL: validated only
    uint64_t *d_valid[EXG_BED_COLUMNS];  // columns 3 .. 11
    uint64_t capacity;
};

struct BedRowInfo {
    uint32_t code;
    uint32_t valid;  // bit c - 3: column c (3 .. 11) is not NULL
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

__device__ __forceinline__ void bed_put_str(void *col, unsigned long long out, uint4 v) {
    if (col) st_stream16(reinterpret_cast<uint4 *>(col) + out, v);
}
__device__ __forceinline__ void bed_put_i64(void *col, unsigned long long out, long long v) {
    if (col) __builtin_nontemporal_store(v, reinterpret_cast<long long *>(col) + out);
}

// One line [s, e) (CR already stripped), stored straight to row `out` (store == false: validate only).  Precedence of the
// errors: the field count, then the fields left to right (the caller checks UTF-8 behind them).
// Everything is statically indexed (runtime-indexed arrays would live in scratch memory).
template <class Src>
__device__ __forceinline__ BedRowInfo bed_line(const Src &src, int s, int e, const BedDev &a, unsigned long long out, bool store) {
    BedRowInfo r;
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
        bed_put_str(a.d_col[0], out, src.str(s, (uint32_t)(t[0] - s)));
        bed_put_i64(a.d_col[1], out, start_v + 1);
        bed_put_i64(a.d_col[2], out, end_v);
        if (a.d_col[3]) bed_put_str(a.d_col[3], out, (valid & 1u) ? src.str(t[2] + 1, (uint32_t)(t[3] - t[2] - 1)) : z);
        bed_put_i64(a.d_col[4], out, score_v);
        if (a.d_col[5]) bed_put_str(a.d_col[5], out, (valid & 4u) ? src.str(t[4] + 1, 1u) : z);
        bed_put_i64(a.d_col[6], out, (valid & 8u) ? ts_v + 1 : 0);
        bed_put_i64(a.d_col[7], out, te_v);
        if (a.d_col[8]) bed_put_str(a.d_col[8], out, (valid & 32u) ? src.str(t[7] + 1, (uint32_t)(t[8] - t[7] - 1)) : z);
        bed_put_i64(a.d_col[9], out, bc_v);
        if (a.d_col[10]) bed_put_str(a.d_col[10], out, (valid & 128u) ? src.str(t[9] + 1, (uint32_t)(bs_end - t[9] - 1)) : z);
        if (a.d_col[11]) bed_put_str(a.d_col[11], out, (valid & 256u) ? src.str(t[10] + 1, (uint32_t)(bt_end - t[10] - 1)) : z);
    }
    return r;
}

__device__ __forceinline__ void bed_report(ScanWsHeader *hdr, uint32_t code, unsigned long long out, uint64_t line_off) {
    atomicMin(&hdr->err_word, (out << 8) | (code & 0x7Fu));
    atomicMin(&hdr->err_off, (unsigned long long)line_off);
}
// the nine validity words (columns 3 .. 11) of 64 consecutive rows from out_base on: nine ballots
__device__ __forceinline__ void bed_store_validity(const BedDev &a, uint32_t valid, long long out_base, uint32_t lane) {
#pragma unroll
    for (int b = 0; b < 9; b++) store_validity64(a.d_valid[3 + b], __ballot((valid >> b) & 1u), out_base, lane);
}

// ---- fused: the any-shape scan ------------------------------------------------------------------------------
#ifndef EXG_BED_HALVES_FULL
#define EXG_BED_HALVES_FULL 2
#endif
#ifndef EXG_BED_WAVES_FULL
#define EXG_BED_WAVES_FULL 4
#endif
#ifndef EXG_BED_NL_CAP
#define EXG_BED_NL_CAP 1024
#endif
struct BedFormat {
    using Dev = BedDev;
    static constexpr int kNlCap = EXG_BED_NL_CAP;  // BED3 lines of ~25 bytes: 650 per half; denser halves go in passes
    static constexpr int kHalves = EXG_BED_HALVES_FULL;  // (no lean instance: only kFullPrimary is instantiated)
    static constexpr int kHalvesFull = EXG_BED_HALVES_FULL;
    // a line's tabs come from its first two 64-byte words in LDS, read when the line is cut (LdsSrc::tabs64): no '\t' map
    static constexpr bool kTabMapLean = false, kTabMapFull = false;
    static constexpr bool kBarriers = false;
    static constexpr int kMinWavesPerSimd = EXG_BED_WAVES_FULL, kMinWavesPerSimdRedo = EXG_BED_WAVES_FULL;
    static constexpr int kMinWavesPerSimdFull = EXG_BED_WAVES_FULL;
    __device__ static __forceinline__ uint32_t eof_extra_lines(unsigned long long) { return 0; }
    __device__ static __forceinline__ unsigned long long analytic_prefix(uint64_t) { return 0; }

    template <int kMode, class L>
    __device__ static __forceinline__ void emit_half(const L &s, const BedDev &a, ScanWsHeader *hdr, const TileCtx &c, unsigned long long halo_nl,
                                                     uint32_t dev_mode, uint32_t lane, uint32_t wave, unsigned long long *__restrict__ tile_qend,
                                                     uint64_t tile_index) {
        static_assert(kMode == kFullPrimary, "the BED scan has the any-shape instance only");
        const uint32_t tid = threadIdx.x;  // this thread's line of a pass of 256
        unsigned long long qend_word = 0;  // (thread 0: what it stored into tile_qend)
        if (tid == 0 && (c.pass_base == 0 || c.n_lines)) {  // offset just past the last line that ends in this half (0: none)
            long long e = 0;
            if (c.n_lines) {
                e = (long long)c.tile_off + (int)s.nlist[4 + c.n_lines - 1] - kWin + 1;
                if ((unsigned long long)e > a.n_bytes) e = (long long)a.n_bytes;
            }
            if (c.pass_base) e |= (long long)(tile_qend[tile_index] & kFarBit);  // (a later pass keeps the first pass's mark)
            qend_word = (unsigned long long)e;
            tile_qend[tile_index] = qend_word;
        }
        if (dev_mode == 3 || dev_mode == 4) return;
        const bool no_store = (a.flags & EXG_F_NO_STORE) != 0;
        const LdsSrc<L> src{s, a.payload_base + c.tile_off - kWin, s.tabmap[0]};
        for (uint32_t jb = 0; jb < c.n_lines; jb += kThreads) {
            const uint32_t j = jb + tid;
            const long long out = (long long)(c.P + j) - (long long)halo_nl;
            bool act = j < c.n_lines;
            int e1 = 0;
            if (act) {
                e1 = s.nlist[4 + j];
                act = (uint64_t)((int64_t)c.tile_off + e1 - kWin) >= a.lead && out >= 0;
                if (act && !no_store && (unsigned long long)out >= a.capacity) {
                    atomicOr(&hdr->flags, EXG_RF_CAPACITY);
                    act = false;
                }
            }
            uint32_t valid = 0;
            if (act) {
                const uint32_t q0 = s.nlist[3 + j];  // newline before the line
                if (q0 == kNoneE) {
                    // the line begins in front of the LDS window (only the first line of a half's first pass can: thread 0):
                    // its row is k_bed_far's
                    FarRec f;
                    f.pos[0] = s.prev32[3];
                    f.pos[1] = c.half * kTile + e1 - kWin;
                    f.pos[2] = f.pos[3] = f.pos[4] = 0;
                    f.flags = c.is_eof_tile ? 1u : 0u;
                    f.out = out;
                    far_rec_of<false>(tile_qend, a.n_bytes)[tile_index] = f;
                    hdr->any_far = 1u;
                    tile_qend[tile_index] = qend_word | kFarBit;  // (this thread stored the word above: no load)
                } else {
                    const int s0 = (int)q0 + 1;
                    if (e1 > s0 && !(c.is_eof_tile && e1 == c.lim_e) && ldb(s, e1 - 1) == '\r') e1--;
                    BedRowInfo r = bed_line(src, s0, e1, a, (unsigned long long)out, !no_store && dev_mode != 2);
                    if (!r.code && c.non_ascii && !utf8_valid_lds(s, s0, e1)) r.code = EXG_PE_INVALID_UTF8;  // noodles reads lines into a String
                    if (r.code) bed_report(hdr, r.code, (unsigned long long)out, c.tile_off + s0 - kWin);
                    else valid = r.valid;
                }
            }
            if (!no_store) bed_store_validity(a, valid, (long long)(c.P + jb + wave * 64) - (long long)halo_nl, lane);
        }
    }
};

// ---- general path: thread = line, bytes from global memory -----------------------------------------------
__global__ __launch_bounds__(256) void k_bed_lines(BedDev a, const uint64_t *__restrict__ nl_pos, ScanWsHeader *hdr) {
    const uint64_t T = hdr->total_lines < hdr->lines_cap ? hdr->total_lines : hdr->lines_cap;
    const uint64_t halo = hdr->halo_nl;
    const bool no_store = (a.flags & EXG_F_NO_STORE) != 0;
    const uint64_t n_iter = (T + 63) / 64;
    const uint64_t wave_id = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t it = wave_id; it < n_iter; it += n_waves) {
        const uint64_t j = it * 64 + lane_id();
        bool act = j < T && j >= halo;
        const uint64_t out = j - halo;
        if (act && !no_store && out >= a.capacity) {
            atomicOr(&hdr->flags, EXG_RF_CAPACITY);
            act = false;
        }
        uint32_t valid = 0;
        if (act) {
            uint64_t e1 = nl_pos[j];
            const bool resolved = j > 0 || (a.flags & EXG_F_BOF);
            uint64_t s0 = j > 0 ? nl_pos[j - 1] + 1 : 0;
            if (!resolved) {
                atomicAdd(&hdr->n_unresolved, 1ull);
                atomicOr(&hdr->flags, EXG_RF_HEAD_UNRESOLVED);
            } else if (e1 - s0 > 0x7FFFFFF0ull) {
                bed_report(hdr, EXG_PE_FIELD_TOO_LONG, out, s0);
            } else {
                if (s0 > e1) s0 = e1;
                const bool virt = e1 >= a.n_bytes;
                if (!virt && e1 > s0 && a.d_in[e1 - 1] == '\r') e1--;
                const GlobalSrc src{a.d_in, s0, a.payload_base, (a.n_bytes + 15) & ~15ull};
                BedRowInfo r = bed_line(src, 0, (int)(e1 - s0), a, out, !no_store);
                if (!r.code && (hdr->flags & EXG_RF_NON_ASCII) && !utf8_valid_global(a.d_in, s0, e1)) r.code = EXG_PE_INVALID_UTF8;
                if (r.code) bed_report(hdr, r.code, out, s0);
                else valid = r.valid;
            }
        }
        if (!no_store) bed_store_validity(a, valid, (long long)(it * 64) - (long long)halo, lane_id());
    }
}

// The rows k_fused<BedFormat> left out: one line per marked half (it begins in front of the half's window), read from global
// memory like the general path reads its lines.  Runs behind k_fused on the stream.
template <uint32_t kHalves>
__global__ __launch_bounds__(256) void k_bed_far(BedDev a, const unsigned int *__restrict__ tileA, const int32_t *__restrict__ tileL,
                                                 const unsigned long long *__restrict__ tile_qend, const FarRec *__restrict__ far_rec,
                                                 ScanWsHeader *hdr, uint32_t n_halves) {
    if (!hdr->any_far) return;
    constexpr uint64_t kSuper = (uint64_t)kHalves * kTile;
    const bool no_store = (a.flags & EXG_F_NO_STORE) != 0;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n_halves; x += (uint64_t)gridDim.x * blockDim.x) {
        if (!(tile_qend[x] & kFarBit)) continue;
        const FarRec f = far_rec[x];
        int64_t p[2];
        const unsigned long long out = (unsigned long long)f.out;
        if (!far_positions<2>(f, (uint32_t)(x / kHalves), kSuper, tileA, tileL, (a.flags & EXG_F_BOF) != 0, p)) {
            atomicAdd(&hdr->n_unresolved, 1ull);  // the line begins in front of d_input[0]: the caller widens the halo
            atomicOr(&hdr->flags, EXG_RF_HEAD_UNRESOLVED);
            continue;
        }
        uint64_t s0 = (uint64_t)(p[0] + 1), e1 = (uint64_t)p[1];
        if (e1 - s0 > 0x7FFFFFF0ull) {
            bed_report(hdr, EXG_PE_FIELD_TOO_LONG, out, s0);
            continue;
        }
        if (s0 > e1) s0 = e1;
        const bool virt = e1 >= a.n_bytes;
        if (!virt && e1 > s0 && a.d_in[e1 - 1] == '\r') e1--;
        const GlobalSrc src{a.d_in, s0, a.payload_base, (a.n_bytes + 15) & ~15ull};
        BedRowInfo r = bed_line(src, 0, (int)(e1 - s0), a, out, !no_store);
        if (!r.code && tiles_non_ascii(tileA, kSuper, (int64_t)s0, (int64_t)e1) && !utf8_valid_global(a.d_in, s0, e1)) r.code = EXG_PE_INVALID_UTF8;
        if (r.code) {
            bed_report(hdr, r.code, out, s0);
        } else if (!no_store) {
#pragma unroll
            for (int b = 0; b < 9; b++)
                if (((r.valid >> b) & 1u) && a.d_valid[3 + b]) atomicOr((unsigned long long *)&a.d_valid[3 + b][out >> 6], 1ull << (out & 63));
        }
    }
}

// Result block.  fused != 0: positions come from tile_qend; else from nl_pos.
__global__ __launch_bounds__(256) void k_bed_finalize(BedDev a, ScanWsHeader *hdr, const unsigned long long *__restrict__ tile_qend,
                                                      uint32_t n_tiles, const uint64_t *__restrict__ nl_pos, int fused, exg_scan_result *res) {
    __shared__ unsigned long long s_qend;
    __shared__ int s_found;
    if (threadIdx.x == 0) {
        s_qend = 0;
        s_found = 0;
    }
    __syncthreads();
    if (fused) {
        for (int64_t base = (int64_t)n_tiles - 1; base >= 0; base -= 256) {
            const int64_t t = base - threadIdx.x;
            const unsigned long long q = t >= 0 ? tile_qend[t] & ~kFarBit : 0;
            if (q) atomicMax(&s_qend, q);
            if (q) s_found = 1;
            __syncthreads();
            if (s_found) break;
        }
    }
    __syncthreads();
    if (threadIdx.x) return;
    const uint64_t T = hdr->total_lines, halo = hdr->halo_nl;
    const uint64_t n_owned = T > halo ? T - halo : 0;
    uint64_t last_end = s_qend;
    if (!fused) {
        const uint64_t Tc = T < hdr->lines_cap ? T : hdr->lines_cap;
        last_end = Tc ? nl_pos[Tc - 1] + 1 : 0;
        if (last_end > a.n_bytes) last_end = a.n_bytes;
    }
    exg_scan_result r;
    r.n_lines = n_owned;
    r.flags = hdr->flags;
    if (!fused && T > hdr->lines_cap) r.flags |= EXG_RF_INDEX_OVERFLOW;
    r.payload_bytes = 0;
    r.redo_tiles = 0;
    r.error_code = 0;
    r.error_offset = ~0ull;
    r.error_record = ~0ull;
    uint64_t n_rec = (n_owned < a.capacity || (a.flags & EXG_F_NO_STORE)) ? n_owned : a.capacity;
    uint64_t consumed = last_end > a.lead ? last_end : a.lead;
    const unsigned long long err = hdr->err_word;
    if (err != kNoError) {
        const uint64_t rec = err >> 8;
        r.error_code = (uint32_t)(err & 0xFF);
        r.error_record = rec;
        r.error_offset = hdr->err_off;
        if (rec < n_rec) {
            n_rec = rec;
            consumed = hdr->err_off > a.lead ? hdr->err_off : a.lead;
        }
    }
    r.n_records = n_rec;
    r.consumed_bytes = n_rec ? consumed : a.lead;
    *res = r;
}

__global__ void k_init_hdr(ScanWsHeader *hdr, uint64_t lines_cap, uint32_t mode);

static int run_bed_general(const BedDev &dev, uint8_t *ws, const FastqWsLayout &l, exg_scan_result *d_result, hipStream_t stream) {
    ScanWsHeader *hdr = reinterpret_cast<ScanWsHeader *>(ws);
    const uint64_t *nl_pos = reinterpret_cast<const uint64_t *>(ws + l.off_nl_pos);
    hipLaunchKernelGGL(k_init_hdr, dim3(1), dim3(1), 0, stream, hdr, l.lines_cap, 0u);
    const int rc = launch_line_index(dev.d_in, dev.n_bytes, dev.lead, ws, l, (dev.flags & EXG_F_EOF) ? 1 : 0, 0, stream);
    if (rc) return rc;
    const uint64_t est = dev.n_bytes / 32 + 256;
    const uint32_t grid = (uint32_t)((est + 255) / 256 < 2048 ? (est + 255) / 256 : 2048);
    hipLaunchKernelGGL(k_bed_lines, dim3(grid), dim3(256), 0, stream, dev, nl_pos, hdr);
    hipLaunchKernelGGL(k_bed_finalize, dim3(1), dim3(256), 0, stream, dev, hdr, (const unsigned long long *)nullptr, 0u, nl_pos, 0, d_result);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

static int run_bed_fused(const BedDev &dev, uint8_t *ws, const FastqWsLayout &l, exg_scan_result *d_result, hipStream_t stream) {
    ScanWsHeader *hdr = reinterpret_cast<ScanWsHeader *>(ws);
    constexpr uint32_t kHalvesHost = BedFormat::kHalvesFull;
    const uint64_t kSuperBytes = (uint64_t)kHalvesHost * kTile;
    uint64_t n_super64 = (dev.n_bytes + kSuperBytes - 1) / kSuperBytes;
    if (n_super64 == 0) n_super64 = 1;
    if (n_super64 > 0x7FFFFFF0ull / kHalvesHost) {
        set_error("exg_bed_scan: buffer too large for one launch");
        return EXG_E_INVALID_ARG;
    }
    const uint32_t n_super = (uint32_t)n_super64;
    // descriptor block (exg_fastq_ws.hpp): u64 tileA[n] (u32 counts), u64 tileP[n], u64 tile_redo[n] (unused here), u64 tile_qend[n],
    // int32 tileL[n][4], FarRec[n]
    const uint64_t n = l.n_tiles_fused;
    unsigned int *tileA = reinterpret_cast<unsigned int *>(ws + l.off_tile_desc);
    unsigned long long *tileP = reinterpret_cast<unsigned long long *>(ws + l.off_tile_desc) + n;
    unsigned long long *tile_qend = tileP + 2 * n;
    int32_t *tileL = reinterpret_cast<int32_t *>(ws + l.off_tile_last4);
    FarRec *far_rec = reinterpret_cast<FarRec *>(ws + l.off_far);
    hipLaunchKernelGGL(k_init_hdr, dim3(1), dim3(1), 0, stream, hdr, l.lines_cap, 0u);
    EXG_HIP_CHECK(hipMemsetAsync(tileA, 0, (size_t)n * 24, stream));
    if (dev.lead) {
        const int rc = exg_count_newlines(dev.d_in, 0, dev.lead, (uint64_t *)&hdr->halo_nl, stream);
        if (rc) return rc;
    }
    hipLaunchKernelGGL((k_fused<BedFormat, kFullPrimary>), dim3(n_super + 1), dim3(kThreads), 0, stream, dev, tileA, tileP, tile_qend, hdr, n_super);
    // the rows of lines that begin in front of their half's window (returns at once when there is none)
    const uint32_t n_halves = n_super * kHalvesHost;
    const uint32_t grid = (n_halves + 255) / 256 < 4096 ? (n_halves + 255) / 256 : 4096;
    hipLaunchKernelGGL(k_bed_far<BedFormat::kHalvesFull>, dim3(grid), dim3(256), 0, stream, dev, tileA, tileL, tile_qend, far_rec, hdr, n_halves);
    hipLaunchKernelGGL(k_bed_finalize, dim3(1), dim3(256), 0, stream, dev, hdr, tile_qend, n_halves, (const uint64_t *)nullptr, 1, d_result);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

}  // namespace exg

using namespace exg;

extern "C" int exg_bed_scan(const exg_bed_scan_args *a) {
    if (!a || !a->d_result || !a->d_workspace || ((uintptr_t)a->d_workspace & 255) || (a->n_bytes && !a->d_input) ||
        ((uintptr_t)a->d_input & 15) || a->lead > a->n_bytes) {
        set_error("exg_bed_scan: bad arguments (null pointer, unaligned input or workspace, or lead > n_bytes)");
        return EXG_E_INVALID_ARG;
    }
    if (a->flags & ~EXG_F_ALL) {
        set_error("exg_bed_scan: unknown flag bits 0x%x", a->flags & ~EXG_F_ALL);
        return EXG_E_INVALID_ARG;
    }
    if (a->algo == EXG_ALGO_FUSED_INDEX || a->algo > EXG_ALGO_FUSED_INDEX) {
        set_error("exg_bed_scan: algo %u is not one of the BED scan's (EXG_ALGO_FUSED_INDEX is exg_vcf_scan's alone)", a->algo);
        return EXG_E_INVALID_ARG;
    }
    const FastqWsLayout l = fastq_ws_layout(a->n_bytes, a->workspace_bytes);
    if (a->workspace_bytes < fastq_ws_layout(a->n_bytes, 0).off_nl_pos + 64) {
        set_error("exg_bed_scan: workspace too small");
        return EXG_E_INVALID_ARG;
    }
    BedDev dev;
    dev.d_in = (const uint8_t *)a->d_input;
    dev.n_bytes = a->n_bytes;
    dev.lead = a->lead;
    dev.first_line_index = 0;
    dev.payload_base = a->payload_base;
    dev.flags = a->flags;
    dev.pad = 0;
    for (int c = 0; c < EXG_BED_COLUMNS; c++) {
        dev.d_col[c] = a->d_columns[c];
        dev.d_valid[c] = c >= 3 && a->d_columns[c] ? a->d_validity[c] : nullptr;
    }
    dev.capacity = a->capacity_records;
    hipStream_t stream = (hipStream_t)a->stream;
    uint8_t *ws = (uint8_t *)a->d_workspace;
    if (a->capacity_records && !(a->flags & EXG_F_NO_STORE)) {
        const size_t vb = (size_t)((a->capacity_records + 63) / 64) * 8;
        for (int c = 3; c < EXG_BED_COLUMNS; c++)
            if (dev.d_valid[c]) EXG_HIP_CHECK(hipMemsetAsync(dev.d_valid[c], 0, vb, stream));
    }
    if (a->algo == EXG_ALGO_MULTIPASS) return run_bed_general(dev, ws, l, a->d_result, stream);
    return run_bed_fused(dev, ws, l, a->d_result, stream);  // EXG_ALGO_AUTO, EXG_ALGO_FUSED, EXG_ALGO_FUSED_FULL: one scan
}
