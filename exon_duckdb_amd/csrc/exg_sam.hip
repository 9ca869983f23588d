// exg_sam.hip — SAM record scan (read_sam_file_records): one row per alignment line, BAM's ten columns — name, flag,
// reference, start, end, mapping_quality, cigar, mate_reference, sequence, quality_score — every string a duckdb::string_t
// slice of the input (there is no side buffer), flag / start / end parsed to int32, `end` from a walk over the CIGAR text.
//
// Replaces the tokenising the reference gets from noodles-sam through exon 0.2.x (registered at
// exon/src/exon_extension.cpp:52; the ten columns pinned by test_sam_record_scan.test:6-17; the value rules are INTEGRATION.md's).
// The header (the leading '@' lines) is the reader's: it hands the scan the bytes behind it.
//
// Two implementations behind exg_sam_scan, one row function (sam_line<Src>):
//   * fused (exg_fused_core.hpp skeleton, the any-shape instance only): thread = line, fields cut out of LDS; the one line per
//     half that begins in front of the 1 KiB window — every line longer than a half among them — is left to k_sam_far behind
//     the kernel (FarRec);
//   * general: line index (exg_lines.hip) + thread = line reading global memory — the differential partner.
#include "exg_fused_core.hpp"
#include "exg_line_src.hpp"
#include "exg_lines.hpp"

namespace exg {

struct SamDev {
    const uint8_t *d_in;
    uint64_t n_bytes;
    uint64_t lead;
    uint64_t first_line_index;  // unused (kept for the core's EOF arithmetic): 0
    uint64_t payload_base;
    uint32_t flags;
    uint32_t pad;
    void *d_col[EXG_SAM_COLUMNS];  // exg_string_t[] (0, 2, 5, 6, 7, 8, 9) / int32_t[] (1, 3, 4); NULL: validated only
    uint64_t *d_valid[EXG_SAM_COLUMNS];  // columns 2, 3, 4, 5, 7
    uint64_t capacity;
};

struct SamRowInfo {
    uint32_t code;
    uint32_t valid;  // bits 0 .. 4: columns 2, 3, 4, 5, 7 are not NULL
};

static constexpr uint32_t kSamCigarLenMax = 268435455u;  // 2^28 - 1: what a BAM CIGAR operation holds

// the tabs of a line in order, 64 bytes at a time: next() = the next tab's position, `e` when the line has no more
template <class Src>
struct SamTabs {
    const Src &src;
    int base, e;  // the word `bits` came from begins at base; the line ends at e
    unsigned long long bits;
    __device__ __forceinline__ SamTabs(const Src &src_, int s, int e_) : src(src_), base(s - 64), e(e_), bits(0) {}
    __device__ __forceinline__ int next() {
        while (!bits) {
            if ((long long)e - base <= 64) {  // no word left (base stays where it is: a line may be 0x7FFFFFF0 bytes long)
                base = e;
                return e;
            }
            base += 64;
            bits = src.tabs64(base);
            const int rem = e - base;
            if (rem < 64) bits &= (1ull << rem) - 1ull;
        }
        const int pos = base + __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        return pos;
    }
};

// one or more ASCII digits, nothing else, at most `max`
template <class Src>
__device__ __forceinline__ bool sam_uint(const Src &src, int s, int e, uint32_t max, uint32_t *out) {
    if (s >= e) return false;
    unsigned long long v = 0;
    for (int i = s; i < e; i++) {
        const uint32_t d = src.b(i) - '0';
        if (d > 9u) return false;
        v = v * 10u + d;
        if (v > max) return false;
    }
    *out = (uint32_t)v;
    return true;
}

// CIGAR text [s, e), not `*`: one or more of [digits, one of MIDNSHP=X], each length <= 2^28 - 1; *span = the reference bases
// M, D, N, = and X consume
template <class Src>
__device__ inline bool sam_cigar(const Src &src, int s, int e, unsigned long long *span) {
    unsigned long long sp = 0;
    int i = s;
    while (i < e) {
        const int d0 = i;
        uint32_t v = 0;
        uint32_t c = 0;
        for (; i < e; i++) {
            c = src.b(i);
            const uint32_t d = c - '0';
            if (d > 9u) break;
            if (v > kSamCigarLenMax / 10u) return false;  // (v * 10 stays below 2^32)
            v = v * 10u + d;
            if (v > kSamCigarLenMax) return false;
        }
        if (i == d0 || i >= e) return false;  // no digits, or no operation behind them
        const bool refc = c == 'M' || c == 'D' || c == 'N' || c == '=' || c == 'X';
        if (!refc && c != 'I' && c != 'S' && c != 'H' && c != 'P') return false;
        if (refc) sp += v;
        i++;
    }
    *span = sp;
    return i > s;
}

__device__ __forceinline__ void sam_put_str(void *col, unsigned long long out, uint4 v) {
    if (col) st_stream16(reinterpret_cast<uint4 *>(col) + out, v);
}
__device__ __forceinline__ void sam_put_i32(void *col, unsigned long long out, int v) {
    if (col) __builtin_nontemporal_store(v, reinterpret_cast<int *>(col) + out);
}

// One line [s, e) (CR already stripped), stored straight to row `out` (store == false: validate only).  Precedence of the
// errors: the field count, then the fields left to right (the caller checks UTF-8 behind them).  Every store comes behind
// the last check.
template <class Src>
__device__ __forceinline__ SamRowInfo sam_line(const Src &src, int s, int e, const SamDev &a, unsigned long long out, bool store) {
    SamRowInfo r;
    r.code = 0;
    r.valid = 0;
    // t[k]: the tab that ends field k + 1 (QNAME .. SEQ: k = 0 .. 9); the first nine sit in the line's first word or two, SEQ's
    // end is searched
    SamTabs<Src> tabs(src, s, e);
    int t[10];
#pragma unroll
    for (int k = 0; k < 10; k++) t[k] = tabs.next();
    if (t[9] >= e) {  // fewer than ten tabs: fewer than eleven fields (an empty line among them)
        r.code = EXG_PE_SAM_FIELD_COUNT;
        return r;
    }
    uint32_t code = 0;
    uint32_t flag_v = 0, pos_v = 0, mapq_v = 0;
    unsigned long long span = 0;
    bool cigar_star = false;
    // QUAL [q0, qe): not searched — `*` apart, with SEQ of length L the byte L behind q0 is a tab or the line's end (the probe is
    // the length check too); on a miss SEQ is `*`, or the line is in error
    const int seq_s = t[8] + 1, L = t[9] - seq_s, q0 = t[9] + 1;
    int qe = q0;
    if (t[0] == s) code = EXG_PE_SAM_EMPTY_FIELD;
    else if (src.b(s) == '@') code = EXG_PE_SAM_HEADER_LINE;
    else if (t[1] == t[0] + 1) code = EXG_PE_SAM_EMPTY_FIELD;
    else if (!sam_uint(src, t[0] + 1, t[1], 65535u, &flag_v)) code = EXG_PE_SAM_FLAG;
    else if (t[2] == t[1] + 1) code = EXG_PE_SAM_EMPTY_FIELD;
    else if (t[3] == t[2] + 1) code = EXG_PE_SAM_EMPTY_FIELD;
    else if (!sam_uint(src, t[2] + 1, t[3], 0x7FFFFFFFu, &pos_v)) code = EXG_PE_SAM_POSITION;
    else if (t[4] == t[3] + 1) code = EXG_PE_SAM_EMPTY_FIELD;
    else if (!sam_uint(src, t[3] + 1, t[4], 255u, &mapq_v)) code = EXG_PE_SAM_MAPQ;
    else if (t[5] == t[4] + 1) code = EXG_PE_SAM_EMPTY_FIELD;
    else {
        cigar_star = t[5] - t[4] == 2 && src.b(t[4] + 1) == '*';
        if (!cigar_star && !sam_cigar(src, t[4] + 1, t[5], &span)) code = EXG_PE_SAM_CIGAR;
        else if (t[6] == t[5] + 1 || t[7] == t[6] + 1 || t[8] == t[7] + 1 || L == 0) code = EXG_PE_SAM_EMPTY_FIELD;
        else if (q0 >= e || src.b(q0) == '\t') code = EXG_PE_SAM_EMPTY_FIELD;
        else {
            // `*` is decided first — QUAL cannot hold a tab, so "*" in front of a tab or the line's end is unambiguous —: with
            // SEQ present the byte L behind q0 may well be an aux field's tab or the line's end
            const int room = e - q0;  // (> 0 here; the probe position q0 + L is formed only where it lies inside the line: a line may
                                      // be 0x7FFFFFF0 bytes long, and q0 + L of a line in error could pass 2^31)
            if (src.b(q0) == '*' && (room == 1 || src.b(q0 + 1) == '\t')) qe = q0 + 1;
            else if (L == room || (L < room && src.b(q0 + L) == '\t')) qe = q0 + L;
            else if (L == 1 && src.b(seq_s) == '*') qe = tabs.next();  // (SEQ absent, QUAL of any length: its end is searched)
            else code = EXG_PE_SAM_LENGTHS;
        }
    }
    if (code) {
        r.code = code;
        return r;
    }
    const bool ref_ok = !(t[2] - t[1] == 2 && src.b(t[1] + 1) == '*');
    const bool mate_eq = t[6] - t[5] == 2 && src.b(t[5] + 1) == '=';
    const bool mate_ok = mate_eq ? ref_ok : !(t[6] - t[5] == 2 && src.b(t[5] + 1) == '*');
    const bool start_ok = pos_v != 0;
    const long long end_v = (long long)pos_v + (long long)span - 1;
    const bool end_ok = start_ok && end_v >= 1 && end_v <= 0x7FFFFFFFll;
    const bool mapq_ok = mapq_v != 255u;
    r.valid = (ref_ok ? 1u : 0u) | (start_ok ? 2u : 0u) | (end_ok ? 4u : 0u) | (mapq_ok ? 8u : 0u) | (mate_ok ? 16u : 0u);
    if (store) {
        const uint4 z = make_uint4(0, 0, 0, 0);
        sam_put_str(a.d_col[0], out, src.str(s, (uint32_t)(t[0] - s)));
        sam_put_i32(a.d_col[1], out, (int)flag_v);
        const uint4 ref = ref_ok ? src.str(t[1] + 1, (uint32_t)(t[2] - t[1] - 1)) : z;
        sam_put_str(a.d_col[2], out, ref);
        sam_put_i32(a.d_col[3], out, (int)pos_v);
        sam_put_i32(a.d_col[4], out, end_ok ? (int)end_v : 0);
        if (a.d_col[5]) {
            int ms = t[3] + 1;  // the canonical decimal text: the field's suffix behind its leading zeros
            while (ms < t[4] - 1 && src.b(ms) == '0') ms++;
            sam_put_str(a.d_col[5], out, mapq_ok ? src.str(ms, (uint32_t)(t[4] - ms)) : z);
        }
        sam_put_str(a.d_col[6], out, cigar_star ? z : src.str(t[4] + 1, (uint32_t)(t[5] - t[4] - 1)));
        sam_put_str(a.d_col[7], out, mate_eq ? ref : mate_ok ? src.str(t[5] + 1, (uint32_t)(t[6] - t[5] - 1)) : z);
        if (a.d_col[8]) sam_put_str(a.d_col[8], out, L == 1 && src.b(seq_s) == '*' ? z : src.str(seq_s, (uint32_t)L));
        if (a.d_col[9]) sam_put_str(a.d_col[9], out, qe - q0 == 1 && src.b(q0) == '*' ? z : src.str(q0, (uint32_t)(qe - q0)));
    }
    return r;
}

__device__ __forceinline__ void sam_report(ScanWsHeader *hdr, uint32_t code, unsigned long long out, uint64_t line_off) {
    atomicMin(&hdr->err_word, (out << 8) | (code & 0x7Fu));
    atomicMin(&hdr->err_off, (unsigned long long)line_off);
}
// column of validity bit b
__device__ __forceinline__ constexpr int sam_valid_col(int b) { return b == 0 ? 2 : b == 1 ? 3 : b == 2 ? 4 : b == 3 ? 5 : 7; }
// the five validity words (columns 2, 3, 4, 5, 7) of 64 consecutive rows from out_base on: five ballots
__device__ __forceinline__ void sam_store_validity(const SamDev &a, uint32_t valid, long long out_base, uint32_t lane) {
#pragma unroll
    for (int b = 0; b < 5; b++) store_validity64(a.d_valid[sam_valid_col(b)], __ballot((valid >> b) & 1u), out_base, lane);
}

// ---- fused: the any-shape scan ------------------------------------------------------------------------------
#ifndef EXG_SAM_HALVES_FULL
#define EXG_SAM_HALVES_FULL 2
#endif
#ifndef EXG_SAM_WAVES_FULL
#define EXG_SAM_WAVES_FULL 4
#endif
#ifndef EXG_SAM_NL_CAP
#define EXG_SAM_NL_CAP 1024
#endif
struct SamFormat {
    using Dev = SamDev;
    static constexpr int kNlCap = EXG_SAM_NL_CAP;  // the densest valid line is 22 bytes with its LF: 744 per half
    static constexpr int kHalves = EXG_SAM_HALVES_FULL;  // (no lean instance: only kFullPrimary is instantiated)
    static constexpr int kHalvesFull = EXG_SAM_HALVES_FULL;
    // a line's tabs come from its 64-byte words in LDS, read when the line is cut (LdsSrc::tabs64): no '\t' map
    static constexpr bool kTabMapLean = false, kTabMapFull = false;
    static constexpr bool kBarriers = false;
    static constexpr int kMinWavesPerSimd = EXG_SAM_WAVES_FULL, kMinWavesPerSimdRedo = EXG_SAM_WAVES_FULL;
    static constexpr int kMinWavesPerSimdFull = EXG_SAM_WAVES_FULL;
    __device__ static __forceinline__ uint32_t eof_extra_lines(unsigned long long) { return 0; }
    __device__ static __forceinline__ unsigned long long analytic_prefix(uint64_t) { return 0; }

    template <int kMode, class L>
    __device__ static __forceinline__ void emit_half(const L &s, const SamDev &a, ScanWsHeader *hdr, const TileCtx &c, unsigned long long halo_nl,
                                                     uint32_t dev_mode, uint32_t lane, uint32_t wave, unsigned long long *__restrict__ tile_qend,
                                                     uint64_t tile_index) {
        static_assert(kMode == kFullPrimary, "the SAM scan has the any-shape instance only");
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
                    // its row is k_sam_far's
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
                    SamRowInfo r = sam_line(src, s0, e1, a, (unsigned long long)out, !no_store && dev_mode != 2);
                    if (!r.code && c.non_ascii && !utf8_valid_lds(s, s0, e1)) r.code = EXG_PE_INVALID_UTF8;  // noodles reads lines into a String
                    if (r.code) sam_report(hdr, r.code, (unsigned long long)out, c.tile_off + s0 - kWin);
                    else valid = r.valid;
                }
            }
            if (!no_store) sam_store_validity(a, valid, (long long)(c.P + jb + wave * 64) - (long long)halo_nl, lane);
        }
    }
};

// ---- general path: thread = line, bytes from global memory -----------------------------------------------
__global__ __launch_bounds__(256) void k_sam_lines(SamDev a, const uint64_t *__restrict__ nl_pos, ScanWsHeader *hdr) {
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
                sam_report(hdr, EXG_PE_FIELD_TOO_LONG, out, s0);
            } else {
                if (s0 > e1) s0 = e1;
                const bool virt = e1 >= a.n_bytes;
                if (!virt && e1 > s0 && a.d_in[e1 - 1] == '\r') e1--;
                const GlobalSrc src{a.d_in, s0, a.payload_base, (a.n_bytes + 15) & ~15ull};
                SamRowInfo r = sam_line(src, 0, (int)(e1 - s0), a, out, !no_store);
                if (!r.code && (hdr->flags & EXG_RF_NON_ASCII) && !utf8_valid_global(a.d_in, s0, e1)) r.code = EXG_PE_INVALID_UTF8;
                if (r.code) sam_report(hdr, r.code, out, s0);
                else valid = r.valid;
            }
        }
        if (!no_store) sam_store_validity(a, valid, (long long)(it * 64) - (long long)halo, lane_id());
    }
}

// The rows k_fused<SamFormat> left out: one line per marked half (it begins in front of the half's window — a long read's
// line always does), read from global memory like the general path reads its lines.  Runs behind k_fused on the stream.
template <uint32_t kHalves>
__global__ __launch_bounds__(256) void k_sam_far(SamDev a, const unsigned int *__restrict__ tileA, const int32_t *__restrict__ tileL,
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
            sam_report(hdr, EXG_PE_FIELD_TOO_LONG, out, s0);
            continue;
        }
        if (s0 > e1) s0 = e1;
        const bool virt = e1 >= a.n_bytes;
        if (!virt && e1 > s0 && a.d_in[e1 - 1] == '\r') e1--;
        const GlobalSrc src{a.d_in, s0, a.payload_base, (a.n_bytes + 15) & ~15ull};
        SamRowInfo r = sam_line(src, 0, (int)(e1 - s0), a, out, !no_store);
        if (!r.code && tiles_non_ascii(tileA, kSuper, (int64_t)s0, (int64_t)e1) && !utf8_valid_global(a.d_in, s0, e1)) r.code = EXG_PE_INVALID_UTF8;
        if (r.code) {
            sam_report(hdr, r.code, out, s0);
        } else if (!no_store) {
#pragma unroll
            for (int b = 0; b < 5; b++)
                if (((r.valid >> b) & 1u) && a.d_valid[sam_valid_col(b)])
                    atomicOr((unsigned long long *)&a.d_valid[sam_valid_col(b)][out >> 6], 1ull << (out & 63));
        }
    }
}

// Result block.  fused != 0: positions come from tile_qend; else from nl_pos.
__global__ __launch_bounds__(256) void k_sam_finalize(SamDev a, ScanWsHeader *hdr, const unsigned long long *__restrict__ tile_qend,
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

static int run_sam_general(const SamDev &dev, uint8_t *ws, const FastqWsLayout &l, exg_scan_result *d_result, hipStream_t stream) {
    ScanWsHeader *hdr = reinterpret_cast<ScanWsHeader *>(ws);
    const uint64_t *nl_pos = reinterpret_cast<const uint64_t *>(ws + l.off_nl_pos);
    hipLaunchKernelGGL(k_init_hdr, dim3(1), dim3(1), 0, stream, hdr, l.lines_cap, 0u);
    const int rc = launch_line_index(dev.d_in, dev.n_bytes, dev.lead, ws, l, (dev.flags & EXG_F_EOF) ? 1 : 0, 0, stream);
    if (rc) return rc;
    const uint64_t est = dev.n_bytes / 64 + 256;
    const uint32_t grid = (uint32_t)((est + 255) / 256 < 2048 ? (est + 255) / 256 : 2048);
    hipLaunchKernelGGL(k_sam_lines, dim3(grid), dim3(256), 0, stream, dev, nl_pos, hdr);
    hipLaunchKernelGGL(k_sam_finalize, dim3(1), dim3(256), 0, stream, dev, hdr, (const unsigned long long *)nullptr, 0u, nl_pos, 0, d_result);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

static int run_sam_fused(const SamDev &dev, uint8_t *ws, const FastqWsLayout &l, exg_scan_result *d_result, hipStream_t stream) {
    ScanWsHeader *hdr = reinterpret_cast<ScanWsHeader *>(ws);
    constexpr uint32_t kHalvesHost = SamFormat::kHalvesFull;
    const uint64_t kSuperBytes = (uint64_t)kHalvesHost * kTile;
    uint64_t n_super64 = (dev.n_bytes + kSuperBytes - 1) / kSuperBytes;
    if (n_super64 == 0) n_super64 = 1;
    if (n_super64 > 0x7FFFFFF0ull / kHalvesHost) {
        set_error("exg_sam_scan: buffer too large for one launch");
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
    hipLaunchKernelGGL((k_fused<SamFormat, kFullPrimary>), dim3(n_super + 1), dim3(kThreads), 0, stream, dev, tileA, tileP, tile_qend, hdr, n_super);
    // the rows of lines that begin in front of their half's window (returns at once when there is none)
    const uint32_t n_halves = n_super * kHalvesHost;
    const uint32_t grid = (n_halves + 255) / 256 < 4096 ? (n_halves + 255) / 256 : 4096;
    hipLaunchKernelGGL(k_sam_far<SamFormat::kHalvesFull>, dim3(grid), dim3(256), 0, stream, dev, tileA, tileL, tile_qend, far_rec, hdr, n_halves);
    hipLaunchKernelGGL(k_sam_finalize, dim3(1), dim3(256), 0, stream, dev, hdr, tile_qend, n_halves, (const uint64_t *)nullptr, 1, d_result);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

}  // namespace exg

using namespace exg;

extern "C" int exg_sam_scan(const exg_sam_scan_args *a) {
    if (!a || !a->d_result || !a->d_workspace || ((uintptr_t)a->d_workspace & 255) || (a->n_bytes && !a->d_input) ||
        ((uintptr_t)a->d_input & 15) || a->lead > a->n_bytes) {
        set_error("exg_sam_scan: bad arguments (null pointer, unaligned input or workspace, or lead > n_bytes)");
        return EXG_E_INVALID_ARG;
    }
    if (a->flags & ~EXG_F_ALL) {
        set_error("exg_sam_scan: unknown flag bits 0x%x", a->flags & ~EXG_F_ALL);
        return EXG_E_INVALID_ARG;
    }
    if (a->algo == EXG_ALGO_FUSED_INDEX || a->algo > EXG_ALGO_FUSED_INDEX) {
        set_error("exg_sam_scan: algo %u is not one of the SAM scan's (EXG_ALGO_FUSED_INDEX is exg_vcf_scan's alone)", a->algo);
        return EXG_E_INVALID_ARG;
    }
    const FastqWsLayout l = fastq_ws_layout(a->n_bytes, a->workspace_bytes);
    if (a->workspace_bytes < fastq_ws_layout(a->n_bytes, 0).off_nl_pos + 64) {
        set_error("exg_sam_scan: workspace too small");
        return EXG_E_INVALID_ARG;
    }
    static const bool kHasValidity[EXG_SAM_COLUMNS] = {false, false, true, true, true, true, false, true, false, false};
    SamDev dev;
    dev.d_in = (const uint8_t *)a->d_input;
    dev.n_bytes = a->n_bytes;
    dev.lead = a->lead;
    dev.first_line_index = 0;
    dev.payload_base = a->payload_base;
    dev.flags = a->flags;
    dev.pad = 0;
    for (int c = 0; c < EXG_SAM_COLUMNS; c++) {
        dev.d_col[c] = a->d_columns[c];
        dev.d_valid[c] = kHasValidity[c] && a->d_columns[c] ? a->d_validity[c] : nullptr;
    }
    dev.capacity = a->capacity_records;
    hipStream_t stream = (hipStream_t)a->stream;
    uint8_t *ws = (uint8_t *)a->d_workspace;
    if (a->capacity_records && !(a->flags & EXG_F_NO_STORE)) {
        const size_t vb = (size_t)((a->capacity_records + 63) / 64) * 8;
        for (int c = 0; c < EXG_SAM_COLUMNS; c++)
            if (dev.d_valid[c]) EXG_HIP_CHECK(hipMemsetAsync(dev.d_valid[c], 0, vb, stream));
    }
    if (a->algo == EXG_ALGO_MULTIPASS) return run_sam_general(dev, ws, l, a->d_result, stream);
    return run_sam_fused(dev, ws, l, a->d_result, stream);  // EXG_ALGO_AUTO, EXG_ALGO_FUSED, EXG_ALGO_FUSED_FULL: one scan
}
