// exg_seqfn.hip — the sequence scalars of exon/src/exon/sequence_functions/module.cpp on a duckdb::string_t column that is
// still in HBM (include/exon_gpu.h: exg_sequence_op).  The rules are exg_seqfn.hpp's; here is the work distribution.
//
// A sequence column holds rows from 0 bytes to a whole chromosome, so the work is cut by BYTES, not by rows:
//   1. two prefix sums over the rows (exg_scan.hpp): goff = the bytes of "tile space" in front of a row — its output payload
//      for the string ops, its input bytes for gc_content; rows of up to 12 such bytes count 0 — and lidx = the number of
//      longer ("long") rows in front of it;
//   2. k_rows, a thread per row: the output string_t of every row (an inlined output is finished here, a long one gets its
//      length, prefix and pointer), the length rule of translate_dna_to_aa, gc_content of the short rows, and the dense list
//      of the long rows (lrow, loff) that the tiles search;
//   3. k_tiles: tile space is cut into 16 KiB tiles, a workgroup takes a run of neighbouring tiles: two waves find a tile's
//      first and last long row by a 64-ary search of loff (the tiles behind the first start from where the last one ended, and
//      a tile inside the row the last one ended in searches and fetches nothing), the rows' offsets and sources are staged in
//      LDS (a tile touches at most 1262 rows of 13 bytes and more), and every thread produces 16-byte groups on the payload's
//      own grid: one aligned 16-byte store from one or two (translate: three or four) aligned 16-byte loads, whatever the
//      source's alignment; a group that holds a row end takes one round per row.  A 125 MB row is 7630 tiles like 125 MB of
//      reads.  gc_content counts per row in LDS; a row inside one tile is divided there, a row that spans tiles adds once per
//      workgroup it touches to its counter in the workspace and k_gc_finish divides;
//   4. k_finish writes the 64-byte result block.
// Errors: atomicMin on (row << 32 | offset + 1), 0 in the low word for the length error, so the lowest row wins and in it
// the length error, else the leftmost byte.  Everything is integer arithmetic and fixed offsets: two runs are byte-identical.
#include "exg_common.hpp"
#include "exg_scan.hpp"
#include "exg_seqfn.hpp"
#include "exg_strcol.hpp"

namespace exg {
namespace seqfn {

static constexpr uint32_t kTile = 16384;
static constexpr uint32_t kTileRows = tile_rows(kTile);  // <= 1262
static constexpr uint32_t kGrid = 1024;  // 4 workgroups a CU: every run of tiles is resident at once

// workspace: goff | lidx | loff (n + 1 u64 each) | scan scratch | err (u64) | lrow (u32 x n) | count (u32 x n, gc_content)
struct Ws {
    uint64_t *goff, *lidx, *loff, *tmp, *err;
    uint32_t *lrow, *count;
    uint64_t bytes;
};
static Ws ws_layout(uint32_t op, uint64_t n, void *base) {
    Ws w;
    uint64_t *p = (uint64_t *)base;
    w.goff = p, p += n + 1;
    w.lidx = p, p += n + 1;
    w.loff = p, p += n + 1;
    w.tmp = p, p += xscan_tmp_entries(n);
    w.err = p, p += 1;
    w.lrow = (uint32_t *)p, p += (n + 1) / 2;
    w.count = (uint32_t *)p, p += op == EXG_SEQ_GC_CONTENT ? (n + 1) / 2 : 0;
    w.bytes = (uint64_t)((uint8_t *)p - (uint8_t *)base) + 64;
    return w;
}

__device__ __forceinline__ uint64_t tile_len(uint32_t op, uint32_t len) {
    const uint64_t w = output_length(op, len);
    return w > EXG_INLINE_LENGTH ? w : 0;
}
struct TileLenF {
    Col c;
    uint32_t op;
    __device__ __forceinline__ uint64_t operator()(uint64_t r) const { return tile_len(op, c.rows[r].x); }
};
struct LongF {
    Col c;
    uint32_t op;
    __device__ __forceinline__ uint64_t operator()(uint64_t r) const { return tile_len(op, c.rows[r].x) ? 1 : 0; }
};

// ---- a thread per row -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rows(Col c, uint32_t op, uint64_t n, Ws w, uint64_t cap, uint4 *out, uint64_t out_base,
                                              float *out_f) {
    const uint64_t total = w.goff[n];
    const bool gc = op == EXG_SEQ_GC_CONTENT;
    if (!gc && total > cap) return;
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r == 0) w.loff[w.lidx[n]] = total;
    if (r >= n) return;
    const uint4 v = c.rows[r];
    const uint32_t len = v.x, wl = (uint32_t)output_length(op, len);
    const uint8_t *src = src_of(c, r, v);
    if (wl > EXG_INLINE_LENGTH) {
        const uint64_t k = w.lidx[r];
        w.lrow[k] = (uint32_t)r;
        w.loff[k] = w.goff[r];
    }
    if (gc) {
        if (wl <= EXG_INLINE_LENGTH) {
            uint32_t cnt = 0;
            for (uint32_t i = 0; i < len; i++) cnt += is_gc(src[i]) ? 1u : 0u;
            out_f[r] = gc_ratio(cnt, len);
        }
        return;
    }
    const bool translate = op == EXG_SEQ_TRANSLATE;
    const ByteMap m = byte_map(op);
    uint64_t key = kNoError;
    if (translate && len % 3) key = r << 32;
    // the whole inlined output, or the 4-byte prefix of a long one (whose bytes the tiles validate)
    const uint32_t nb = wl > EXG_INLINE_LENGTH ? 4 : wl;
    uint32_t o[3] = {0, 0, 0};
    for (uint32_t i = 0; i < nb; i++) {
        uint32_t b;
        bool ok;
        if (translate) {
            const uint32_t x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
            ok = codon_ok(x, y, z);
            b = (uint8_t)codon_aa(codon_index(x, y, z));
        } else {
            const uint32_t x = src[i];
            ok = base_ok(m.from, x);
            b = base_to(m.to, x);
        }
        if (!ok && key == kNoError) key = (r << 32) | ((translate ? 3 * i : i) + 1);
        put_byte(o, i, b);
    }
    out[r] = wl > EXG_INLINE_LENGTH ? long_string(wl, o[0], out_base + w.goff[r]) : inline_string(wl, o);
    if (key != kNoError) atomicMin((unsigned long long *)w.err, (unsigned long long)key);
}

// ---- tiles ----------------------------------------------------------------------------------------------------
// The window of n16 x 16 bytes at address A (any alignment) from aligned 16-byte loads.  Only the bytes [A + lo, A + hi) of
// it belong to a row: an aligned block is read — whole — when it holds one of them, so every block read lies in a page the
// row lies in; the other blocks read as zeros (A itself may lie in front of the row).
template <int n16>
__device__ __forceinline__ void load_window(uintptr_t A, uint32_t lo, uint32_t hi, uint32_t (&d)[4 * n16]) {
    const uint32_t mis = (uint32_t)A & 15u;
    const uint4 *blk = reinterpret_cast<const uint4 *>(A - mis);
    uint32_t w[4 * n16 + 4];
#pragma unroll
    for (int k = 0; k <= n16; k++) {
        const int first = 16 * k - (int)mis;  // the block's first byte, relative to A
        uint4 v = make_uint4(0, 0, 0, 0);
        if (first < (int)hi && first + 16 > (int)lo) v = blk[k];
        w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
    }
    const uint32_t dw = mis >> 2, by = mis & 3u;
    uint32_t e[4 * n16 + 1];
#pragma unroll
    for (int j = 0; j <= 4 * n16; j++) e[j] = dw == 0 ? w[j] : dw == 1 ? w[j + 1] : dw == 2 ? w[j + 2] : w[j + 3];
#pragma unroll
    for (int j = 0; j < 4 * n16; j++) d[j] = __builtin_amdgcn_alignbyte(e[j + 1], e[j], by);
}
__device__ __forceinline__ uint32_t byte_of(const uint32_t *d, int i) { return (d[i >> 2] >> (8 * (i & 3))) & 0xFFu; }
// bits 4j .. 4j + 3 of a 16-bit byte mask as the four bytes 0xFF / 0x00 of dword j
__device__ __forceinline__ uint32_t dword_mask(uint32_t mask16, int j) {
    return ((((mask16 >> (4 * j)) & 15u) * 0x00204081u) & 0x01010101u) * 0xFFu;
}

enum { kBytes = 0, kCodons = 1, kGc = 2 };

template <int kKind>
__global__ __launch_bounds__(256) void k_tiles(Col c, uint32_t op, uint64_t n, Ws w, uint64_t cap, uint8_t *out, float *out_f) {
    constexpr int kIn = kKind == kCodons ? 3 : 1;  // input bytes a unit of tile space
    __shared__ uint64_t s_off[kTileRows + 1];
    __shared__ const uint8_t *s_src[kTileRows];
    __shared__ uint32_t s_row[kTileRows];
    __shared__ uint32_t s_cnt[kKind == kGc ? kTileRows : 1];
    __shared__ uint64_t s_k[2];
    __shared__ uint8_t s_aa[64];
    const uint64_t total = w.goff[n], L = w.lidx[n];
    if (kKind != kGc && total > cap) return;
    // a workgroup takes a run of neighbouring tiles: what it knows of one tile's last row serves the next
    const uint64_t n_tiles = (total + kTile - 1) / kTile, per = (n_tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t tile_begin = blockIdx.x * per, tile_end = tile_begin + per < n_tiles ? tile_begin + per : n_tiles;
    const uint32_t t = threadIdx.x;
    if (kKind == kCodons && t < 64) s_aa[t] = (uint8_t)codon_aa(t);
    const ByteMap m = byte_map(op);
    uint64_t key = kNoError;
    bool have = false;  // the three below describe the tile before: its last long row and where that row ends
    uint64_t prev_k1 = 0, prev_end = 0;
    uint32_t cnt = 0;
    for (uint64_t tile = tile_begin; tile < tile_end; tile++) {
        const uint64_t T0 = tile * kTile, T1 = T0 + kTile < total ? T0 + kTile : total;
        __syncthreads();  // the tile before is done with the staged rows
        // the last row of the tile before, when it goes on into this one (gc_content: with what was counted of it so far)
        const bool goes_on = have && prev_end > T0;
        uint64_t e_off = 0;
        const uint8_t *e_src = nullptr;
        uint32_t e_row = 0, carry = 0;
        if (goes_on) {
            e_off = s_off[cnt - 1], e_src = s_src[cnt - 1], e_row = s_row[cnt - 1];
            if (kKind == kGc) carry = s_cnt[cnt - 1];
        }
        __syncthreads();
        uint64_t k0;
        if (goes_on && prev_end >= T1) {  // that row covers the whole tile: nothing to search, nothing to fetch
            k0 = prev_k1, cnt = 1;
            if (t == 0) {
                s_off[0] = e_off, s_off[1] = prev_end, s_src[0] = e_src, s_row[0] = e_row;
                if (kKind == kGc) s_cnt[0] = carry;
            }
        } else {
            if (t < 64) {
                const uint64_t k = have ? (goes_on ? prev_k1 : prev_k1 + 1) : wave_search(w.loff, 0, L, T0);
                if (t == 0) s_k[0] = k;
            } else if (t < 128) {  // the last row is at most kTileRows behind the first
                const uint64_t hi = have && prev_k1 + kTileRows + 1 < L ? prev_k1 + kTileRows + 1 : L;
                const uint64_t k = wave_search(w.loff, have ? prev_k1 : 0, hi, T1 - 1);
                if (t == 64) s_k[1] = k;
            }
            __syncthreads();
            k0 = s_k[0];
            cnt = (uint32_t)(s_k[1] - k0 + 1);
            if (cnt > kTileRows) cnt = kTileRows;  // (cannot happen: long rows have 13 bytes and more)
            for (uint32_t i = t; i <= cnt; i += 256) s_off[i] = w.loff[k0 + i];
            for (uint32_t i = t; i < cnt; i += 256) {
                const uint32_t r = w.lrow[k0 + i];
                s_row[i] = r;
                s_src[i] = src_of(c, r, c.rows[r]);
                if (kKind == kGc) s_cnt[i] = i ? 0 : carry;
            }
        }
        __syncthreads();
        have = true, prev_k1 = k0 + cnt - 1, prev_end = s_off[cnt];
#pragma unroll 1
        for (uint32_t it = 0; it < kTile / (256 * 16); it++) {
            const uint64_t p = T0 + (uint64_t)(it * 256 + t) * 16;
            uint32_t gi = ~0u, gcnt = 0;  // gc_content: this thread's row and count
            if (p < T1) {
                uint32_t i = 0, hi = cnt;  // largest i < cnt with s_off[i] <= p
                while (hi - i > 1) {
                    const uint32_t mid = (i + hi) >> 1;
                    if (s_off[mid] <= p)
                        i = mid;
                    else
                        hi = mid;
                }
                // the group, one row's share at a time: all of it in one round unless a row ends in it
                const uint32_t lim = T1 - p < 16 ? (uint32_t)(T1 - p) : 16u;
                uint32_t o[4] = {0, 0, 0, 0}, done = 0;
                gi = i;
                do {
                    const uint64_t q = p + done;
                    while (i + 1 < cnt && s_off[i + 1] <= q) i++;
                    const uint64_t rel = q - s_off[i], left = s_off[i + 1] - q;
                    const uint32_t mm = left < lim - done ? (uint32_t)left : lim - done;
                    const uint32_t range = ((1u << (done + mm)) - 1u) & ~((1u << done) - 1u);  // the group's bytes of this row
                    // the window lies where the group would if the row filled it: unit b of the group is unit b of the window
                    const uintptr_t A = (uintptr_t)s_src[i] + kIn * rel - kIn * done;
                    uint32_t d[4 * kIn], y[4] = {0, 0, 0, 0}, bad = 0;
                    load_window<kIn>(A, kIn * done, kIn * (done + mm), d);
                    if (kKind == kGc) {
                        if (i != gi) {
                            if (gcnt) atomicAdd(&s_cnt[gi], gcnt);
                            gi = i, gcnt = 0;
                        }
#pragma unroll
                        for (int j = 0; j < 4; j++) gcnt += __popc(match4(d[j] & 0xFBFBFBFBu, 0x43434343u) & dword_mask(range, j));
                    } else {
#pragma unroll
                        for (int b = 0; b < 16; b++) {
                            uint32_t v;
                            bool ok;
                            if (kKind == kBytes) {
                                const uint32_t x = byte_of(d, b);
                                ok = base_ok(m.from, x), v = base_to(m.to, x);
                            } else {
                                const uint32_t x = byte_of(d, 3 * b), yy = byte_of(d, 3 * b + 1), z = byte_of(d, 3 * b + 2);
                                ok = codon_ok(x, yy, z), v = s_aa[codon_index(x, yy, z)];
                            }
                            bad |= ok ? 0u : 1u << b;
                            y[b >> 2] |= v << (8 * (b & 3));
                        }
                        if (range == 0xFFFFu) {
                            o[0] = y[0], o[1] = y[1], o[2] = y[2], o[3] = y[3];
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; j++) o[j] |= y[j] & dword_mask(range, j);
                        }
                        bad &= range;
                        if (bad) {
                            const uint64_t unit = rel + (uint32_t)(__ffs((int)bad) - 1) - done;
                            const uint64_t e = ((uint64_t)s_row[i] << 32) | (kIn * unit + 1);
                            key = e < key ? e : key;
                        }
                    }
                    done += mm;
                } while (done < lim);
                if (kKind != kGc) {
                    if (lim == 16) {
                        *reinterpret_cast<uint4 *>(out + p) = make_uint4(o[0], o[1], o[2], o[3]);
                    } else {
                        for (uint32_t b = 0; b < lim; b++) out[p + b] = (uint8_t)(o[b >> 2] >> (8 * (b & 3)));
                    }
                }
            }
            if (kKind == kGc) {  // a wave inside one row adds once
                const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)gi);
                if (__all(gi == first)) {
#pragma unroll
                    for (int dlt = 32; dlt; dlt >>= 1) gcnt += __shfl_xor(gcnt, dlt, 64);
                    if ((t & 63) == 0 && first != ~0u && gcnt) atomicAdd(&s_cnt[first], gcnt);
                } else if (gi != ~0u && gcnt) {
                    atomicAdd(&s_cnt[gi], gcnt);
                }
            }
        }
        if (kKind == kGc) {
            __syncthreads();
            const bool more = tile + 1 < tile_end;
            for (uint32_t i = t; i < cnt; i += 256) {
                const uint64_t a = s_off[i], b = s_off[i + 1];
                if (a >= T0 && b <= T0 + kTile) {
                    out_f[s_row[i]] = gc_ratio(s_cnt[i], (uint32_t)(b - a));
                } else if (more && i == cnt - 1 && b > T0 + kTile) {
                    // goes on into this workgroup's next tile: the count goes along (one atomic a row and workgroup)
                } else if (s_cnt[i]) {
                    atomicAdd(&w.count[s_row[i]], s_cnt[i]);
                }
            }
        }
    }
    if (kKind != kGc) wave_min_error(key, w.err, t & 63);
}

// gc_content of the rows that span tiles: their counters are complete now
__global__ __launch_bounds__(256) void k_gc_finish(Col c, uint64_t n, Ws w, float *out_f) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const uint32_t len = c.rows[r].x;
    if (len <= EXG_INLINE_LENGTH) return;
    const uint64_t a = w.goff[r];
    if (a / kTile != (a + len - 1) / kTile) out_f[r] = gc_ratio(w.count[r], len);
}

__global__ void k_finish(Col c, uint32_t op, uint64_t n, Ws w, uint64_t cap, exg_seq_result *res) {
    if (threadIdx.x || blockIdx.x) return;
    exg_seq_result r;
    memset(&r, 0, sizeof r);
    const bool gc = op == EXG_SEQ_GC_CONTENT;
    r.total_bytes = gc ? 0 : w.goff[n];
    if (!gc && r.total_bytes > cap) r.flags = EXG_RF_CAPACITY;
    const uint64_t key = *w.err;
    if (key != kNoError) {
        const uint64_t row = key >> 32;
        const uint32_t low = (uint32_t)key;
        const uint4 v = c.rows[row];
        r.error_row = row;
        r.error_length = v.x;
        if (!low) {
            r.error_code = EXG_PE_SEQ_LENGTH;
        } else {
            const uint8_t *src = src_of(c, row, v);
            const bool translate = op == EXG_SEQ_TRANSLATE;
            r.error_offset = low - 1;
            r.error_code = translate ? EXG_PE_SEQ_CODON : EXG_PE_SEQ_INVALID_CHARACTER;
            r.error_bytes[0] = src[r.error_offset];
            if (translate) r.error_bytes[1] = src[r.error_offset + 1], r.error_bytes[2] = src[r.error_offset + 2];
        }
    }
    *res = r;
}

}  // namespace seqfn
}  // namespace exg

using namespace exg;
using namespace exg::seqfn;

static_assert(sizeof(exg_seq_result) == 64, "exg_seq_result is 64 bytes");

extern "C" uint64_t exg_sequence_workspace_bytes(uint32_t op, uint64_t n_rows) { return ws_layout(op, n_rows, nullptr).bytes; }

extern "C" int exg_sequence_op(const exg_sequence_op_args *a) {
    if (!a || !a->d_result || ((uintptr_t)a->d_result & 7) || !a->d_workspace || ((uintptr_t)a->d_workspace & 7) ||
        (a->n_rows && !a->d_strings) || ((uintptr_t)a->d_strings & 15)) {
        set_error("exg_sequence_op: bad arguments (null or unaligned strings, workspace or result)");
        return EXG_E_INVALID_ARG;
    }
    if (a->op < EXG_SEQ_COMPLEMENT || a->op > EXG_SEQ_GC_CONTENT) {
        set_error("exg_sequence_op: unknown op %u", a->op);
        return EXG_E_INVALID_ARG;
    }
    if (a->n_rows >= 0xFFFFFFFFull) {
        set_error("exg_sequence_op: %llu rows (at most 2^32 - 2 a call)", (unsigned long long)a->n_rows);
        return EXG_E_INVALID_ARG;
    }
    const bool gc = a->op == EXG_SEQ_GC_CONTENT;
    if (gc ? (a->n_rows && !a->d_out_float)
           : ((a->n_rows && !a->d_out_strings) || ((uintptr_t)a->d_out_strings & 15) || (a->out_capacity && !a->d_out_payload) ||
              ((uintptr_t)a->d_out_payload & 15))) {
        set_error("exg_sequence_op: bad arguments (null or unaligned output)");
        return EXG_E_INVALID_ARG;
    }
    const Ws w = ws_layout(a->op, a->n_rows, a->d_workspace);
    if (a->workspace_bytes < w.bytes) {
        set_error("exg_sequence_op: workspace too small (%llu bytes, need %llu)", (unsigned long long)a->workspace_bytes,
                  (unsigned long long)w.bytes);
        return EXG_E_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)a->stream;
    const uint64_t n = a->n_rows;
    if (!n) {
        EXG_HIP_CHECK(hipMemsetAsync(a->d_result, 0, sizeof(exg_seq_result), s));
        return EXG_OK;
    }
    const Col c{(const uint4 *)a->d_strings, (const uint8_t *)a->d_payload, a->payload_base};
    EXG_HIP_CHECK(hipMemsetAsync(w.err, 0xFF, 8, s));
    if (gc) EXG_HIP_CHECK(hipMemsetAsync(w.count, 0, n * 4, s));
    launch_xscan(TileLenF{c, a->op}, n, w.goff, w.tmp, s);
    launch_xscan(LongF{c, a->op}, n, w.lidx, w.tmp, s);
    const uint32_t row_grid = (uint32_t)((n + 255) / 256);
    uint4 *out = (uint4 *)a->d_out_strings;
    hipLaunchKernelGGL(k_rows, dim3(row_grid), dim3(256), 0, s, c, a->op, n, w, a->out_capacity, out, a->out_base, a->d_out_float);
    if (gc) {
        hipLaunchKernelGGL(k_tiles<kGc>, dim3(kGrid), dim3(256), 0, s, c, a->op, n, w, a->out_capacity, a->d_out_payload, a->d_out_float);
        hipLaunchKernelGGL(k_gc_finish, dim3(row_grid), dim3(256), 0, s, c, n, w, a->d_out_float);
    } else if (a->op == EXG_SEQ_TRANSLATE) {
        hipLaunchKernelGGL(k_tiles<kCodons>, dim3(kGrid), dim3(256), 0, s, c, a->op, n, w, a->out_capacity, a->d_out_payload, a->d_out_float);
    } else {
        hipLaunchKernelGGL(k_tiles<kBytes>, dim3(kGrid), dim3(256), 0, s, c, a->op, n, w, a->out_capacity, a->d_out_payload, a->d_out_float);
    }
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(64), 0, s, c, a->op, n, w, a->out_capacity, a->d_result);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

extern "C" int exg_sequence_result(const exg_seq_result *d_result, void *stream, exg_seq_result *out) {
    if (const int rc = fetch_result("exg_sequence_result", d_result, stream, out)) return rc;
    if (out->error_code) {
        char text[96];
        format_error(out->error_code, out->error_bytes, out->error_length, text, sizeof text);
        set_error("%s in row %llu", text, (unsigned long long)out->error_row);
        return EXG_E_PARSE;
    }
    return EXG_OK;
}
