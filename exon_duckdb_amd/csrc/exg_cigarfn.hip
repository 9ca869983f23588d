// exg_cigarfn.hip — parse_cigar / extract_from_cigar (exon/src/exon/sam_functions/module.cpp:32-131) on the cigar column a BAM
// or SAM scan left in HBM (include/exon_gpu.h: exg_cigar_op).  The rules are exg_cigarfn.hpp's; here is the work distribution.
//
// A cigar column holds short-read rows (`150M`, `75M2I73M`: inlined in their string_t) next to long-read rows of tens of
// thousands of operations, so — as exg_seqfn.hip does — the rows of up to 12 bytes get a thread each, straight out of the
// string_t, and the longer ("long") rows are cut by BYTES: "tile space" is the concatenation of their bytes in row order, cut
// into tiles of 4 KiB.  A tile is one wave's (a workgroup is one wave: nothing but the error word is shared between tiles): it
// finds its rows by a 64-ary search of loff, stages their offsets and sources in LDS (a tile touches at most 318 rows of 13
// bytes and more) and takes 64 rounds of one byte a lane.  A lane judges its byte by the byte in front of it (the lane below's,
// handed up): a byte that is neither digit nor letter, a letter behind a non-digit, a digit that ends the row are the row's
// errors where they stand.  The lane that TERMINATES a digit run — the letter, the bad byte, the row's last digit — reads the
// run's length with run_before(): one walker a run, back into the tile in front if the run began there, never in front of the
// row; a row of a million zeros is one lane's linear walk, and every other digit lane does nothing.
// parse_cigar:
//   1. prefix sums over the rows (exg_scan.hpp): goff / lidx place the long rows in tile space (k_rows lists them: lrow, loff);
//   2. counting: k_rows counts the letters of the short rows, k_tiles<true> those of a tile (tcnt) and of each long row (one
//      atomicAdd a row and tile into rowops);
//   3. prefix sums of the counts: ent over all rows (the list entries), lpre over the long rows, tpre over the tiles: the letter
//      at a byte of tile space is operation ent[row] - lpre[row] + tpre[tile] + (letters of the tile in front of it);
//   4. k_tiles<false>: the lane that holds a letter validates its run and writes its operation: one 16-byte store and one
//      4-byte store, neighbouring letters of a round to neighbouring entries; k_emit_rows writes the entries and the short rows;
// extract_from_cigar: k_tiles<false> validates the long rows (no counts, no stores), k_extract — a thread per row — validates
// the short ones and reads the first operation behind the first run and the last one from the row's end.
// Errors: atomicMin on (row << 32 | offset + 1), 0xFFFFFFFF in the low word for the range error: the lowest row wins, in it the
// leftmost offset, the range error last.  Integer arithmetic and fixed offsets only: two runs are byte-identical.
#include "exg_common.hpp"
#include "exg_scan.hpp"
#include "exg_cigarfn.hpp"
#include "exg_strcol.hpp"

namespace exg {
namespace cigarfn {

static constexpr uint32_t kTile = 4096;
static constexpr uint32_t kTileRows = tile_rows(kTile);  // <= 318
static constexpr uint32_t kGrid = 8192;  // waves that take the tiles in turn: 32 a CU
static constexpr uint32_t kRangeKey = 0xFFFFFFFFu;

// workspace: goff | lidx | loff | ent | lpre (n + 1 u64 each) | tpre (tiles + 1) | scan scratch | err (u64) | lrow | rowops
// (u32 x n) | tcnt (u32 x tiles); ent, lpre, tpre, rowops and tcnt for parse_cigar only
struct Ws {
    uint64_t *goff, *lidx, *loff, *ent, *lpre, *tpre, *tmp, *err;
    uint32_t *lrow, *rowops, *tcnt;
    uint64_t tiles_cap, bytes;
};
static Ws ws_layout(uint32_t op, uint64_t n, uint64_t tiles, void *base) {
    const bool parse = op == EXG_CIGAR_PARSE;
    Ws w;
    uint64_t *p = (uint64_t *)base;
    w.goff = p, p += n + 1;
    w.lidx = p, p += n + 1;
    w.loff = p, p += n + 1;
    w.ent = p, p += parse ? n + 1 : 0;
    w.lpre = p, p += parse ? n + 1 : 0;
    w.tpre = p, p += parse ? tiles + 1 : 0;
    w.tmp = p, p += xscan_tmp_entries(parse && tiles > n ? tiles : n);
    w.err = p, p += 1;
    w.lrow = (uint32_t *)p, p += (n + 1) / 2;
    w.rowops = (uint32_t *)p, p += parse ? (n + 1) / 2 : 0;
    w.tcnt = (uint32_t *)p, p += parse ? (tiles + 1) / 2 : 0;
    w.tiles_cap = tiles;
    w.bytes = (uint64_t)((uint8_t *)p - (uint8_t *)base) + 64;
    return w;
}

struct LongLenF {
    Col c;
    __device__ __forceinline__ uint64_t operator()(uint64_t r) const {
        const uint32_t len = c.rows[r].x;
        return len > EXG_INLINE_LENGTH ? len : 0;
    }
};
struct LongF {
    Col c;
    __device__ __forceinline__ uint64_t operator()(uint64_t r) const { return c.rows[r].x > EXG_INLINE_LENGTH ? 1 : 0; }
};
struct RowOpsF {
    const uint32_t *rowops;
    __device__ __forceinline__ uint64_t operator()(uint64_t r) const { return rowops[r]; }
};
struct LongOpsF {
    Col c;
    const uint32_t *rowops;
    __device__ __forceinline__ uint64_t operator()(uint64_t r) const { return c.rows[r].x > EXG_INLINE_LENGTH ? rowops[r] : 0; }
};
__device__ __forceinline__ uint4 op_string(uint32_t letter) { return make_uint4(1u, letter, 0u, 0u); }
__device__ __forceinline__ uint64_t syntax_key(uint64_t row, uint64_t offset) { return (row << 32) | (offset + 1); }

// ---- a thread per row: the list of the long rows; parse_cigar: the short rows validated and counted -----------
__global__ __launch_bounds__(256) void k_rows(Col c, uint64_t n, Ws w, bool parse) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r == 0) w.loff[w.lidx[n]] = w.goff[n];
    if (r >= n) return;
    const uint4 v = c.rows[r];
    const uint32_t len = v.x;
    if (len > EXG_INLINE_LENGTH) {
        const uint64_t k = w.lidx[r];
        w.lrow[k] = (uint32_t)r;
        w.loff[k] = w.goff[r];
        return;
    }
    if (!parse) return;  // (extract_from_cigar: k_extract reads the short rows)
    const uint8_t *s = src_of(c, r, v);
    uint32_t letters = 0;
    for (uint32_t i = 0; i < len; i++) letters += is_op(s[i]) ? 1u : 0u;
    w.rowops[r] = letters;
    const Check ck = check(s, len);
    if (!ck.ok) atomicMin((unsigned long long *)w.err, (unsigned long long)syntax_key(r, ck.offset));
}

// ---- tiles: a wave each ---------------------------------------------------------------------------------------
// kCount: the letters of the tile and of its rows, nothing else.  Otherwise: every row error of the tile's bytes, and — parse,
// when the children hold all operations — the operations of its letters.
template <bool kCount>
__global__ __launch_bounds__(64) void k_tiles(Col c, uint64_t n, Ws w, bool parse, uint64_t cap, uint4 *out_op, int32_t *out_len) {
    __shared__ uint64_t s_off[kTileRows + 1];
    __shared__ const uint8_t *s_src[kTileRows];
    __shared__ uint32_t s_row[kTileRows];
    __shared__ uint64_t s_aux[kTileRows];  // kCount: the row's letters in this tile; else: ent - lpre + tpre, what a letter's rank starts from
    const uint64_t total = w.goff[n], L = w.lidx[n];
    const uint64_t n_tiles = (total + kTile - 1) / kTile;
    if (parse && n_tiles > w.tiles_cap) return;
    const bool store = !kCount && parse && w.ent[n] <= cap;
    const uint32_t lane = lane_id();
    uint64_t key = kNoError;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t T0 = tile * kTile, T1 = T0 + kTile < total ? T0 + kTile : total;
        __syncthreads();  // the tile before is done with the staged rows
        const uint64_t k0 = wave_search(w.loff, 0, L, T0);
        const uint64_t k_hi = k0 + kTileRows + 1 < L ? k0 + kTileRows + 1 : L;  // the last row is at most kTileRows behind the first
        const uint64_t k1 = wave_search(w.loff, k0, k_hi, T1 - 1);
        uint32_t cnt = (uint32_t)(k1 - k0 + 1);
        if (cnt > kTileRows) cnt = kTileRows;  // (cannot happen: long rows have 13 bytes and more)
        const uint64_t tile_rank = !kCount && parse ? w.tpre[tile] : 0;
        for (uint32_t i = lane; i <= cnt; i += 64) s_off[i] = w.loff[k0 + i];
        for (uint32_t i = lane; i < cnt; i += 64) {
            const uint32_t r = w.lrow[k0 + i];
            s_row[i] = r;
            s_src[i] = src_of(c, r, c.rows[r]);
            s_aux[i] = !kCount && parse ? w.ent[r] - w.lpre[r] + tile_rank : 0;
        }
        __syncthreads();
        uint32_t i0 = 0;       // the row of the round's first byte
        uint32_t letters = 0;  // of the tile's rounds so far
#pragma unroll 1
        for (uint64_t q0 = T0; q0 < T1; q0 += 64) {
            const uint64_t q = q0 + lane;
            const bool active = q < T1;
            uint32_t li = i0;
            while (li + 1 < cnt && s_off[li + 1] <= q) li++;
            const uint32_t i_last = (uint32_t)__shfl((int)li, 63, 64);
            const uint64_t off = s_off[li];
            const uint32_t j = (uint32_t)(q - off), len = (uint32_t)(s_off[li + 1] - off);
            const uint8_t *s = s_src[li];
            const uint32_t ch = active ? s[j] : 0u;
            const bool op = active && is_op(ch);
            const uint64_t op_mask = __ballot(op);
            if (kCount) {
                for (uint32_t rr = i0; rr <= i_last; rr++) {  // (a round of 64 bytes touches six rows at the most)
                    const uint32_t k = (uint32_t)__popcll(__ballot(op && li == rr));
                    if (lane == 0) s_aux[rr] += k;
                }
            } else {
                const uint32_t up = (uint32_t)__shfl_up((int)ch, 1, 64);
                const uint32_t prev = !active || j == 0 ? 0u : (lane ? up : (uint32_t)s[j - 1]);
                const bool dg = active && is_digit(ch), pd = is_digit(prev);
                uint64_t bad = kNoError, e = 0;
                bool term = false;
                if (active) {
                    if ((!op && !dg) || (op && !pd)) bad = j;
                    if (!dg && pd) {
                        term = true, e = j;
                    } else if (dg && j + 1 == len) {
                        term = true, e = len, bad = len;
                    }
                }
                uint32_t val = 0;
                if (term) {
                    const Run rn = run_before(s, e);
                    if (!rn.ok) bad = rn.bad;  // (in front of e: the leftmost of the two)
                    val = rn.len;
                }
                if (bad != kNoError) {
                    const uint64_t k = syntax_key(s_row[li], bad);
                    key = k < key ? k : key;
                }
                if (store && op) {
                    const uint64_t rank = s_aux[li] + letters + (uint32_t)__popcll(op_mask & ((1ull << lane) - 1ull));
                    if (rank < cap) {
                        out_op[rank] = op_string(ch);
                        out_len[rank] = (int32_t)val;
                    }
                }
            }
            letters += (uint32_t)__popcll(op_mask);
            i0 = i_last;
        }
        if (kCount) {
            __syncthreads();
            for (uint32_t i = lane; i < cnt; i += 64)
                if (s_aux[i]) atomicAdd(&w.rowops[s_row[i]], (uint32_t)s_aux[i]);
            if (lane == 0) w.tcnt[tile] = letters;
        }
    }
    if (!kCount) wave_min_error(key, w.err, lane);
}

// ---- parse_cigar, a thread per row: the list entries, and the operations of the short rows ----------------------
__global__ __launch_bounds__(256) void k_emit_rows(Col c, uint64_t n, Ws w, uint64_t cap, uint64_t *entries, uint4 *out_op,
                                                   int32_t *out_len) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n || (w.goff[n] + kTile - 1) / kTile > w.tiles_cap) return;
    uint64_t k = w.ent[r];
    if (entries) entries[2 * r] = k, entries[2 * r + 1] = w.rowops[r];
    const uint4 v = c.rows[r];
    const uint32_t len = v.x;
    if (w.ent[n] > cap || len > EXG_INLINE_LENGTH) return;
    const uint8_t *s = src_of(c, r, v);
    if (is_absent(s, len)) return;
    for (uint64_t i = 0; i < len;) {
        const Step st = next_op(s, len, i);
        if (!st.ok) break;  // (a failing row: reported by k_rows)
        out_op[k] = op_string(st.op);
        out_len[k] = (int32_t)st.len;
        i = st.next, k++;
    }
}

// ---- extract_from_cigar, a thread per row -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_extract(Col c, Col q, uint64_t n, Ws w, int32_t *out_start, int32_t *out_end, uint4 *out_seq) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const uint4 cv = c.rows[r], sv = q.rows[r];
    const uint32_t clen = cv.x, slen = sv.x;
    const uint8_t *cs = src_of(c, r, cv);
    const bool absent = is_absent(cs, clen);
    uint32_t first_op = 0, first_len = 0, last_op = 0, last_len = 0;
    uint64_t key = kNoError;
    bool ok = true;
    if (!absent) {
        if (clen <= EXG_INLINE_LENGTH) {  // (a long row: the tiles validate it)
            const Check ck = check(cs, clen);
            if (!ck.ok) key = syntax_key(r, ck.offset), ok = false;
        }
        if (ok) {  // the first operation behind the first run, the last one from the row's end: the row is not walked
            const Step f = next_op(cs, clen, 0);
            const uint32_t last = cs[clen - 1];
            ok = f.ok && is_op(last) && clen >= 2 && is_digit(cs[clen - 2]);
            if (ok) {
                const Run rn = run_before(cs, clen - 1);
                ok = rn.ok;
                first_op = f.op, first_len = f.len, last_op = last, last_len = rn.len;
            }
        }
    }
    if (ok) {
        int32_t start = 0, end = 0;
        if (!extract_range(absent, first_op, first_len, last_op, last_len, slen, &start, &end)) {
            key = (r << 32) | kRangeKey;
        } else {
            const uint32_t m = (uint32_t)(end - start);
            const uint8_t *p = src_of(q, r, sv) + start;
            uint32_t o[3] = {0, 0, 0};
#pragma unroll
            for (int i = 0; i < EXG_INLINE_LENGTH; i++)
                if ((uint32_t)i < (m > EXG_INLINE_LENGTH ? 4u : m)) put_byte(o, i, p[i]);
            out_start[r] = start, out_end[r] = end;
            if (m > EXG_INLINE_LENGTH)  // a slice of the caller's payload: the input's pointer + start
                out_seq[r] = long_string(m, o[0], ((uint64_t)sv.z | ((uint64_t)sv.w << 32)) + (uint32_t)start);
            else
                out_seq[r] = inline_string(m, o);
        }
    }
    if (key != kNoError) atomicMin((unsigned long long *)w.err, (unsigned long long)key);
}

__global__ void k_finish(Col c, uint64_t n, Ws w, bool parse, uint64_t cap, struct exg_cigar_result *res) {
    if (threadIdx.x || blockIdx.x) return;
    struct exg_cigar_result r;
    memset(&r, 0, sizeof r);
    r.n_rows = n;
    if (parse && (w.goff[n] + kTile - 1) / kTile > w.tiles_cap) {
        r.flags = EXG_RF_INDEX_OVERFLOW;
        *res = r;
        return;
    }
    if (parse) {
        r.total_ops = w.ent[n];
        if (r.total_ops > cap) r.flags = EXG_RF_CAPACITY;
    }
    const uint64_t key = *w.err;
    if (key != kNoError) {
        const uint64_t row = key >> 32;
        const uint32_t low = (uint32_t)key;
        r.error_row = row;
        if (low == kRangeKey) {
            r.error_code = EXG_PE_CIGAR_RANGE;
        } else {
            const uint4 v = c.rows[row];
            r.error_code = EXG_PE_CIGAR_INVALID;
            r.error_offset = low - 1;
            if (r.error_offset < v.x) r.error_byte = src_of(c, row, v)[r.error_offset];
        }
    }
    *res = r;
}

}  // namespace cigarfn
}  // namespace exg

using namespace exg;
using namespace exg::cigarfn;

static_assert(sizeof(struct exg_cigar_result) == 64, "exg_cigar_result is 64 bytes");

extern "C" uint64_t exg_cigar_workspace_bytes(uint32_t op, uint64_t n_rows, uint64_t cigar_payload_bytes) {
    return ws_layout(op, n_rows, (cigar_payload_bytes + kTile - 1) / kTile, nullptr).bytes;
}

extern "C" int exg_cigar_op(const exg_cigar_op_args *a) {
    if (!a || !a->d_result || ((uintptr_t)a->d_result & 7) || !a->d_workspace || ((uintptr_t)a->d_workspace & 7) ||
        (a->n_rows && !a->d_cigar) || ((uintptr_t)a->d_cigar & 15)) {
        set_error("exg_cigar_op: bad arguments (null or unaligned cigar column, workspace or result)");
        return EXG_E_INVALID_ARG;
    }
    if (a->op != EXG_CIGAR_PARSE && a->op != EXG_CIGAR_EXTRACT) {
        set_error("exg_cigar_op: unknown op %u", a->op);
        return EXG_E_INVALID_ARG;
    }
    if (a->n_rows >= 0xFFFFFFFFull) {
        set_error("exg_cigar_op: %llu rows (at most 2^32 - 2 a call)", (unsigned long long)a->n_rows);
        return EXG_E_INVALID_ARG;
    }
    const bool parse = a->op == EXG_CIGAR_PARSE;
    if (parse ? ((a->ops_capacity && (!a->d_out_op || !a->d_out_len || (a->n_rows && !a->d_out_entries))) || ((uintptr_t)a->d_out_op & 15) ||
                 ((uintptr_t)a->d_out_len & 3) || ((uintptr_t)a->d_out_entries & 7))
              : ((a->n_rows && (!a->d_sequence || !a->d_out_start || !a->d_out_end || !a->d_out_sequence)) || ((uintptr_t)a->d_sequence & 15) ||
                 ((uintptr_t)a->d_out_sequence & 15) || ((uintptr_t)a->d_out_start & 3) || ((uintptr_t)a->d_out_end & 3))) {
        set_error("exg_cigar_op: bad arguments (null or unaligned sequence column or output)");
        return EXG_E_INVALID_ARG;
    }
    const uint64_t n = a->n_rows;
    // the tiles the workspace has counters for: the largest count whose layout fits
    uint64_t tiles = 0;
    if (a->workspace_bytes < ws_layout(a->op, n, 0, nullptr).bytes) {
        set_error("exg_cigar_op: workspace too small (%llu bytes, need %llu)", (unsigned long long)a->workspace_bytes,
                  (unsigned long long)ws_layout(a->op, n, 0, nullptr).bytes);
        return EXG_E_INVALID_ARG;
    }
    if (parse) {
        uint64_t hi = a->workspace_bytes / 8;
        while (tiles < hi) {
            const uint64_t mid = tiles + (hi - tiles + 1) / 2;
            if (ws_layout(a->op, n, mid, nullptr).bytes <= a->workspace_bytes)
                tiles = mid;
            else
                hi = mid - 1;
        }
    }
    const Ws w = ws_layout(a->op, n, tiles, a->d_workspace);
    hipStream_t s = (hipStream_t)a->stream;
    if (!n) {
        EXG_HIP_CHECK(hipMemsetAsync(a->d_result, 0, sizeof(struct exg_cigar_result), s));
        return EXG_OK;
    }
    const Col c{(const uint4 *)a->d_cigar, (const uint8_t *)a->d_cigar_payload, a->cigar_payload_base};
    const uint32_t row_grid = (uint32_t)((n + 255) / 256);
    const uint32_t tile_grid = parse && tiles < kGrid ? (uint32_t)(tiles ? tiles : 1) : kGrid;
    uint4 *out_op = (uint4 *)a->d_out_op;
    EXG_HIP_CHECK(hipMemsetAsync(w.err, 0xFF, 8, s));
    launch_xscan(LongLenF{c}, n, w.goff, w.tmp, s);
    launch_xscan(LongF{c}, n, w.lidx, w.tmp, s);
    if (parse) {
        EXG_HIP_CHECK(hipMemsetAsync(w.rowops, 0, n * 4, s));
        if (tiles) EXG_HIP_CHECK(hipMemsetAsync(w.tcnt, 0, tiles * 4, s));
        hipLaunchKernelGGL(k_rows, dim3(row_grid), dim3(256), 0, s, c, n, w, true);
        hipLaunchKernelGGL(k_tiles<true>, dim3(tile_grid), dim3(64), 0, s, c, n, w, true, a->ops_capacity, out_op, a->d_out_len);
        launch_xscan(RowOpsF{w.rowops}, n, w.ent, w.tmp, s);
        launch_xscan(LongOpsF{c, w.rowops}, n, w.lpre, w.tmp, s);
        launch_xscan(RowOpsF{w.tcnt}, tiles, w.tpre, w.tmp, s);
        hipLaunchKernelGGL(k_tiles<false>, dim3(tile_grid), dim3(64), 0, s, c, n, w, true, a->ops_capacity, out_op, a->d_out_len);
        hipLaunchKernelGGL(k_emit_rows, dim3(row_grid), dim3(256), 0, s, c, n, w, a->ops_capacity, (uint64_t *)a->d_out_entries, out_op,
                           a->d_out_len);
    } else {
        const Col q{(const uint4 *)a->d_sequence, (const uint8_t *)a->d_sequence_payload, a->sequence_payload_base};
        hipLaunchKernelGGL(k_rows, dim3(row_grid), dim3(256), 0, s, c, n, w, false);
        hipLaunchKernelGGL(k_tiles<false>, dim3(tile_grid), dim3(64), 0, s, c, n, w, false, 0ull, (uint4 *)nullptr, (int32_t *)nullptr);
        hipLaunchKernelGGL(k_extract, dim3(row_grid), dim3(256), 0, s, c, q, n, w, a->d_out_start, a->d_out_end, (uint4 *)a->d_out_sequence);
    }
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(64), 0, s, c, n, w, parse, a->ops_capacity, a->d_result);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

extern "C" int exg_cigar_result(const struct exg_cigar_result *d_result, void *stream, struct exg_cigar_result *out) {
    if (const int rc = fetch_result("exg_cigar_result", d_result, stream, out)) return rc;
    if (out->error_code) {
        char text[96];
        format_error(out->error_code, out->error_row, out->error_offset, text, sizeof text);
        set_error("%s", text);
        return EXG_E_PARSE;
    }
    return EXG_OK;
}
