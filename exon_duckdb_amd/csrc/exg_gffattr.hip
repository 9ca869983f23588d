// exg_gffattr.hip — exg_gff_attributes: a column of GFF3 ninth fields -> list entries + key / value string_t, the children of
// gff_parse_attributes' MAP(VARCHAR, VARCHAR).  Count -> prefix sum -> emit, shaped like exg_gtf_attributes (exg_gtf.hip; DESIGN
// 4.18, 4.19): same arguments, same row map, same chunk-relative list offsets, same two-call capacity protocol.
//
// A wavefront takes a row, 64 bytes a step, lane = byte.  The grammar (exg_gffattr.hpp) has no quotes, so a word is three
// ballots — `;` (the field's end is a virtual one), `=`, the six blanks — and everything else is bit arithmetic on them plus the
// open segment's few scalars carried from word to word (gffattr::Segment).  A segment is judged by the lane on its `;`: its
// trailing blanks and a third piece are known only there.  That lane writes both string_t of the entry.
#include <string.h>

#include "exg_gffattr.hpp"
#include "exg_scan.hpp"
#include "exg_strcol.hpp"

namespace exg {
namespace gffattr {

static constexpr uint32_t kGrid = 4096;  // workgroups of four waves that take the rows in turn

// workspace: ent (n + 1 u64) | scan scratch | err (u64) | cnt (u32 x n)
struct Ws {
    uint64_t *ent, *tmp, *err;
    uint32_t *cnt;
    uint64_t bytes;
};
static Ws ws_layout(uint64_t n, void *base) {
    Ws w;
    uint64_t *p = (uint64_t *)base;
    w.ent = p, p += n + 1;
    w.tmp = p, p += xscan_tmp_entries(n);
    w.err = p, p += 1;
    w.cnt = (uint32_t *)p, p += (n + 1) / 2;
    w.bytes = (uint64_t)((uint8_t *)p - (uint8_t *)base) + 64;
    return w;
}
struct CntF {
    const uint32_t *cnt;
    __device__ __forceinline__ uint64_t operator()(uint64_t r) const { return cnt[r]; }
};

// a token [start, start + len), len >= 1, of the row at s as a string_t: up to 12 bytes inlined, else its prefix and the row's
// pointer + start.  All twelve byte loads are issued whatever the token's length — a position behind the bytes taken reads the
// last of them again and is masked — so that they are in flight together: a load under `if (i < take)` is a branch and a wait of
// its own, twelve round trips a token one behind the other.
__device__ __forceinline__ uint4 token_string(const uint8_t *s, uint64_t row_ptr, uint32_t start, uint32_t len) {
    uint32_t o[3] = {0, 0, 0};
    const uint32_t take = len > EXG_INLINE_LENGTH ? 4u : len;
#pragma unroll
    for (uint32_t i = 0; i < EXG_INLINE_LENGTH; i++) put_byte(o, i, s[start + min(i, take - 1u)]);
#pragma unroll
    for (uint32_t d = 0; d < 3; d++) {  // keep bytes [0, take): arithmetic, not twelve compare masks held across the loads
        const uint32_t keep = min(take - min(take, 4u * d), 4u);
        o[d] &= keep == 4u ? ~0u : (1u << (8u * keep)) - 1u;
    }
    return len > EXG_INLINE_LENGTH ? long_string(len, o[0], row_ptr + start) : inline_string(len, o);
}

// what a row came to: its entries (those in front of its error, if it has one); err_offset != kNone: R6's offset and length
struct RowOut {
    uint32_t entries, err_offset, err_length;
};

// One row, one wave: the entries of field s[0, len).  kEmit: entry k of the row goes to keys[k] / vals[k] for k < room.
template <bool kEmit>
__device__ __forceinline__ RowOut walk_row(const uint8_t *s, uint32_t len, uint64_t row_ptr, uint32_t lane, uint4 *keys, uint4 *vals, uint64_t room) {
    Segment open = fresh(0);
    bool piece_open = false;
    uint32_t entries = 0;
#pragma unroll 1
    for (uint64_t base = 0; base <= len; base += 64) {
        const uint64_t pos = base + lane;
        const bool real = pos < len;
        const uint32_t ch = real ? s[pos] : 0u;
        const Word w = make_word(__ballot(real), __ballot(ch == ';'), __ballot(ch == '='), __ballot(is_blank(ch)), __ballot(pos == len),
                                 open.first == kNone, piece_open);
        if (w.sc) {
            Verdict v{kNothing, 0, 0, 0, 0};
            if ((w.sc >> lane) & 1ull) v = judge(open, (uint32_t)base, lane, w);
            const unsigned long long en = __ballot(v.kind == kEntry);
            if (kEmit) {
                // no error is looked for here: the counting pass found them, and a failing row's entries stop at `room`, what that
                // pass saw in front of the row's error.  The row is done with its last entry
                const uint64_t k = (uint64_t)entries + bits_of(en & below(lane));
                if (v.kind == kEntry && k < room) {
                    keys[k] = token_string(s, row_ptr, v.a, v.b);
                    vals[k] = token_string(s, row_ptr, v.c, v.d);
                }
                entries += bits_of(en);
                if (entries >= room) break;
            } else {
                const unsigned long long er = __ballot(v.kind == kError);
                const unsigned long long ahead = er ? below(lo_bit(er)) : ~0ull;
                entries += bits_of(en & ahead);
                if (er) {
                    const int src = (int)lo_bit(er);
                    return RowOut{entries, (uint32_t)__shfl((int)v.a, src, 64), (uint32_t)__shfl((int)v.b, src, 64)};
                }
            }
        }
        if (len - base < 64) break;
        advance(open, (uint32_t)base, w);
        piece_open = w.tail;
    }
    if (!entries) return RowOut{0, 0, len};  // no segment at all: the field is the segment (R1), and it holds no `=`
    return RowOut{entries, kNone, 0};
}

// row j of the call: its field's bytes, length and pointer
struct RowRef {
    const uint8_t *s;
    uint32_t len;
    uint64_t ptr;
};
__device__ __forceinline__ RowRef row_of(const Col &c, const uint32_t *row_map, uint64_t j) {
    const uint64_t r = row_map ? (uint64_t)row_map[j] : j;
    const uint4 v = c.rows[r];
    return {src_of(c, r, v), v.x, (uint64_t)v.z | ((uint64_t)v.w << 32)};
}

// a wave per row: counting pass (every row validated, cnt[j] = its entries, err = the lowest failing row) and emit pass (the
// children and the list entries)
template <bool kEmit>
__global__ __launch_bounds__(256) void k_rows(Col c, const uint32_t *row_map, uint64_t n, Ws w, uint64_t cap, uint64_t chunk_rows, uint64_t *entries,
                                              uint64_t *chunk_base, uint4 *keys, uint4 *vals) {
    const uint32_t lane = lane_id();
    // (the wave's number through readfirstlane: the row, its length and the carried scalars are then the scalar unit's)
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const bool fits = kEmit && w.ent[n] <= cap;
    uint64_t bad = kNoError;
    for (uint64_t j = wave; j < n; j += n_waves) {
        const RowRef row = row_of(c, row_map, j);
        if (!kEmit) {
            const RowOut o = walk_row<false>(row.s, row.len, row.ptr, lane, nullptr, nullptr, 0);
            if (lane == 0) w.cnt[j] = o.entries;
            if (o.err_offset != kNone && bad == kNoError) bad = j;  // (a wave's rows come in rising order)
        } else {
            const uint64_t e0 = w.ent[j], cnt = w.cnt[j];
            if (lane == 0 && entries) {
                const uint64_t first = chunk_rows ? j / chunk_rows * chunk_rows : 0;
                entries[2 * j] = chunk_rows ? e0 - w.ent[first] : e0;
                entries[2 * j + 1] = cnt;
                if (chunk_rows && j == first) chunk_base[j / chunk_rows] = e0;
            }
            if (fits && cnt) walk_row<true>(row.s, row.len, row.ptr, lane, keys + e0, vals + e0, cnt);
        }
    }
    if (!kEmit && lane == 0 && bad != kNoError) atomicMin((unsigned long long *)w.err, (unsigned long long)bad);
}

// one wave: the result block; the failing row is walked once more for its offset and length
__global__ __launch_bounds__(64) void k_finish(Col c, const uint32_t *row_map, uint64_t n, Ws w, uint64_t cap, uint64_t chunk_rows, uint64_t *chunk_base,
                                               struct exg_gff_attributes_result *res) {
    if (blockIdx.x) return;
    struct exg_gff_attributes_result r;
    memset(&r, 0, sizeof r);
    r.n_rows = n;
    r.total_entries = w.ent[n];
    if (r.total_entries > cap) r.flags = EXG_RF_CAPACITY;
    const uint64_t bad = *w.err;
    if (bad < n) {
        const RowRef row = row_of(c, row_map, bad);
        const RowOut o = walk_row<false>(row.s, row.len, row.ptr, lane_id(), nullptr, nullptr, 0);
        r.error_code = EXG_PE_GFF_ATTRIBUTES;
        r.error_row = bad;
        r.error_offset = o.err_offset;
        r.error_length = o.err_length;
    }
    if (threadIdx.x) return;
    if (chunk_rows && chunk_base) chunk_base[(n + chunk_rows - 1) / chunk_rows] = w.ent[n];
    *res = r;
}

}  // namespace gffattr
}  // namespace exg

using namespace exg;

static_assert(sizeof(struct exg_gff_attributes_result) == 64, "exg_gff_attributes_result is 64 bytes");

extern "C" uint64_t exg_gff_attributes_workspace_bytes(uint64_t n_rows) { return gffattr::ws_layout(n_rows, nullptr).bytes; }

extern "C" int exg_gff_attributes(const exg_gff_attributes_args *a) {
    using namespace exg::gffattr;
    if (!a || !a->d_result || ((uintptr_t)a->d_result & 7) || !a->d_workspace || ((uintptr_t)a->d_workspace & 7) || (a->n_rows && !a->d_strings) ||
        ((uintptr_t)a->d_strings & 15)) {
        set_error("exg_gff_attributes: bad arguments (null or unaligned column, workspace or result)");
        return EXG_E_INVALID_ARG;
    }
    if (a->n_rows >= 0xFFFFFFFFull) {
        set_error("exg_gff_attributes: %llu rows (at most 2^32 - 2 a call)", (unsigned long long)a->n_rows);
        return EXG_E_INVALID_ARG;
    }
    if ((a->entries_capacity && (!a->d_out_keys || !a->d_out_values || (a->n_rows && !a->d_out_entries))) || ((uintptr_t)a->d_out_keys & 15) ||
        ((uintptr_t)a->d_out_values & 15) || ((uintptr_t)a->d_out_entries & 7) || (a->chunk_rows && !a->d_out_chunk_base)) {
        set_error("exg_gff_attributes: bad arguments (null or unaligned output)");
        return EXG_E_INVALID_ARG;
    }
    const uint64_t n = a->n_rows;
    if (a->workspace_bytes < ws_layout(n, nullptr).bytes) {
        set_error("exg_gff_attributes: workspace too small (%llu bytes, need %llu)", (unsigned long long)a->workspace_bytes,
                  (unsigned long long)ws_layout(n, nullptr).bytes);
        return EXG_E_INVALID_ARG;
    }
    const Ws w = ws_layout(n, a->d_workspace);
    hipStream_t s = (hipStream_t)a->stream;
    if (!n) {
        EXG_HIP_CHECK(hipMemsetAsync(a->d_result, 0, sizeof(struct exg_gff_attributes_result), s));
        if (a->chunk_rows) EXG_HIP_CHECK(hipMemsetAsync(a->d_out_chunk_base, 0, 8, s));
        return EXG_OK;
    }
    const Col c{(const uint4 *)a->d_strings, (const uint8_t *)a->d_payload, a->payload_base};
    const uint32_t grid = (uint32_t)((n + 3) / 4 < kGrid ? (n + 3) / 4 : kGrid);
    EXG_HIP_CHECK(hipMemsetAsync(w.err, 0xFF, 8, s));
    hipLaunchKernelGGL(k_rows<false>, dim3(grid), dim3(256), 0, s, c, a->d_row_map, n, w, 0ull, 0ull, (uint64_t *)nullptr, (uint64_t *)nullptr,
                       (uint4 *)nullptr, (uint4 *)nullptr);
    launch_xscan(CntF{w.cnt}, n, w.ent, w.tmp, s);
    hipLaunchKernelGGL(k_rows<true>, dim3(grid), dim3(256), 0, s, c, a->d_row_map, n, w, a->entries_capacity, a->chunk_rows,
                       (uint64_t *)a->d_out_entries, a->d_out_chunk_base, (uint4 *)a->d_out_keys, (uint4 *)a->d_out_values);
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(64), 0, s, c, a->d_row_map, n, w, a->entries_capacity, a->chunk_rows, a->d_out_chunk_base, a->d_result);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

extern "C" int exg_gff_attributes_result(const struct exg_gff_attributes_result *d_result, void *stream, struct exg_gff_attributes_result *out) {
    if (const int rc = fetch_result("exg_gff_attributes_result", d_result, stream, out)) return rc;
    if (out->error_code) {
        set_error("Invalid GFF attribute in row %llu at byte %llu", (unsigned long long)out->error_row, (unsigned long long)out->error_offset);
        return EXG_E_PARSE;
    }
    return EXG_OK;
}
