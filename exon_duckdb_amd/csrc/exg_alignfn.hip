// exg_alignfn.hip — alignment_score / alignment_score_wfa_gap_affine (exon/src/exon/alignment_functions/module.cpp:264-329)
// on two duckdb::string_t columns that are still in HBM (include/exon_gpu.h: exg_align_score).  The rules and the recurrences
// are exg_alignfn.hpp's, the string readers and ring policies exg_align_core.hpp's; here is the work distribution.
//
// The exact wavefront algorithm, score only.  A pair keeps, per diagonal k = h - v (index d = k + m, 0 .. n + m), the offsets
// of M for the last max(x, o + e) + 1 scores and of I and D for the last e + 1: a ring, indexed by s mod depth.  The lanes of
// a pair lie on neighbouring diagonals; one score step is one pass over the diagonals any wavefront has reached, widened by
// one on either side.  The columns of the ring a step may read are kept initialised: when the reached range
// comes within a diagonal of the initialised one, seven more diagonals are set to kNone in every wavefront of the ring.
//
// One body (k_align) serves two storage policies, the way LdsSrc / GlobalSrc serve the line scans:
//   LdsPolicy     strings staged in LDS, 16-bit offsets in LDS: a row takes it when the worst case, n + m + 1 diagonals times
//                 the ring depth, fits the LDS share of a pair.  A wave holds 64 / lanes pairs, each on its own rows: the
//                 pairs of a wave step in lockstep (one barrier a step), a pair that is done claims the next row.
//   GlobalPolicy  the rows that do not fit (k_align<LdsPolicy> lists them): strings read in place, 32-bit offsets in a slot of
//                 the workspace that the workgroup owns, sized by max_pair_bytes; one pair a wave.
// Rows are claimed from an atomic counter by persistent workgroups (eight at a time while they fit LDS, one at a time in the
// global pass): an expensive pair holds up at most the seven LDS-sized rows claimed with it, never the column.  The score
// loop ends at the hard bound 2o + e(n + m) whatever happens.  Every result depends on its row alone: two launches are
// byte-identical.  Too-long rows: atomicMin on the row number.
#include "exg_align_core.hpp"

namespace exg {
namespace alignfn {

static constexpr uint32_t kDefaultLanes = 64;    // DESIGN 4.13 has the measurement

struct Counters {  // 64 bytes at the front of the workspace
    unsigned long long next_row, n_list, next_list, err_row, n_capped, flags, pad[2];
};
struct Params {
    uint32_t x, o, e, rm, rg, max_penalty;
    uint64_t max_pair_bytes;
};
// workspace: counters | list (u32 x n_rows) | kSlots slots of (rm + 2 rg) x (max_pair_bytes + 1) int32
struct Ws {
    Counters *c;
    uint32_t *list;
    int32_t *slots;
    uint64_t slot_entries, bytes;
};
static Ws ws_layout(uint64_t n, uint64_t max_pair_bytes, uint32_t x, uint32_t o, uint32_t e, void *base) {
    Ws w;
    uint8_t *p = (uint8_t *)base;
    w.c = (Counters *)p, p += sizeof(Counters);
    w.list = (uint32_t *)p, p += ((n * 4 + 15) & ~15ull);
    w.slots = (int32_t *)p;
    // no slots when every admissible row fits LDS with the whole workgroup's share to itself
    const bool all_lds = lds_need(depth_of(x, o, e), max_pair_bytes) <= kLdsPerWorkgroup / 4;
    w.slot_entries = all_lds ? 0 : (((uint64_t)depth_of(x, o, e) * (max_pair_bytes + 1) + 3) & ~3ull);
    p += w.slot_entries * 4 * kSlots;
    w.bytes = (uint64_t)(p - (uint8_t *)base);
    return w;
}

template <class P, int kLanes>
__global__ __launch_bounds__(64) void k_align(Col tc, Col pc, uint64_t n_rows, Params prm, Ws w, uint32_t lds_share, float *out,
                                              unsigned long long *valid) {
    typedef typename P::off_t off_t;
    typedef typename P::idx_t idx_t;
    extern __shared__ uint32_t s_mem[];
    const uint32_t j = threadIdx.x & (kLanes - 1), g = threadIdx.x / kLanes;
    const int32_t x = (int32_t)prm.x, oe = (int32_t)(prm.o + prm.e), e = (int32_t)prm.e, rm = (int32_t)prm.rm, rg = (int32_t)prm.rg;
    const uint32_t depth = prm.rm + 2 * prm.rg;
    const uint64_t limit = P::kLds ? n_rows : w.c->n_list;
    unsigned long long *counter = P::kLds ? &w.c->next_row : &w.c->next_list;

    // the state of this group's pair (uniform over the group's lanes)
    bool have = false, exhausted = false;
    uint64_t row = 0;
    unsigned long long next = 0, last = 0;  // the rows this group has claimed and not begun
    int32_t n = 0, m = 0, nd = 1, s = 0, s_max = 0;
    int32_t lo = 0, hi = 0, wlo = 0, whi = 0;  // diagonals reached; diagonals initialised
    int32_t ms = 0, gs = 0;                    // s mod rm, s mod rg
    typename P::Str t{}, p{};
    off_t *M = nullptr, *I = nullptr, *D = nullptr;

    // every wavefront of the ring := kNone on the diagonals [a, b) (M, I and D lie behind one another: depth rows of nd)
    auto clear = [&](int32_t a, int32_t b) {
        for (uint32_t slot = 0; slot < depth; slot++) {
            off_t *ring = M + (idx_t)slot * nd;
            for (int32_t d = a + (int32_t)j; d < b; d += kLanes) ring[d] = (off_t)kNone;
        }
    };

    for (;;) {
        if (!have && !exhausted) {
            // rows that fit LDS are claimed eight at a time: one counter takes ~10^8 atomics a second, which is what 3 M
            // near-identical read pairs ran at when every pair paid one.  A pair of the global pass is claimed alone.
            if (next == last) {
                constexpr unsigned long long kClaim = P::kLds ? 8 : 1;
                if (j == 0) next = atomicAdd(counter, kClaim);
                next = __shfl(next, 0, kLanes);
                last = next + kClaim < limit ? next + kClaim : limit;
                if (next >= limit) exhausted = true, last = next;
            }
            if (!exhausted) {
                const unsigned long long idx = next++;
                row = P::kLds ? idx : w.list[idx];
                const uint4 tv = tc.rows[row], pv = pc.rows[row];
                const uint64_t nm = (uint64_t)tv.x + pv.x;
                if (P::kLds && nm > prm.max_pair_bytes) {
                    if (j == 0) atomicMin(&w.c->err_row, (unsigned long long)row);
                } else if (P::kLds && lds_need(depth, nm) > lds_share) {
                    if (j == 0) w.list[atomicAdd(&w.c->n_list, 1ull)] = (uint32_t)row;
                } else {
                    have = true;
                    n = (int32_t)tv.x, m = (int32_t)pv.x, nd = n + m + 1;
                    const GlobalStr gt{src_of(tc, row, tv), tv.x}, gp{src_of(pc, row, pv), pv.x};
                    if constexpr (P::kLds) {
                        uint32_t *base = s_mem + g * (lds_share / 4);
                        const uint32_t tw = str_words(tv.x), pw = str_words(pv.x);
                        for (uint32_t i = j; 4 * i < tv.x; i += kLanes) base[i] = gt.get4(4 * i);
                        for (uint32_t i = j; 4 * i < pv.x; i += kLanes) base[tw + i] = gp.get4(4 * i);
                        t = LdsStr{base, tv.x}, p = LdsStr{base + tw, pv.x};
                        M = reinterpret_cast<off_t *>(base + tw + pw);
                    } else {
                        t = gt, p = gp;
                        M = w.slots + (uint64_t)blockIdx.x * w.slot_entries;
                    }
                    I = M + (idx_t)rm * nd, D = I + (idx_t)rg * nd;
                    s = 0, ms = 0, gs = 0, lo = hi = m;
                    const uint32_t bound = penalty_bound(prm.o, prm.e, (uint64_t)n, (uint64_t)m);
                    s_max = (int32_t)(prm.max_penalty && prm.max_penalty < bound ? prm.max_penalty : bound);
                    wlo = m > (int32_t)kGrow ? m - (int32_t)kGrow : 0, whi = m + (int32_t)kGrow < nd - 1 ? m + (int32_t)kGrow : nd - 1;
                    clear(wlo, whi + 1);
                }
            }
        }
        if (!__any(have || !exhausted)) break;
        __syncthreads();  // staged strings, cleared columns and the last step's wavefronts are visible to the pair's lanes
        if (have) {
            const int32_t from = s ? (lo > 0 ? lo - 1 : 0) : m, to = s ? (hi < nd - 1 ? hi + 1 : nd - 1) : m;
            const bool sub = s >= x, open = s >= oe, ext = s >= e;
            const off_t *m_sub = M + (idx_t)(ms >= x ? ms - x : ms + rm - x) * nd;
            const off_t *m_open = M + (idx_t)(ms >= oe ? ms - oe : ms + rm - oe) * nd;
            const idx_t g_prev = (idx_t)(gs >= e ? gs - e : gs + rg - e) * nd;
            const off_t *i_prev = I + g_prev, *d_prev = D + g_prev;
            off_t *m_now = M + (idx_t)ms * nd, *i_now = I + (idx_t)gs * nd, *d_now = D + (idx_t)gs * nd;
            int32_t vmin = 0x7FFFFFFF, vmax = -1, done = 0;
            for (int32_t d = from + (int32_t)j; d <= to; d += kLanes) {
                int32_t ml = kNone, il = kNone, mr = kNone, dr = kNone, msb = kNone;
                if (d - 1 >= wlo) {
                    if (open) ml = m_open[d - 1];
                    if (ext) il = i_prev[d - 1];
                }
                if (d + 1 <= whi) {
                    if (open) mr = m_open[d + 1];
                    if (ext) dr = d_prev[d + 1];
                }
                if (sub) msb = m_sub[d];
                const int32_t k = d - m;
                Cell c = cell(ml, il, mr, dr, msb, k, n, m);
                if (!s) c.m = 0;
                if (c.m >= 0) {
                    c.m = extend(t, p, c.m, k, n, m);
                    vmin = d < vmin ? d : vmin, vmax = d > vmax ? d : vmax;
                    if (d == n && c.m >= n) done = 1;
                }
                i_now[d] = (off_t)c.i, d_now[d] = (off_t)c.d, m_now[d] = (off_t)c.m;
            }
            vmin = group_min<kLanes>(vmin), vmax = -group_min<kLanes>(-vmax), done = -group_min<kLanes>(-done);
            lo = vmin < lo ? vmin : lo, hi = vmax > hi ? vmax : hi;
            if (done || s >= s_max) {
                if (j == 0) {
                    if (done) {
                        out[row] = score_of((uint32_t)s);
                    } else if (prm.max_penalty && (uint32_t)s_max == prm.max_penalty) {
                        out[row] = -__builtin_inff();
                        if (valid) atomicAnd(valid + (row >> 6), ~(1ull << (row & 63)));
                        atomicAdd(&w.c->n_capped, 1ull);
                    } else {  // the hard bound without an alignment: a defect, reported and not spun on
                        out[row] = score_of((uint32_t)s_max);
                        atomicOr(&w.c->flags, 1ull);
                    }
                }
                have = false;
            } else {
                // keep a diagonal beyond the reached range initialised on either side
                if (lo - 1 < wlo && wlo > 0) {
                    const int32_t a = wlo > (int32_t)kGrow ? wlo - (int32_t)kGrow : 0;
                    clear(a, wlo);
                    wlo = a;
                }
                if (hi + 1 > whi && whi < nd - 1) {
                    const int32_t b = whi + (int32_t)kGrow < nd - 1 ? whi + (int32_t)kGrow : nd - 1;
                    clear(whi + 1, b + 1);
                    whi = b;
                }
                s++;
                ms = ms + 1 == rm ? 0 : ms + 1, gs = gs + 1 == rg ? 0 : gs + 1;
            }
        }
    }
}

__global__ void k_init(Ws w) {
    if (threadIdx.x || blockIdx.x) return;
    Counters c;
    memset(&c, 0, sizeof c);
    c.err_row = ~0ull;
    *w.c = c;
}

__global__ void k_finish(Col tc, Col pc, Params prm, Ws w, exg_align_score_result *res) {
    if (threadIdx.x || blockIdx.x) return;
    exg_align_score_result r;
    memset(&r, 0, sizeof r);
    r.n_capped = w.c->n_capped;
    r.n_global = w.c->n_list;
    r.flags = (uint32_t)w.c->flags;
    const uint64_t row = w.c->err_row;
    if (row != ~0ull) {
        r.error_code = EXG_PE_ALIGN_TOO_LONG;
        r.error_row = row;
        r.error_length = (uint64_t)tc.rows[row].x + pc.rows[row].x;
        r.error_limit = prm.max_pair_bytes;
    }
    *res = r;
}

}  // namespace alignfn
}  // namespace exg

using namespace exg;
using namespace exg::alignfn;

static_assert(sizeof(exg_align_score_result) == 64, "exg_align_score_result is 64 bytes");
static_assert(sizeof(Counters) == 64, "the counters are 64 bytes");

extern "C" uint64_t exg_align_workspace_bytes(uint64_t n_rows, uint64_t max_pair_bytes, uint32_t mismatch, uint32_t gap_opening,
                                              uint32_t gap_extension) {
    if (!params_ok(mismatch, gap_opening, gap_extension) || max_pair_bytes > kMaxPairBytes || n_rows >= 0xFFFFFFFFull) return 0;
    return ws_layout(n_rows, max_pair_bytes, mismatch, gap_opening, gap_extension, nullptr).bytes;
}

template <int kLanes>
static void launch_lds(uint32_t grid, uint32_t lds_bytes, hipStream_t s, const Col &tc, const Col &pc, uint64_t n, const Params &prm,
                       const Ws &w, uint32_t share, float *out, unsigned long long *valid) {
    hipLaunchKernelGGL((k_align<LdsPolicy, kLanes>), dim3(grid), dim3(64), lds_bytes, s, tc, pc, n, prm, w, share, out, valid);
}

extern "C" int exg_align_score(const exg_align_score_args *a) {
    if (!a || !a->d_result || ((uintptr_t)a->d_result & 7) || !a->d_workspace || ((uintptr_t)a->d_workspace & 15) ||
        (a->n_rows && (!a->d_text || !a->d_pattern || !a->d_out_float)) || ((uintptr_t)a->d_text & 15) || ((uintptr_t)a->d_pattern & 15) ||
        ((uintptr_t)a->d_out_valid & 7)) {
        set_error("exg_align_score: bad arguments (null or unaligned strings, output, workspace or result)");
        return EXG_E_INVALID_ARG;
    }
    if (!params_ok(a->mismatch, a->gap_opening, a->gap_extension)) {
        set_error("exg_align_score: mismatch %u, gap_opening %u, gap_extension %u (1..1023, 0..1023, 1..1023)", a->mismatch, a->gap_opening,
                  a->gap_extension);
        return EXG_E_INVALID_ARG;
    }
    if (a->max_pair_bytes > kMaxPairBytes) {
        set_error("exg_align_score: max_pair_bytes %llu (at most %llu)", (unsigned long long)a->max_pair_bytes, (unsigned long long)kMaxPairBytes);
        return EXG_E_INVALID_ARG;
    }
    if (a->n_rows >= 0xFFFFFFFFull) {
        set_error("exg_align_score: %llu rows (at most 2^32 - 2 a call)", (unsigned long long)a->n_rows);
        return EXG_E_INVALID_ARG;
    }
    if ((a->lanes && a->lanes != 16 && a->lanes != 32 && a->lanes != 64) || a->reserved) {
        set_error("exg_align_score: lanes %u (0, 16, 32 or 64), reserved %u (0)", a->lanes, a->reserved);
        return EXG_E_INVALID_ARG;
    }
    const Ws w = ws_layout(a->n_rows, a->max_pair_bytes, a->mismatch, a->gap_opening, a->gap_extension, a->d_workspace);
    if (a->workspace_bytes < w.bytes) {
        set_error("exg_align_score: workspace too small (%llu bytes, need %llu)", (unsigned long long)a->workspace_bytes,
                  (unsigned long long)w.bytes);
        return EXG_E_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)a->stream;
    const uint64_t n = a->n_rows;
    if (!n) {
        EXG_HIP_CHECK(hipMemsetAsync(a->d_result, 0, sizeof(exg_align_score_result), s));
        return EXG_OK;
    }
    int dev = 0, cus = 0;
    EXG_HIP_CHECK(hipGetDevice(&dev));
    EXG_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (cus < 1) cus = 1;
    const Col tc{(const uint4 *)a->d_text, (const uint8_t *)a->d_text_payload, a->text_payload_base};
    const Col pc{(const uint4 *)a->d_pattern, (const uint8_t *)a->d_pattern_payload, a->pattern_payload_base};
    Params prm;
    prm.x = a->mismatch, prm.o = a->gap_opening, prm.e = a->gap_extension;
    prm.rm = m_ring_depth(prm.x, prm.o, prm.e), prm.rg = gap_ring_depth(prm.e);
    prm.max_penalty = a->max_penalty, prm.max_pair_bytes = a->max_pair_bytes;
    // a pair's share of LDS: what the longest admissible pair takes, at most the workgroup's LDS over its pairs
    const uint32_t lanes = a->lanes ? a->lanes : kDefaultLanes, groups = 64 / lanes;
    const uint64_t need = (lds_need(depth_of(prm.x, prm.o, prm.e), a->max_pair_bytes) + 255) & ~255ull;
    const uint32_t share = (uint32_t)(need < kLdsPerWorkgroup / groups ? need : kLdsPerWorkgroup / groups);
    const uint32_t lds_bytes = share * groups;
    // persistent workgroups: what a CU holds by LDS (160 KiB) and by waves (32), no more than there are rows
    uint64_t per_cu = (160 * 1024) / lds_bytes;
    per_cu = per_cu > 32 ? 32 : per_cu;
    uint64_t grid = (n + groups - 1) / groups;
    grid = grid < per_cu * cus ? grid : per_cu * cus;
    hipLaunchKernelGGL(k_init, dim3(1), dim3(64), 0, s, w);
    unsigned long long *valid = (unsigned long long *)a->d_out_valid;
    if (lanes == 16)
        launch_lds<16>((uint32_t)grid, lds_bytes, s, tc, pc, n, prm, w, share, a->d_out_float, valid);
    else if (lanes == 32)
        launch_lds<32>((uint32_t)grid, lds_bytes, s, tc, pc, n, prm, w, share, a->d_out_float, valid);
    else
        launch_lds<64>((uint32_t)grid, lds_bytes, s, tc, pc, n, prm, w, share, a->d_out_float, valid);
    if (w.slot_entries)
        hipLaunchKernelGGL((k_align<GlobalPolicy, 64>), dim3(kSlots), dim3(64), 0, s, tc, pc, n, prm, w, 0u, a->d_out_float, valid);
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(64), 0, s, tc, pc, prm, w, a->d_result);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

extern "C" int exg_align_result(const exg_align_score_result *d_result, void *stream, exg_align_score_result *out) {
    if (!d_result || !out) {
        set_error("exg_align_result: null pointer");
        return EXG_E_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    EXG_HIP_CHECK(hipMemcpyAsync(out, d_result, sizeof(*out), hipMemcpyDeviceToHost, s));
    EXG_HIP_CHECK(hipStreamSynchronize(s));
    if (out->error_code) {
        char text[96];
        format_error(out->error_code, out->error_length, out->error_limit, text, sizeof text);
        set_error("%s in row %llu", text, (unsigned long long)out->error_row);
        return EXG_E_PARSE;
    }
    return EXG_OK;
}
