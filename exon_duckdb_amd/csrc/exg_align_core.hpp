// exg_align_core.hpp — the wavefront forward pass of the two alignment translation units (exg_alignfn.hip: the scores,
// exg_alignstr.hip: the CIGARs), stated once: the two ways a pair's strings are read, the two storage policies of the ring,
// the claim of rows, a pair's set-up, the score step and the ring's growth (Forward), the kernel around them (k_align), and
// what both C entries share on the host.  What an op does with a pair goes through its RECORDER R, built in the kernel from
// R::Args: too_long(row), by lane 0 for a row over max_pair_bytes; begin_step(f, from, width), false when there is no room to
// record the step; store(d, cell), M after extend; ended(f, done, room) — done: M[s, n - m] reached n, else max_penalty, the
// hard bound or a refused step ended the pair — true to hold the pair for trace(f) behind the next barrier.  NoHistory has the
// hooks of a recorder that keeps no wavefronts: constants and empty bodies, gone when compiled.
// Internal; everything here is inline, static or a template, so both objects may define it.  The rules are exg_alignfn.hpp's.
#pragma once
#include "exg_alignfn.hpp"
#include "exg_strcol.hpp"

namespace exg {
namespace alignfn {

static constexpr uint32_t kGrow = 7;             // diagonals initialised at a time on either side: 15 at the start, a store a lane
static constexpr uint32_t kSlots = 256;          // workgroups of the global pass = slots of the workspace
static constexpr uint32_t kLdsPerWorkgroup = 65536;  // LDS of a workgroup, shared by its 64 / lanes pairs
static constexpr uint32_t kDefaultLanes = 64;    // DESIGN 4.13 and 4.16 have the measurements

struct Counters {  // 64 bytes at the front of either workspace; staged is the string op's, the score op leaves it 0
    unsigned long long next_row, n_list, next_list, err_row, n_capped, flags, staged, pad;
};
struct Params {
    uint32_t x, o, e, rm, rg, max_penalty;
    uint64_t max_pair_bytes;
};
// what the forward pass takes of a workspace: the counters, the list of the rows that do not fit LDS, kSlots ring slots
struct Pass {
    Counters *c;
    uint32_t *list;
    int32_t *rings;
    uint64_t ring_entries;
};
// LDS bytes a pair of n + m = nm bytes takes: 16-bit rings and the two staged strings (whole dwords, two of slack each)
__host__ __device__ static inline uint64_t lds_need(uint32_t depth, uint64_t nm) { return 2ull * depth * (nm + 1) + nm + 24; }
static inline uint32_t depth_of(uint32_t x, uint32_t o, uint32_t e) { return m_ring_depth(x, o, e) + 2 * gap_ring_depth(e); }
// int32 entries of a ring slot; none when every admissible row fits LDS with the whole workgroup's share to itself
static inline uint64_t ring_entries_of(uint32_t x, uint32_t o, uint32_t e, uint64_t max_pair_bytes) {
    const uint32_t depth = depth_of(x, o, e);
    return lds_need(depth, max_pair_bytes) <= kLdsPerWorkgroup / 4 ? 0 : (((uint64_t)depth * (max_pair_bytes + 1) + 3) & ~3ull);
}

// A string where the scan left it, at any alignment.  Only aligned dwords that hold a byte of the string are read, so every
// read lies in a page the string lies in; what the result holds past the string's end is unspecified (extend clips).
struct GlobalStr {
    const uint8_t *p;
    uint32_t len;
    __device__ __forceinline__ uint32_t get4(uint32_t h) const {  // bytes [h, h + 4), h < len
        const uintptr_t a = (uintptr_t)p + h, end = (uintptr_t)p + len;
        const uint32_t mis = (uint32_t)a & 3u;
        const uint32_t *w = reinterpret_cast<const uint32_t *>(a - mis);
        const uint32_t w0 = w[0], w1 = (mis && (uintptr_t)(w + 1) < end) ? w[1] : 0u;
        return __builtin_amdgcn_alignbyte(w1, w0, mis);
    }
    __device__ __forceinline__ uint64_t get8(uint32_t h) const {  // bytes [h, h + 8), h < len
        const uintptr_t a = (uintptr_t)p + h, end = (uintptr_t)p + len;
        const uint32_t mis = (uint32_t)a & 3u;
        const uint32_t *w = reinterpret_cast<const uint32_t *>(a - mis);
        const uint32_t w0 = w[0], w1 = (uintptr_t)(w + 1) < end ? w[1] : 0u, w2 = (mis && (uintptr_t)(w + 2) < end) ? w[2] : 0u;
        return (uint64_t)__builtin_amdgcn_alignbyte(w1, w0, mis) | ((uint64_t)__builtin_amdgcn_alignbyte(w2, w1, mis) << 32);
    }
};
// A string staged in LDS from byte 0 of a dword array with two dwords of slack behind its last one
struct LdsStr {
    const uint32_t *w;
    uint32_t len;
    __device__ __forceinline__ uint64_t get8(uint32_t h) const {
        const uint32_t i = h >> 2, mis = h & 3u;
        const uint32_t w0 = w[i], w1 = w[i + 1], w2 = w[i + 2];
        return (uint64_t)__builtin_amdgcn_alignbyte(w1, w0, mis) | ((uint64_t)__builtin_amdgcn_alignbyte(w2, w1, mis) << 32);
    }
};
__host__ __device__ static inline uint32_t str_words(uint32_t len) { return (len + 3) / 4 + 2; }

struct LdsPolicy {
    static constexpr bool kLds = true;
    typedef int16_t off_t;
    typedef uint32_t idx_t;
    typedef LdsStr Str;
};
struct GlobalPolicy {
    static constexpr bool kLds = false;
    typedef int32_t off_t;
    typedef uint64_t idx_t;
    typedef GlobalStr Str;
};

template <class Str>
__device__ __forceinline__ int32_t extend(const Str &t, const Str &p, int32_t h, int32_t k, int32_t n, int32_t m) {
    int32_t v = h - k;
    for (;;) {
        const int32_t left = n - h < m - v ? n - h : m - v;  // never past either string's end
        if (left <= 0) break;
        int32_t c = (int32_t)equal_prefix8(t.get8((uint32_t)h), p.get8((uint32_t)v));
        c = c < left ? c : left;
        h += c, v += c;
        if (c < 8) break;
    }
    return h;
}

template <int kLanes, typename T>
__device__ __forceinline__ T group_min(T v) {
#pragma unroll
    for (int d = kLanes / 2; d; d >>= 1) {
        const T o = __shfl_xor(v, d, kLanes);
        v = o < v ? o : v;
    }
    return v;
}

struct NoHistory {
    __device__ __forceinline__ void too_long(uint64_t) {}
    template <class F>
    __device__ __forceinline__ bool begin_step(const F &, int32_t, int32_t) {
        return true;
    }
    __device__ __forceinline__ void store(int32_t, const Cell &) {}
    template <class F>
    __device__ __forceinline__ void trace(const F &) {}
};

// what claim and step leave a group with: no pair (claim next), no rows to claim any more, a pair to step, a pair the recorder holds
enum Turn { kNoPair, kNoRows, kPair, kHeld };

// The forward pass of one group of kLanes lanes: its pair and what it does to it.
template <class P, int kLanes>
struct Forward {
    typedef typename P::off_t off_t;
    typedef typename P::idx_t idx_t;
    static constexpr int kGroupLanes = kLanes;
    const Col &tc, &pc;
    const Params &prm;
    const Pass &w;
    const uint64_t n_rows;
    const uint32_t lds_share;
    const uint32_t j = threadIdx.x & (kLanes - 1), g = threadIdx.x / kLanes;  // the lane of the group, the group of the wave
    const int32_t x = (int32_t)prm.x, oe = (int32_t)(prm.o + prm.e), e = (int32_t)prm.e, rm = (int32_t)prm.rm, rg = (int32_t)prm.rg;
    const uint32_t depth = prm.rm + 2 * prm.rg;
    const uint64_t limit = P::kLds ? n_rows : w.c->n_list;
    unsigned long long *const counter = P::kLds ? &w.c->next_row : &w.c->next_list;
    // the state of this group's pair (uniform over the group's lanes)
    uint64_t row = 0;
    unsigned long long next = 0, last = 0;  // the rows this group has claimed and not begun
    int32_t n = 0, m = 0, nd = 1, s = 0, s_max = 0;
    int32_t lo = 0, hi = 0, wlo = 0, whi = 0;  // diagonals reached; diagonals initialised
    int32_t ms = 0, gs = 0;                    // s mod rm, s mod rg
    typename P::Str t{}, p{};
    off_t *M = nullptr, *I = nullptr, *D = nullptr;

    // max_penalty ended the pair (and not the hard bound 2o + e(n + m), which ends the loop whatever happens)
    __device__ __forceinline__ bool capped() const { return prm.max_penalty && (uint32_t)s_max == prm.max_penalty; }

    // every wavefront of the ring := kNone on the diagonals [a, b) (M, I and D lie behind one another: depth rows of nd)
    __device__ __forceinline__ void clear(int32_t a, int32_t b) {
        for (uint32_t slot = 0; slot < depth; slot++) {
            off_t *ring = M + (idx_t)slot * nd;
            for (int32_t d = a + (int32_t)j; d < b; d += kLanes) ring[d] = (off_t)kNone;
        }
    }

    // The next row, if there is one and this pass takes it: strings staged, ring cleared around diagonal 0, s = 0.
    // Rows that fit LDS are claimed eight at a time: one counter takes ~10^8 atomics a second, which is what 3 M
    // near-identical read pairs ran at when every pair paid one.  A pair of the global pass is claimed alone.
    template <class R>
    __device__ __forceinline__ Turn claim(R &rec) {
        Turn turn = kNoPair;
        if (next == last) {
            constexpr unsigned long long kClaim = P::kLds ? 8 : 1;
            if (j == 0) next = atomicAdd(counter, kClaim);
            next = __shfl(next, 0, kLanes);
            last = next + kClaim < limit ? next + kClaim : limit;
            if (next >= limit) turn = kNoRows, last = next;
        }
        if (turn != kNoRows) {
            const unsigned long long idx = next++;
            row = P::kLds ? idx : w.list[idx];
            const uint4 tv = tc.rows[row], pv = pc.rows[row];
            const uint64_t nm = (uint64_t)tv.x + pv.x;
            if (P::kLds && nm > prm.max_pair_bytes) {
                if (j == 0) {
                    atomicMin(&w.c->err_row, (unsigned long long)row);
                    rec.too_long(row);
                }
            } else if (P::kLds && lds_need(depth, nm) > lds_share) {
                if (j == 0) w.list[atomicAdd(&w.c->n_list, 1ull)] = (uint32_t)row;
            } else {
                turn = kPair;
                n = (int32_t)tv.x, m = (int32_t)pv.x, nd = n + m + 1;
                const GlobalStr gt{src_of(tc, row, tv), tv.x}, gp{src_of(pc, row, pv), pv.x};
                if constexpr (P::kLds) {
                    extern __shared__ uint32_t s_mem[];
                    uint32_t *base = s_mem + g * (lds_share / 4);
                    const uint32_t tw = str_words(tv.x), pw = str_words(pv.x);
                    for (uint32_t i = j; 4 * i < tv.x; i += kLanes) base[i] = gt.get4(4 * i);
                    for (uint32_t i = j; 4 * i < pv.x; i += kLanes) base[tw + i] = gp.get4(4 * i);
                    t = LdsStr{base, tv.x}, p = LdsStr{base + tw, pv.x};
                    M = reinterpret_cast<off_t *>(base + tw + pw);
                } else {
                    t = gt, p = gp;
                    M = w.rings + (uint64_t)blockIdx.x * w.ring_entries;
                }
                I = M + (idx_t)rm * nd, D = I + (idx_t)rg * nd;
                s = 0, ms = 0, gs = 0, lo = hi = m;
                const uint32_t bound = penalty_bound(prm.o, prm.e, (uint64_t)n, (uint64_t)m);
                s_max = (int32_t)(prm.max_penalty && prm.max_penalty < bound ? prm.max_penalty : bound);
                wlo = m > (int32_t)kGrow ? m - (int32_t)kGrow : 0, whi = m + (int32_t)kGrow < nd - 1 ? m + (int32_t)kGrow : nd - 1;
                clear(wlo, whi + 1);
            }
        }
        return turn;
    }

    // One score step: a pass over the diagonals any wavefront has reached, widened by one on either side; then the pair is
    // done, stopped, or goes on to s + 1 with a diagonal beyond the reached range initialised on either side.
    template <class R>
    __device__ __forceinline__ Turn step(R &rec) {
        const int32_t from = s ? (lo > 0 ? lo - 1 : 0) : m, to = s ? (hi < nd - 1 ? hi + 1 : nd - 1) : m;
        const bool room = rec.begin_step(*this, from, to - from + 1);
        const bool sub = s >= x, open = s >= oe, ext = s >= e;
        const off_t *m_sub = M + (idx_t)(ms >= x ? ms - x : ms + rm - x) * nd;
        const off_t *m_open = M + (idx_t)(ms >= oe ? ms - oe : ms + rm - oe) * nd;
        const idx_t g_prev = (idx_t)(gs >= e ? gs - e : gs + rg - e) * nd;
        const off_t *i_prev = I + g_prev, *d_prev = D + g_prev;
        off_t *m_now = M + (idx_t)ms * nd, *i_now = I + (idx_t)gs * nd, *d_now = D + (idx_t)gs * nd;
        int32_t vmin = 0x7FFFFFFF, vmax = -1, done = 0;
        if (room) {
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
                rec.store(d, c);
            }
        }
        vmin = group_min<kLanes>(vmin), vmax = -group_min<kLanes>(-vmax), done = -group_min<kLanes>(-done);
        lo = vmin < lo ? vmin : lo, hi = vmax > hi ? vmax : hi;
        if (done || s >= s_max || !room) return rec.ended(*this, done, room) ? kHeld : kNoPair;
        {
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
        return kPair;
    }
};

// One body serves both ops (R), both storage policies (P) and 16, 32 or 64 lanes a pair.  The pairs of a wave step in lockstep,
// one barrier a step; a group whose pair has ended claims the next row.  slot: the group's number among the resident ones.
template <class P, int kLanes, class R>
__global__ __launch_bounds__(64) void k_align(Col tc, Col pc, uint64_t n_rows, Params prm, Pass w, uint32_t lds_share, typename R::Args ra) {
    Forward<P, kLanes> f{tc, pc, prm, w, n_rows, lds_share};
    R rec(ra, blockIdx.x * (64 / kLanes) + f.g);
    bool have = false, exhausted = false, held = false;  // (uniform over the group's lanes)
    for (;;) {
        if (!have && !exhausted) {
            const Turn t = f.claim(rec);
            have = t == kPair, exhausted = t == kNoRows;
        }
        if (!__any(have || !exhausted)) break;
        __syncthreads();  // staged strings, cleared columns, the last step's wavefronts and records are visible to the pair's lanes
        if (have && held) {
            rec.trace(f);
            have = held = false;
        } else if (have) {
            const Turn t = f.step(rec);
            have = t != kNoPair, held = t == kHeld;
        }
    }
}

static __global__ void k_init(Counters *c) {
    if (threadIdx.x || blockIdx.x) return;
    Counters v;
    memset(&v, 0, sizeof v);
    v.err_row = ~0ull;
    *c = v;
}

// what both result blocks report of a run: the counters, and the lowest too-long row if there is one
template <class Res>
__device__ __forceinline__ void report(const Col &tc, const Col &pc, const Params &prm, const Counters *c, Res *r) {
    r->n_capped = c->n_capped, r->n_global = c->n_list, r->flags = (uint32_t)c->flags;
    const uint64_t row = c->err_row;
    if (row == ~0ull) return;
    r->error_code = EXG_PE_ALIGN_TOO_LONG, r->error_row = row;
    r->error_length = (uint64_t)tc.rows[row].x + pc.rows[row].x, r->error_limit = prm.max_pair_bytes;
}

// ---- the host side of both C entries ------------------------------------------------------------------------------
static inline Params params_of(uint32_t mismatch, uint32_t gap_opening, uint32_t gap_extension, uint32_t max_penalty, uint64_t max_pair_bytes) {
    return Params{mismatch, gap_opening, gap_extension, m_ring_depth(mismatch, gap_opening, gap_extension), gap_ring_depth(gap_extension),
                  max_penalty, max_pair_bytes};
}

// the checks of what the two args structs have in common; bad_out: the op's own pointer checks
template <class A>
static int check_args(const char *fn, const A *a, bool bad_out) {
    if (!a || bad_out || !a->d_result || ((uintptr_t)a->d_result & 7) || !a->d_workspace || ((uintptr_t)a->d_workspace & 15) ||
        (a->n_rows && (!a->d_text || !a->d_pattern)) || ((uintptr_t)a->d_text & 15) || ((uintptr_t)a->d_pattern & 15) ||
        ((uintptr_t)a->d_out_valid & 7)) {
        set_error("%s: bad arguments (null or unaligned strings, output, workspace or result)", fn);
    } else if (!params_ok(a->mismatch, a->gap_opening, a->gap_extension)) {
        set_error("%s: mismatch %u, gap_opening %u, gap_extension %u (1..1023, 0..1023, 1..1023)", fn, a->mismatch, a->gap_opening,
                  a->gap_extension);
    } else if (a->max_pair_bytes > kMaxPairBytes) {
        set_error("%s: max_pair_bytes %llu (at most %llu)", fn, (unsigned long long)a->max_pair_bytes, (unsigned long long)kMaxPairBytes);
    } else if (a->n_rows >= 0xFFFFFFFFull) {
        set_error("%s: %llu rows (at most 2^32 - 2 a call)", fn, (unsigned long long)a->n_rows);
    } else if ((a->lanes && a->lanes != 16 && a->lanes != 32 && a->lanes != 64) || a->reserved) {
        set_error("%s: lanes %u (0, 16, 32 or 64), reserved %u (0)", fn, a->lanes, a->reserved);
    } else {
        return EXG_OK;
    }
    return EXG_E_INVALID_ARG;
}

// The launch of the LDS pass.  A pair's share of LDS: what the longest admissible pair takes, at most the workgroup's LDS over
// its pairs.  Persistent workgroups: what a CU holds by LDS (160 KiB) and by waves (32), no more than there are rows.
struct Geometry {
    uint32_t lanes, groups, share, lds_bytes;
    uint64_t grid;
};
static int lds_geometry(uint32_t lanes, const Params &prm, uint64_t n, Geometry *g) {
    int dev = 0, cus = 0;
    EXG_HIP_CHECK(hipGetDevice(&dev));
    EXG_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    g->lanes = lanes ? lanes : kDefaultLanes, g->groups = 64 / g->lanes;
    const uint64_t need = (lds_need(prm.rm + 2 * prm.rg, prm.max_pair_bytes) + 255) & ~255ull;
    g->share = (uint32_t)(need < kLdsPerWorkgroup / g->groups ? need : kLdsPerWorkgroup / g->groups);
    g->lds_bytes = g->share * g->groups;
    const uint64_t per_cu = (160 * 1024) / g->lds_bytes, fit = (per_cu > 32 ? 32 : per_cu) * (cus < 1 ? 1 : cus);
    g->grid = (n + g->groups - 1) / g->groups;
    g->grid = g->grid < fit ? g->grid : fit;
    return EXG_OK;
}
template <class R>
static void launch_lds(const Geometry &g, hipStream_t s, const Col &tc, const Col &pc, uint64_t n, const Params &prm, const Pass &w,
                       const typename R::Args &ra) {
    const dim3 grid((uint32_t)g.grid), block(64);
    if (g.lanes == 16)
        hipLaunchKernelGGL((k_align<LdsPolicy, 16, R>), grid, block, g.lds_bytes, s, tc, pc, n, prm, w, g.share, ra);
    else if (g.lanes == 32)
        hipLaunchKernelGGL((k_align<LdsPolicy, 32, R>), grid, block, g.lds_bytes, s, tc, pc, n, prm, w, g.share, ra);
    else
        hipLaunchKernelGGL((k_align<LdsPolicy, 64, R>), grid, block, g.lds_bytes, s, tc, pc, n, prm, w, g.share, ra);
}

}  // namespace alignfn
}  // namespace exg
