// exg_alignstr.hip — alignment_string / alignment_string_wfa_gap_affine (exon/src/exon/alignment_functions/module.cpp:150-247)
// on two duckdb::string_t columns that are still in HBM (include/exon_gpu.h: exg_align_string).  The rules, the recurrences
// and the backtrace are exg_alignfn.hpp's, the string readers and ring policies exg_align_core.hpp's; here is the work
// distribution.
//
// The method is the reference's memory_high, as the host scalar: the forward pass of exg_alignfn.hip (the ring in LDS while it
// fits a pair's share, in a slot of the workspace otherwise; rows claimed from an atomic counter; the lanes of a pair on
// neighbouring diagonals), and every step appends the diagonals it visited — M after extend, I and D, three planes of `width`
// entries — to the HISTORY SLOT of the pair, with one directory entry {start, from, width} a step.  Lanes store neighbouring
// entries.  When M[s, n - m] reaches n, one lane of the group walks the history back with backtrace_step (at most five reads
// an operation) and writes the run-length text backwards into the slot's text area; a text of up to 12 bytes goes straight
// into its string_t, a longer one is copied by the group's lanes to a staging area (bump-allocated: its order depends on the
// run, nothing else does).  Then the lengths of the long rows are scanned (exg_scan.hpp, as exg_cigar_op scans) and k_place
// moves each staged text to out_payload_base + its prefix sum: the output is a function of the input alone.
//
// Sizing: diagonal k needs s >= o + |k| e, so a step at score s visits at most min(max_pair_bytes + 1, 2 (s / e) + 3)
// diagonals; a slot holds the sum of that over s = 0 .. P, P = max_penalty or the bound of the longest admissible pair
// (history_entries).  "History full" and "capped" are therefore one event and no row needs a fallback; the kernel checks the
// slot's end all the same (flags bit 1).  Entries are 16-bit when max_pair_bytes < 30000.  kPairs slots = resident pairs.
#include "exg_align_core.hpp"
#include "exg_scan.hpp"

namespace exg {
namespace alignstr {
using namespace exg::alignfn;

static constexpr uint32_t kPairs = 1024;       // resident pairs = history slots: 0.92 GiB of them at max_pair_bytes 320, defaults, no cap
static constexpr uint32_t kDefaultLanes = 64;  // four waves a CU at kPairs slots; DESIGN 4.16
static constexpr uint64_t kShortEntries = 30000;  // max_pair_bytes below this: 16-bit history
static constexpr uint64_t kMaxWorkspace = 1ull << 48;
static constexpr uint64_t kNotStaged = ~0ull;

struct Counters {  // 64 bytes at the front of the workspace
    unsigned long long next_row, n_list, next_list, err_row, n_capped, flags, staged, pad;
};
struct Params {
    uint32_t x, o, e, rm, rg, max_penalty;
    uint64_t max_pair_bytes;
};
struct HStep {  // the directory entry of one score step
    uint64_t start;  // of the M plane, in entries from the slot's history; I at start + width, D at start + 2 width
    int32_t from, width;
};
// workspace: counters | list, rowlen (u32 x n) | rowpos (u64 x n) | offs (u64 x n + 1) | scan scratch | kSlots ring slots of
// the global pass | n_slots x (directory of P + 1 steps | history | text) | staging (out_capacity bytes)
struct Ws {
    Counters *c;
    uint32_t *list, *rowlen;
    uint64_t *rowpos, *offs, *tmp;
    int32_t *rings;
    uint8_t *slots, *stage;
    uint64_t ring_entries, slot_bytes, dir_bytes, hist_bytes, hist_entries, text_bytes, steps, bytes;
    uint32_t n_slots, hsize;
};
static Ws ws_layout(uint64_t n, uint64_t max_pair_bytes, uint32_t x, uint32_t o, uint32_t e, uint32_t max_penalty, uint64_t out_capacity,
                    void *base) {
    Ws w;
    uint64_t at = 0;
    auto take = [&](uint64_t b) {
        uint8_t *p = (uint8_t *)base + at;
        at += (b + 15) & ~15ull;
        return p;
    };
    w.c = (Counters *)take(sizeof(Counters));
    w.list = (uint32_t *)take(n * 4), w.rowlen = (uint32_t *)take(n * 4);
    w.rowpos = (uint64_t *)take(n * 8), w.offs = (uint64_t *)take((n + 1) * 8), w.tmp = (uint64_t *)take(xscan_tmp_entries(n) * 8);
    const bool all_lds = lds_need(depth_of(x, o, e), max_pair_bytes) <= kLdsPerWorkgroup / 4;
    w.ring_entries = all_lds ? 0 : (((uint64_t)depth_of(x, o, e) * (max_pair_bytes + 1) + 3) & ~3ull);
    w.rings = (int32_t *)take(w.ring_entries * 4 * kSlots);
    w.n_slots = n >= kPairs ? kPairs : (uint32_t)((n + 3) & ~3ull);
    const uint64_t P = history_steps(o, e, max_pair_bytes, max_penalty);
    w.hsize = max_pair_bytes < kShortEntries ? 2 : 4;
    w.hist_entries = 3 * history_entries(e, max_pair_bytes, P);
    w.steps = P + 1;
    w.dir_bytes = w.steps * sizeof(HStep);
    w.hist_bytes = (w.hist_entries * w.hsize + 15) & ~15ull;
    w.text_bytes = (2 * max_pair_bytes + 16 + 15) & ~15ull;
    w.slot_bytes = w.dir_bytes + w.hist_bytes + w.text_bytes;
    if (w.slot_bytes > kMaxWorkspace / kPairs || out_capacity > kMaxWorkspace) {
        w.bytes = 0;
        return w;
    }
    w.slots = take(w.slot_bytes * w.n_slots);
    w.stage = take(out_capacity);
    w.bytes = at <= kMaxWorkspace ? at : 0;
    return w;
}

// the stored wavefronts of one pair, as backtrace_step reads them
template <class H>
struct HistView {
    const HStep *dir;
    const H *hist;
    int32_t m_len;
    __device__ __forceinline__ int32_t at(int32_t s, int32_t k, int32_t plane) const {
        if (s < 0) return kNone;
        const HStep st = dir[s];
        const int32_t d = k + m_len - st.from;
        if (d < 0 || d >= st.width) return kNone;
        return (int32_t)hist[st.start + (uint64_t)(plane * st.width + d)];
    }
    __device__ __forceinline__ int32_t m(int32_t s, int32_t k) const { return at(s, k, 0); }
    __device__ __forceinline__ int32_t i(int32_t s, int32_t k) const { return at(s, k, 1); }
    __device__ __forceinline__ int32_t d(int32_t s, int32_t k) const { return at(s, k, 2); }
};

struct Out {
    uint4 *strings;
    float *score;
    unsigned long long *valid;
    uint64_t capacity;
};

// P: where the ring lives (exg_align_core.hpp), H: the history's entry type
template <class P, int kLanes, class H>
__global__ __launch_bounds__(64) void k_align_str(Col tc, Col pc, uint64_t n_rows, Params prm, Ws w, uint32_t lds_share, Out out) {
    typedef typename P::off_t off_t;
    typedef typename P::idx_t idx_t;
    extern __shared__ uint32_t s_mem[];
    const uint32_t j = threadIdx.x & (kLanes - 1), g = threadIdx.x / kLanes;
    const int32_t x = (int32_t)prm.x, oe = (int32_t)(prm.o + prm.e), e = (int32_t)prm.e, rm = (int32_t)prm.rm, rg = (int32_t)prm.rg;
    const uint32_t depth = prm.rm + 2 * prm.rg;
    const uint64_t limit = P::kLds ? n_rows : w.c->n_list;
    unsigned long long *counter = P::kLds ? &w.c->next_row : &w.c->next_list;
    // this group's history slot
    uint8_t *slot = w.slots + (uint64_t)(blockIdx.x * (64 / kLanes) + g) * w.slot_bytes;
    HStep *dir = reinterpret_cast<HStep *>(slot);
    H *hist = reinterpret_cast<H *>(slot + w.dir_bytes);
    uint8_t *text_end = slot + w.slot_bytes;

    bool have = false, exhausted = false, tracing = false;
    uint64_t row = 0, hpos = 0;
    unsigned long long next = 0, last = 0;
    int32_t n = 0, m = 0, nd = 1, s = 0, s_max = 0;
    int32_t lo = 0, hi = 0, wlo = 0, whi = 0;
    int32_t ms = 0, gs = 0;
    typename P::Str t{}, p{};
    off_t *M = nullptr, *I = nullptr, *D = nullptr;

    auto clear = [&](int32_t a, int32_t b) {
        for (uint32_t r = 0; r < depth; r++) {
            off_t *ring = M + (idx_t)r * nd;
            for (int32_t d = a + (int32_t)j; d < b; d += kLanes) ring[d] = (off_t)kNone;
        }
    };
    // a row without a CIGAR: NULL (16 zero bytes), no payload
    auto no_string = [&](uint64_t r) {
        out.strings[r] = make_uint4(0, 0, 0, 0);
        w.rowlen[r] = 0;
    };

    for (;;) {
        if (!have && !exhausted) {
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
                    if (j == 0) {
                        atomicMin(&w.c->err_row, (unsigned long long)row);
                        no_string(row);
                    }
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
                        M = w.rings + (uint64_t)blockIdx.x * w.ring_entries;
                    }
                    I = M + (idx_t)rm * nd, D = I + (idx_t)rg * nd;
                    s = 0, ms = 0, gs = 0, lo = hi = m, hpos = 0;
                    const uint32_t bound = penalty_bound(prm.o, prm.e, (uint64_t)n, (uint64_t)m);
                    s_max = (int32_t)(prm.max_penalty && prm.max_penalty < bound ? prm.max_penalty : bound);
                    wlo = m > (int32_t)kGrow ? m - (int32_t)kGrow : 0, whi = m + (int32_t)kGrow < nd - 1 ? m + (int32_t)kGrow : nd - 1;
                    clear(wlo, whi + 1);
                }
            }
        }
        if (!__any(have || !exhausted)) break;
        __syncthreads();  // staged strings, cleared columns, the last step's wavefronts and history are visible to the pair's lanes
        if (have && tracing) {
            // the pair is done at penalty s: one lane walks the history back and writes the text backwards
            uint32_t len = 0;
            uint64_t pos = kNotStaged;
            if (j == 0) {
                const HistView<H> view{dir, hist, m};
                RunWriter rw{text_end, text_end - w.text_bytes, 0, 0, false};
                const bool ok = backtrace(view, s, x, (int32_t)prm.o, e, n, m, &rw);
                const uint8_t *begin = rw.finish();
                len = ok ? (uint32_t)(text_end - begin) : 0u;
                if (!ok) atomicOr(&w.c->flags, 4ull);
                if (len <= EXG_INLINE_LENGTH) {
                    uint32_t v[4] = {len, 0, 0, 0};
                    for (uint32_t i = 0; i < len; i++) v[1 + (i >> 2)] |= (uint32_t)begin[i] << (8 * (i & 3));
                    out.strings[row] = make_uint4(v[0], v[1], v[2], v[3]);
                } else {
                    pos = atomicAdd(&w.c->staged, (unsigned long long)len);
                    if (pos + len > out.capacity) pos = kNotStaged;  // more text than out_capacity: only the length counts
                }
                w.rowlen[row] = len, w.rowpos[row] = pos;
                if (out.score) out.score[row] = score_of((uint32_t)s);
            }
            len = __shfl(len, 0, kLanes), pos = (uint64_t)__shfl((unsigned long long)pos, 0, kLanes);
            if (pos != kNotStaged) {
                __threadfence_block();  // lane 0's text, for the lanes that copy it
                const uint8_t *begin = text_end - len;
                for (uint32_t i = j; i < len; i += kLanes) w.stage[pos + i] = begin[i];
            }
            have = false, tracing = false;
        } else if (have) {
            const int32_t from = s ? (lo > 0 ? lo - 1 : 0) : m, to = s ? (hi < nd - 1 ? hi + 1 : nd - 1) : m;
            const int32_t width = to - from + 1;
            const bool room = (uint64_t)s < w.steps && hpos + 3ull * (uint64_t)width <= w.hist_entries;
            const bool sub = s >= x, open = s >= oe, ext = s >= e;
            const off_t *m_sub = M + (idx_t)(ms >= x ? ms - x : ms + rm - x) * nd;
            const off_t *m_open = M + (idx_t)(ms >= oe ? ms - oe : ms + rm - oe) * nd;
            const idx_t g_prev = (idx_t)(gs >= e ? gs - e : gs + rg - e) * nd;
            const off_t *i_prev = I + g_prev, *d_prev = D + g_prev;
            off_t *m_now = M + (idx_t)ms * nd, *i_now = I + (idx_t)gs * nd, *d_now = D + (idx_t)gs * nd;
            H *h_m = hist + hpos - from, *h_i = h_m + width, *h_d = h_i + width;
            int32_t vmin = 0x7FFFFFFF, vmax = -1, done = 0;
            if (room) {
                if (j == 0) dir[s] = HStep{hpos, from, width};
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
                    h_m[d] = (H)c.m, h_i[d] = (H)c.i, h_d[d] = (H)c.d;
                }
            }
            hpos += 3ull * (uint64_t)width;
            vmin = group_min<kLanes>(vmin), vmax = -group_min<kLanes>(-vmax), done = -group_min<kLanes>(-done);
            lo = vmin < lo ? vmin : lo, hi = vmax > hi ? vmax : hi;
            if (done) {
                tracing = true;  // after the next barrier: the history is the other lanes' stores
            } else if (s >= s_max || !room) {
                if (j == 0) {
                    no_string(row);
                    if (room && prm.max_penalty && (uint32_t)s_max == prm.max_penalty) {
                        if (out.score) out.score[row] = -__builtin_inff();
                        if (out.valid) atomicAnd(out.valid + (row >> 6), ~(1ull << (row & 63)));
                        atomicAdd(&w.c->n_capped, 1ull);
                    } else {  // the hard bound without an alignment, or a full slot: defects, reported and not spun on
                        if (out.score) out.score[row] = score_of((uint32_t)s_max);
                        atomicOr(&w.c->flags, room ? 1ull : 2ull);
                    }
                }
                have = false;
            } else {
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

struct LongLenF {
    const uint32_t *len;
    __device__ uint64_t operator()(uint64_t i) const { return len[i] > EXG_INLINE_LENGTH ? len[i] : 0u; }
};

// every long row's text from the staging area to its prefix sum, and its string_t; a wave moves the long rows of its 64 one
// after another with all lanes.  Nothing is placed when the whole does not fit.
__global__ __launch_bounds__(256) void k_place(uint64_t n, Ws w, uint4 *out_strings, uint8_t *payload, uint64_t capacity, uint64_t base) {
    const uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool fits = w.offs[n] <= capacity;
    uint32_t len = row < n ? w.rowlen[row] : 0u;
    uint64_t off = 0, pos = 0;
    bool place = fits && len > EXG_INLINE_LENGTH;
    if (place) {
        off = w.offs[row], pos = w.rowpos[row];
        place = pos != kNotStaged && off + len <= capacity;
    }
    if (place) {
        const uint8_t *src = w.stage + pos;
        const uint64_t ptr = base + off;
        out_strings[row] = make_uint4(len, (uint32_t)src[0] | ((uint32_t)src[1] << 8) | ((uint32_t)src[2] << 16) | ((uint32_t)src[3] << 24),
                                      (uint32_t)ptr, (uint32_t)(ptr >> 32));
    }
    unsigned long long todo = __ballot(place);
    while (todo) {
        const int from = __ffsll(todo) - 1;
        todo &= todo - 1;
        const uint32_t l = __shfl(len, from, 64);
        const uint64_t o = (uint64_t)__shfl((unsigned long long)off, from, 64), q = (uint64_t)__shfl((unsigned long long)pos, from, 64);
        for (uint32_t i = lane; i < l; i += 64) payload[o + i] = w.stage[q + i];
    }
}

__global__ void k_finish(Col tc, Col pc, uint64_t n, Params prm, Ws w, uint64_t capacity, struct exg_align_string_result *res) {
    if (threadIdx.x || blockIdx.x) return;
    struct exg_align_string_result r;
    memset(&r, 0, sizeof r);
    r.n_capped = w.c->n_capped;
    r.n_global = w.c->n_list;
    r.flags = (uint32_t)w.c->flags;
    r.out_bytes = w.offs[n];
    r.out_capacity = capacity;
    const uint64_t row = w.c->err_row;
    if (row != ~0ull) {
        r.error_code = EXG_PE_ALIGN_TOO_LONG;
        r.error_row = row;
        r.error_length = (uint64_t)tc.rows[row].x + pc.rows[row].x;
        r.error_limit = prm.max_pair_bytes;
    }
    *res = r;
}

template <int kLanes>
static void launch_lds(uint32_t grid, uint32_t lds_bytes, hipStream_t s, const Col &tc, const Col &pc, uint64_t n, const Params &prm,
                       const Ws &w, uint32_t share, const Out &out) {
    hipLaunchKernelGGL((k_align_str<LdsPolicy, kLanes, int16_t>), dim3(grid), dim3(64), lds_bytes, s, tc, pc, n, prm, w, share, out);
}

}  // namespace alignstr
}  // namespace exg

using namespace exg;
using namespace exg::alignstr;

static_assert(sizeof(struct exg_align_string_result) == 64, "exg_align_string_result is 64 bytes");
static_assert(sizeof(Counters) == 64 && sizeof(HStep) == 16, "the counters are 64 bytes, a directory entry 16");

extern "C" uint64_t exg_align_string_workspace_bytes(uint64_t n_rows, uint64_t max_pair_bytes, uint32_t mismatch, uint32_t gap_opening,
                                                     uint32_t gap_extension, uint32_t max_penalty, uint64_t out_capacity) {
    if (!params_ok(mismatch, gap_opening, gap_extension) || max_pair_bytes > kMaxPairBytes || n_rows >= 0xFFFFFFFFull) return 0;
    return ws_layout(n_rows, max_pair_bytes, mismatch, gap_opening, gap_extension, max_penalty, out_capacity, nullptr).bytes;
}

extern "C" int exg_align_string(const exg_align_string_args *a) {
    if (!a || !a->d_result || ((uintptr_t)a->d_result & 7) || !a->d_workspace || ((uintptr_t)a->d_workspace & 15) ||
        (a->n_rows && (!a->d_text || !a->d_pattern || !a->d_out_strings)) || ((uintptr_t)a->d_text & 15) || ((uintptr_t)a->d_pattern & 15) ||
        ((uintptr_t)a->d_out_strings & 15) || (a->out_capacity && !a->d_out_payload) || ((uintptr_t)a->d_out_valid & 7) ||
        ((uintptr_t)a->d_out_score & 3)) {
        set_error("exg_align_string: bad arguments (null or unaligned strings, output, workspace or result)");
        return EXG_E_INVALID_ARG;
    }
    if (!params_ok(a->mismatch, a->gap_opening, a->gap_extension)) {
        set_error("exg_align_string: mismatch %u, gap_opening %u, gap_extension %u (1..1023, 0..1023, 1..1023)", a->mismatch, a->gap_opening,
                  a->gap_extension);
        return EXG_E_INVALID_ARG;
    }
    if (a->max_pair_bytes > kMaxPairBytes) {
        set_error("exg_align_string: max_pair_bytes %llu (at most %llu)", (unsigned long long)a->max_pair_bytes, (unsigned long long)kMaxPairBytes);
        return EXG_E_INVALID_ARG;
    }
    if (a->n_rows >= 0xFFFFFFFFull) {
        set_error("exg_align_string: %llu rows (at most 2^32 - 2 a call)", (unsigned long long)a->n_rows);
        return EXG_E_INVALID_ARG;
    }
    if ((a->lanes && a->lanes != 16 && a->lanes != 32 && a->lanes != 64) || a->reserved) {
        set_error("exg_align_string: lanes %u (0, 16, 32 or 64), reserved %u (0)", a->lanes, a->reserved);
        return EXG_E_INVALID_ARG;
    }
    const Ws w = ws_layout(a->n_rows, a->max_pair_bytes, a->mismatch, a->gap_opening, a->gap_extension, a->max_penalty, a->out_capacity,
                           a->d_workspace);
    if (!w.bytes) {
        set_error("exg_align_string: the wavefront history of max_pair_bytes %llu at max_penalty %u passes 2^48 bytes (set a max_penalty)",
                  (unsigned long long)a->max_pair_bytes, a->max_penalty);
        return EXG_E_INVALID_ARG;
    }
    if (a->workspace_bytes < w.bytes) {
        set_error("exg_align_string: workspace too small (%llu bytes, need %llu)", (unsigned long long)a->workspace_bytes,
                  (unsigned long long)w.bytes);
        return EXG_E_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)a->stream;
    const uint64_t n = a->n_rows;
    if (!n) {
        EXG_HIP_CHECK(hipMemsetAsync(a->d_result, 0, sizeof(struct exg_align_string_result), s));
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
    const Out out{(uint4 *)a->d_out_strings, a->d_out_score, (unsigned long long *)a->d_out_valid, a->out_capacity};
    // a pair's share of LDS as in exg_align_score; the grid is bounded by the history slots as well
    const uint32_t lanes = a->lanes ? a->lanes : kDefaultLanes, groups = 64 / lanes;
    const uint64_t need = (lds_need(depth_of(prm.x, prm.o, prm.e), a->max_pair_bytes) + 255) & ~255ull;
    const uint32_t share = (uint32_t)(need < kLdsPerWorkgroup / groups ? need : kLdsPerWorkgroup / groups);
    const uint32_t lds_bytes = share * groups;
    uint64_t per_cu = (160 * 1024) / lds_bytes;
    per_cu = per_cu > 32 ? 32 : per_cu;
    uint64_t grid = (n + groups - 1) / groups;
    grid = grid < per_cu * cus ? grid : per_cu * cus;
    grid = grid < w.n_slots / groups ? grid : w.n_slots / groups;
    hipLaunchKernelGGL(k_init, dim3(1), dim3(64), 0, s, w);
    if (lanes == 16)
        launch_lds<16>((uint32_t)grid, lds_bytes, s, tc, pc, n, prm, w, share, out);
    else if (lanes == 32)
        launch_lds<32>((uint32_t)grid, lds_bytes, s, tc, pc, n, prm, w, share, out);
    else
        launch_lds<64>((uint32_t)grid, lds_bytes, s, tc, pc, n, prm, w, share, out);
    if (w.ring_entries) {
        const uint32_t g = w.n_slots < kSlots ? w.n_slots : kSlots;
        if (w.hsize == 2)
            hipLaunchKernelGGL((k_align_str<GlobalPolicy, 64, int16_t>), dim3(g), dim3(64), 0, s, tc, pc, n, prm, w, 0u, out);
        else
            hipLaunchKernelGGL((k_align_str<GlobalPolicy, 64, int32_t>), dim3(g), dim3(64), 0, s, tc, pc, n, prm, w, 0u, out);
    }
    launch_xscan(LongLenF{w.rowlen}, n, w.offs, w.tmp, s);
    hipLaunchKernelGGL(k_place, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, n, w, out.strings, a->d_out_payload, a->out_capacity,
                       a->out_payload_base);
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(64), 0, s, tc, pc, n, prm, w, a->out_capacity, a->d_result);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

extern "C" int exg_align_string_result(const struct exg_align_string_result *d_result, void *stream, struct exg_align_string_result *out) {
    if (!d_result || !out) {
        set_error("exg_align_string_result: null pointer");
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
    if (out->out_bytes > out->out_capacity) {
        set_error("exg_align_string: the CIGARs take %llu payload bytes, out_capacity is %llu", (unsigned long long)out->out_bytes,
                  (unsigned long long)out->out_capacity);
        return EXG_E_CAPACITY;
    }
    return EXG_OK;
}
