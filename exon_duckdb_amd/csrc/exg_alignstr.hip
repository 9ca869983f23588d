// exg_alignstr.hip — alignment_string / alignment_string_wfa_gap_affine (exon/src/exon/alignment_functions/module.cpp:150-247)
// on two duckdb::string_t columns that are still in HBM (include/exon_gpu.h: exg_align_string).  The rules, the recurrences
// and the backtrace are exg_alignfn.hpp's, the forward pass exg_align_core.hpp's (Forward, k_align); here are the workspace,
// the recorder that keeps the wavefronts and walks them back (HistoryRec), k_place and the C entry.
//
// The method is the reference's memory_high, as the host scalar: the forward pass of exg_align_score (the ring in LDS while it
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
static constexpr uint64_t kShortEntries = 30000;  // max_pair_bytes below this: 16-bit history
static constexpr uint64_t kMaxWorkspace = 1ull << 48;
static constexpr uint64_t kNotStaged = ~0ull;

struct HStep {  // the directory entry of one score step
    uint64_t start;  // of the M plane, in entries from the slot's history; I at start + width, D at start + 2 width
    int32_t from, width;
};
// workspace: counters | list, rowlen (u32 x n) | rowpos (u64 x n) | offs (u64 x n + 1) | scan scratch | kSlots ring slots of
// the global pass | n_slots x (directory of P + 1 steps | history | text) | staging (out_capacity bytes)
struct Ws {
    Pass f;
    uint32_t *rowlen;
    uint64_t *rowpos, *offs, *tmp;
    uint8_t *slots, *stage;
    uint64_t slot_bytes, dir_bytes, hist_bytes, hist_entries, text_bytes, steps, bytes;
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
    w.f.c = (Counters *)take(sizeof(Counters));
    w.f.list = (uint32_t *)take(n * 4), w.rowlen = (uint32_t *)take(n * 4);
    w.rowpos = (uint64_t *)take(n * 8), w.offs = (uint64_t *)take((n + 1) * 8), w.tmp = (uint64_t *)take(xscan_tmp_entries(n) * 8);
    w.f.ring_entries = ring_entries_of(x, o, e, max_pair_bytes);
    w.f.rings = (int32_t *)take(w.f.ring_entries * 4 * kSlots);
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

// The recorder of the string op.  H: the history's entry type.  Every step's wavefronts go to the group's history slot; when the
// pair is done, the next round of the kernel's loop — behind the barrier: the history is the other lanes' stores — walks them
// back.  hpos is 0 between pairs.
struct Out {
    Ws w;
    uint4 *strings;
    float *score;
    unsigned long long *valid;
    uint64_t capacity;
};
template <class H>
struct HistoryRec {
    typedef Out Args;
    const Out &out;
    const Ws &w = out.w;
    HStep *dir;
    H *hist, *h_m = nullptr, *h_i = nullptr, *h_d = nullptr;  // the slot's history; this step's planes, by diagonal
    uint8_t *text_end;
    uint64_t hpos = 0;

    __device__ __forceinline__ HistoryRec(const Out &out, uint32_t slot_no) : out(out) {
        uint8_t *slot = w.slots + (uint64_t)slot_no * w.slot_bytes;
        dir = reinterpret_cast<HStep *>(slot), hist = reinterpret_cast<H *>(slot + w.dir_bytes), text_end = slot + w.slot_bytes;
    }
    // a row without a CIGAR: NULL (16 zero bytes), no payload
    __device__ __forceinline__ void too_long(uint64_t r) {
        out.strings[r] = make_uint4(0, 0, 0, 0);
        w.rowlen[r] = 0;
    }
    template <class F>
    __device__ __forceinline__ bool begin_step(const F &f, int32_t from, int32_t width) {
        const bool room = (uint64_t)f.s < w.steps && hpos + 3ull * (uint64_t)width <= w.hist_entries;
        h_m = hist + hpos - from, h_i = h_m + width, h_d = h_i + width;
        if (room && f.j == 0) dir[f.s] = HStep{hpos, from, width};
        hpos += 3ull * (uint64_t)width;
        return room;
    }
    __device__ __forceinline__ void store(int32_t d, const Cell &c) { h_m[d] = (H)c.m, h_i[d] = (H)c.i, h_d[d] = (H)c.d; }
    template <class F>
    __device__ __forceinline__ bool ended(const F &f, bool done, bool room) {
        if (done) return true;
        hpos = 0;
        if (f.j == 0) {
            too_long(f.row);
            if (room && f.capped()) {
                if (out.score) out.score[f.row] = -__builtin_inff();
                if (out.valid) atomicAnd(out.valid + (f.row >> 6), ~(1ull << (f.row & 63)));
                atomicAdd(&f.w.c->n_capped, 1ull);
            } else {  // the hard bound without an alignment, or a full slot: defects, reported and not spun on
                if (out.score) out.score[f.row] = score_of((uint32_t)f.s_max);
                atomicOr(&f.w.c->flags, room ? 1ull : 2ull);
            }
        }
        return false;
    }
    // the pair is done at penalty s: one lane walks the history back and writes the text backwards; a text of up to 12 bytes
    // goes into its string_t, a longer one is copied to the staging area by the group's lanes
    template <class F>
    __device__ __forceinline__ void trace(const F &f) {
        constexpr int kLanes = F::kGroupLanes;
        uint32_t len = 0;
        uint64_t pos = kNotStaged;
        if (f.j == 0) {
            const HistView<H> view{dir, hist, f.m};
            RunWriter rw{text_end, text_end - w.text_bytes, 0, 0, false};
            const bool ok = backtrace(view, f.s, f.x, (int32_t)f.prm.o, f.e, f.n, f.m, &rw);
            const uint8_t *begin = rw.finish();
            len = ok ? (uint32_t)(text_end - begin) : 0u;
            if (!ok) atomicOr(&f.w.c->flags, 4ull);
            if (len <= EXG_INLINE_LENGTH) {
                uint32_t v[3] = {0, 0, 0};
                for (uint32_t i = 0; i < len; i++) put_byte(v, i, begin[i]);
                out.strings[f.row] = inline_string(len, v);
            } else {
                pos = atomicAdd(&f.w.c->staged, (unsigned long long)len);
                if (pos + len > out.capacity) pos = kNotStaged;  // more text than out_capacity: only the length counts
            }
            w.rowlen[f.row] = len, w.rowpos[f.row] = pos;
            if (out.score) out.score[f.row] = score_of((uint32_t)f.s);
        }
        len = __shfl(len, 0, kLanes), pos = (uint64_t)__shfl((unsigned long long)pos, 0, kLanes);
        if (pos != kNotStaged) {
            __threadfence_block();  // lane 0's text, for the lanes that copy it
            const uint8_t *begin = text_end - len;
            for (uint32_t i = f.j; i < len; i += kLanes) w.stage[pos + i] = begin[i];
        }
        hpos = 0;
    }
};

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
        uint32_t prefix = 0;
        for (uint32_t i = 0; i < 4; i++) put_byte(&prefix, i, src[i]);
        out_strings[row] = long_string(len, prefix, base + off);
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
    r.out_bytes = w.offs[n], r.out_capacity = capacity;
    report(tc, pc, prm, w.f.c, &r);
    *res = r;
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
    const bool bad = a && ((a->n_rows && !a->d_out_strings) || ((uintptr_t)a->d_out_strings & 15) || (a->out_capacity && !a->d_out_payload) ||
                           ((uintptr_t)a->d_out_score & 3));
    if (const int rc = check_args("exg_align_string", a, bad)) return rc;
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
    const Col tc{(const uint4 *)a->d_text, (const uint8_t *)a->d_text_payload, a->text_payload_base};
    const Col pc{(const uint4 *)a->d_pattern, (const uint8_t *)a->d_pattern_payload, a->pattern_payload_base};
    const Params prm = params_of(a->mismatch, a->gap_opening, a->gap_extension, a->max_penalty, a->max_pair_bytes);
    const Out out{w, (uint4 *)a->d_out_strings, a->d_out_score, (unsigned long long *)a->d_out_valid, a->out_capacity};
    // the geometry of exg_align_score; the grid is bounded by the history slots as well
    Geometry g;
    if (const int rc = lds_geometry(a->lanes, prm, n, &g)) return rc;
    g.grid = g.grid < w.n_slots / g.groups ? g.grid : w.n_slots / g.groups;
    hipLaunchKernelGGL(k_init, dim3(1), dim3(64), 0, s, w.f.c);
    launch_lds<HistoryRec<int16_t>>(g, s, tc, pc, n, prm, w.f, out);
    if (w.f.ring_entries) {
        const uint32_t slots = w.n_slots < kSlots ? w.n_slots : kSlots;
        if (w.hsize == 2)
            hipLaunchKernelGGL((k_align<GlobalPolicy, 64, HistoryRec<int16_t>>), dim3(slots), dim3(64), 0, s, tc, pc, n, prm, w.f, 0u, out);
        else
            hipLaunchKernelGGL((k_align<GlobalPolicy, 64, HistoryRec<int32_t>>), dim3(slots), dim3(64), 0, s, tc, pc, n, prm, w.f, 0u, out);
    }
    launch_xscan(LongLenF{w.rowlen}, n, w.offs, w.tmp, s);
    hipLaunchKernelGGL(k_place, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, n, w, out.strings, a->d_out_payload, a->out_capacity,
                       a->out_payload_base);
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(64), 0, s, tc, pc, n, prm, w, a->out_capacity, a->d_result);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

extern "C" int exg_align_string_result(const struct exg_align_string_result *d_result, void *stream, struct exg_align_string_result *out) {
    if (const int rc = fetch_result("exg_align_string_result", d_result, stream, out)) return rc;
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
