// exg_alignfn.hip — alignment_score / alignment_score_wfa_gap_affine (exon/src/exon/alignment_functions/module.cpp:264-329)
// on two duckdb::string_t columns that are still in HBM (include/exon_gpu.h: exg_align_score).  The rules and the recurrences
// are exg_alignfn.hpp's, the forward pass exg_align_core.hpp's (Forward, k_align); here are the method, the workspace, what
// is written when a pair ends (ScoreRec) and the C entry.
//
// The exact wavefront algorithm, score only.  A pair keeps, per diagonal k = h - v (index d = k + m, 0 .. n + m), the offsets
// of M for the last max(x, o + e) + 1 scores and of I and D for the last e + 1: a ring, indexed by s mod depth.  The lanes of
// a pair lie on neighbouring diagonals; one score step is one pass over the diagonals any wavefront has reached, widened by
// one on either side.  The columns of the ring a step may read are kept initialised: when the reached range
// comes within a diagonal of the initialised one, seven more diagonals are set to kNone in every wavefront of the ring.
//
// One body (k_align) serves two storage policies, the way LdsSrc / GlobalSrc serve the line scans, and — through its recorder
// — exg_alignstr.hip, which keeps the wavefronts this op drops:
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

// workspace: counters | list (u32 x n_rows) | kSlots slots of (rm + 2 rg) x (max_pair_bytes + 1) int32
struct Ws {
    Pass f;
    uint64_t bytes;
};
static Ws ws_layout(uint64_t n, uint64_t max_pair_bytes, uint32_t x, uint32_t o, uint32_t e, void *base) {
    Ws w;
    uint8_t *p = (uint8_t *)base;
    w.f.c = (Counters *)p, p += sizeof(Counters);
    w.f.list = (uint32_t *)p, p += ((n * 4 + 15) & ~15ull);
    w.f.rings = (int32_t *)p;
    w.f.ring_entries = ring_entries_of(x, o, e, max_pair_bytes);
    p += w.f.ring_entries * 4 * kSlots;
    w.bytes = (uint64_t)(p - (uint8_t *)base);
    return w;
}

// the recorder of the score op: no wavefront is kept, a pair's end writes its row
struct ScoreRec : NoHistory {
    struct Args {
        float *out;
        unsigned long long *valid;
    };
    const Args a;
    __device__ __forceinline__ ScoreRec(const Args &a, uint32_t) : a(a) {}
    template <class F>
    __device__ __forceinline__ bool ended(const F &f, bool done, bool) {
        if (f.j == 0) {
            if (done) {
                a.out[f.row] = score_of((uint32_t)f.s);
            } else if (f.capped()) {
                a.out[f.row] = -__builtin_inff();
                if (a.valid) atomicAnd(a.valid + (f.row >> 6), ~(1ull << (f.row & 63)));
                atomicAdd(&f.w.c->n_capped, 1ull);
            } else {  // the hard bound without an alignment: a defect, reported and not spun on
                a.out[f.row] = score_of((uint32_t)f.s_max);
                atomicOr(&f.w.c->flags, 1ull);
            }
        }
        return false;
    }
};

__global__ void k_finish(Col tc, Col pc, Params prm, Counters *c, exg_align_score_result *res) {
    if (threadIdx.x || blockIdx.x) return;
    exg_align_score_result r;
    memset(&r, 0, sizeof r);
    report(tc, pc, prm, c, &r);
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

extern "C" int exg_align_score(const exg_align_score_args *a) {
    if (const int rc = check_args("exg_align_score", a, a && a->n_rows && !a->d_out_float)) return rc;
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
    const Col tc{(const uint4 *)a->d_text, (const uint8_t *)a->d_text_payload, a->text_payload_base};
    const Col pc{(const uint4 *)a->d_pattern, (const uint8_t *)a->d_pattern_payload, a->pattern_payload_base};
    const Params prm = params_of(a->mismatch, a->gap_opening, a->gap_extension, a->max_penalty, a->max_pair_bytes);
    const ScoreRec::Args ra{a->d_out_float, (unsigned long long *)a->d_out_valid};
    Geometry g;
    if (const int rc = lds_geometry(a->lanes, prm, n, &g)) return rc;
    hipLaunchKernelGGL(k_init, dim3(1), dim3(64), 0, s, w.f.c);
    launch_lds<ScoreRec>(g, s, tc, pc, n, prm, w.f, ra);
    if (w.f.ring_entries)
        hipLaunchKernelGGL((k_align<GlobalPolicy, 64, ScoreRec>), dim3(kSlots), dim3(64), 0, s, tc, pc, n, prm, w.f, 0u, ra);
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(64), 0, s, tc, pc, prm, w.f.c, a->d_result);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

extern "C" int exg_align_result(const exg_align_score_result *d_result, void *stream, exg_align_score_result *out) {
    if (const int rc = fetch_result("exg_align_result", d_result, stream, out)) return rc;
    if (out->error_code) {
        char text[96];
        format_error(out->error_code, out->error_length, out->error_limit, text, sizeof text);
        set_error("%s in row %llu", text, (unsigned long long)out->error_row);
        return EXG_E_PARSE;
    }
    return EXG_OK;
}
