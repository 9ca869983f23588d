// exg_vcf_region.hip — exg_vcf_region_keep: which rows of a scanned VCF batch overlap a region, as keep words for the reader's row
// selection (vcf_query).  The rules are exg_vcf_region.hpp's, the same code the host driver runs.
//
// A lane takes a row, a wave a word of 64 rows: chrom's string_t (16 B a lane, coalesced) and POS decide almost every row —
// another chrom, or pos inside [start, end].  Only a row of the region's chrom that begins in front of `start` reads REF's length
// and walks its INFO text for `END=`, byte by byte in its own lane; behind an index those are the few rows that reach into the
// region from the left.  One ballot makes the word, lane 0 stores it: rows >= n_rows vote 0, so the last word's tail is zero.
// No LDS, no scratch, no workspace.
#include "exg_strcol.hpp"
#include "exg_vcf_region.hpp"

namespace exg {
namespace vcf_region {

static constexpr uint32_t kGrid = 2048;  // workgroups of four waves that take the words in turn

__global__ __launch_bounds__(256) void k_keep(Col chrom, const uint4 *__restrict__ ref, const int64_t *__restrict__ pos, Col info, uint64_t n,
                                              const uint8_t *__restrict__ name, uint32_t name_len, int64_t start, int64_t end, uint64_t *__restrict__ keep) {
    const uint32_t lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint64_t words = (n + 63) / 64;
    for (uint64_t w = wave; w < words; w += n_waves) {
        const uint64_t r = w * 64 + lane;
        bool k = false;
        if (r < n) {
            const uint4 c = chrom.rows[r];
            if (same_name(src_of(chrom, r, c), c.x, name, name_len)) {
                const int64_t p = pos[r];
                if (p >= start) {
                    k = p <= end;  // E4
                } else {
                    const uint4 iv = info.rows[r];
                    k = overlaps(p, ref[r].x, src_of(info, r, iv), iv.x, start, end);
                }
            }
        }
        const unsigned long long word = __ballot(k);
        if (lane == 0) keep[w] = word;
    }
}

}  // namespace vcf_region
}  // namespace exg

using namespace exg;

extern "C" int exg_vcf_region_keep(const exg_vcf_region_args *a) {
    if (!a || (a->n_rows && (!a->d_chrom || !a->d_ref || !a->d_pos || !a->d_info || !a->d_keep || !a->d_name)) || ((uintptr_t)a->d_chrom & 15) ||
        ((uintptr_t)a->d_ref & 15) || ((uintptr_t)a->d_info & 15) || ((uintptr_t)a->d_pos & 7) || ((uintptr_t)a->d_keep & 7)) {
        set_error("exg_vcf_region_keep: bad arguments (null or unaligned column, name or keep words)");
        return EXG_E_INVALID_ARG;
    }
    if (!a->name_len || a->start < 1 || a->end < a->start || a->reserved) {
        set_error("exg_vcf_region_keep: bad region (an empty name, start %lld below 1, end %lld below start, or a reserved word that is not 0)",
                  (long long)a->start, (long long)a->end);
        return EXG_E_INVALID_ARG;
    }
    if (!a->n_rows) return EXG_OK;
    const uint64_t words = (a->n_rows + 63) / 64;
    const uint32_t grid = (uint32_t)((words + 3) / 4 < vcf_region::kGrid ? (words + 3) / 4 : vcf_region::kGrid);
    const Col chrom{(const uint4 *)a->d_chrom, (const uint8_t *)a->d_payload, a->payload_base};
    const Col info{(const uint4 *)a->d_info, (const uint8_t *)a->d_payload, a->payload_base};
    hipLaunchKernelGGL(vcf_region::k_keep, dim3(grid), dim3(256), 0, (hipStream_t)a->stream, chrom, (const uint4 *)a->d_ref, a->d_pos, info, a->n_rows,
                       a->d_name, a->name_len, a->start, a->end, a->d_keep);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}
