// exg_strcol.hpp — what the scalar ops on duckdb::string_t columns in HBM share (exg_seqfn.hip, exg_cigarfn.hip and, through
// exg_align_core.hpp, the two alignment units): the column, the search of the long rows, the string_t packers, the error
// epilogue and the result fetch.  Internal; everything here is inline or a template.
#pragma once
#include "exg_common.hpp"

namespace exg {

struct Col {
    const uint4 *rows;
    const uint8_t *base;
    uint64_t payload_base;
};
__device__ __forceinline__ const uint8_t *src_of(const Col &c, uint64_t r, uint4 v) {
    if (v.x <= EXG_INLINE_LENGTH) return reinterpret_cast<const uint8_t *>(c.rows + r) + 4;
    return c.base + (((uint64_t)v.z | ((uint64_t)v.w << 32)) - c.payload_base);
}
// rows a tile of tile space touches at the most: first + last + the whole rows (13 bytes and more) between
constexpr uint32_t tile_rows(uint32_t tile) { return tile / (EXG_INLINE_LENGTH + 1) + 3; }

// largest k in [lo, hi) with a[k] <= pos, for a[lo] <= pos < a[hi]; one wave, 64 probes a round
__device__ __forceinline__ uint64_t wave_search(const uint64_t *__restrict__ a, uint64_t lo, uint64_t hi, uint64_t pos) {
    const uint32_t lane = lane_id();
    while (hi - lo > 1) {
        const uint64_t step = (hi - lo + 63) >> 6;
        uint64_t idx = lo + (lane + 1) * step;
        if (idx > hi) idx = hi;  // (a[hi] > pos: a clamped probe never counts)
        const uint64_t c = __popcll(__ballot(a[idx] <= pos));
        const uint64_t nh = lo + (c + 1) * step;
        lo += c * step;
        hi = nh < hi ? nh : hi;
    }
    return lo;
}

// a string_t from its bytes: put_byte gathers up to 12 of them (or the 4 of a prefix) into dwords
__device__ __forceinline__ void put_byte(uint32_t *o, uint32_t i, uint32_t b) { o[i >> 2] |= b << (8 * (i & 3)); }
__device__ __forceinline__ uint4 inline_string(uint32_t len, const uint32_t *o) { return make_uint4(len, o[0], o[1], o[2]); }
__device__ __forceinline__ uint4 long_string(uint32_t len, uint32_t prefix, uint64_t ptr) {
    return make_uint4(len, prefix, (uint32_t)ptr, (uint32_t)(ptr >> 32));
}

// the smallest error key of a wave, one atomicMin a wave (lane: the caller's number in its wave)
__device__ __forceinline__ void wave_min_error(uint64_t key, uint64_t *err, uint32_t lane) {
#pragma unroll
    for (int dlt = 32; dlt; dlt >>= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)key, dlt, 64);
        key = o < key ? o : key;
    }
    if (lane == 0 && key != kNoError) atomicMin((unsigned long long *)err, (unsigned long long)key);
}

// the result block of a *_result function on the host, once the stream has run; fn names the caller in the message
template <class R>
static int fetch_result(const char *fn, const R *d_result, void *stream, R *out) {
    if (!d_result || !out) {
        set_error("%s: null pointer", fn);
        return EXG_E_INVALID_ARG;
    }
    EXG_HIP_CHECK(hipMemcpyAsync(out, d_result, sizeof(*out), hipMemcpyDeviceToHost, (hipStream_t)stream));
    EXG_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return EXG_OK;
}

}  // namespace exg
