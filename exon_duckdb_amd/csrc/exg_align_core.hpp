// exg_align_core.hpp — what the two alignment translation units share on the device (exg_alignfn.hip: the scores,
// exg_alignstr.hip: the CIGARs): a string_t column, the two ways a pair's strings are read, the two storage policies of the
// wavefront ring, extend and the group reduction.  Internal; everything here is inline or a template, so both objects may
// define it.  The rules are exg_alignfn.hpp's.
#pragma once
#include "exg_alignfn.hpp"
#include "exg_common.hpp"

namespace exg {
namespace alignfn {

static constexpr uint32_t kGrow = 7;             // diagonals initialised at a time on either side: 15 at the start, a store a lane
static constexpr uint32_t kSlots = 256;          // workgroups of the global pass = slots of the workspace
static constexpr uint32_t kLdsPerWorkgroup = 65536;  // LDS of a workgroup, shared by its 64 / lanes pairs

struct Col {
    const uint4 *rows;
    const uint8_t *base;
    uint64_t payload_base;
};
// LDS bytes a pair of n + m = nm bytes takes: 16-bit rings and the two staged strings (whole dwords, two of slack each)
__host__ __device__ static inline uint64_t lds_need(uint32_t depth, uint64_t nm) { return 2ull * depth * (nm + 1) + nm + 24; }
static inline uint32_t depth_of(uint32_t x, uint32_t o, uint32_t e) { return m_ring_depth(x, o, e) + 2 * gap_ring_depth(e); }

__device__ __forceinline__ const uint8_t *src_of(const Col &c, uint64_t r, uint4 v) {
    if (v.x <= EXG_INLINE_LENGTH) return reinterpret_cast<const uint8_t *>(c.rows + r) + 4;
    return c.base + (((uint64_t)v.z | ((uint64_t)v.w << 32)) - c.payload_base);
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

}  // namespace alignfn
}  // namespace exg
