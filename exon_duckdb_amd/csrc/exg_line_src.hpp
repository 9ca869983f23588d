// exg_line_src.hpp — byte sources of the line tokenisers (VCF, BED): a row function template <class Src> reads its line
// through one of them.  LdsSrc: the fused scans (exg_fused_core.hpp), the line's bytes in the staged half; GlobalSrc: the
// general path and the k_*_far kernels, the line's bytes in global memory.  Src: b(i) byte, u32(i) 4 bytes at any alignment,
// u96(i) 12 bytes, str(i, len) -> string_t, tabs64(i) the '\t' mask of 64 bytes, tab_bits(i) the same out of a half's map.
#pragma once
#include "exg_fused_core.hpp"

namespace exg {

// validity bits of 64 consecutive rows starting at out_base (may be negative for unowned lanes)
__device__ __forceinline__ void store_validity64(uint64_t *words, unsigned long long bits, long long out_base,
                                                 uint32_t lane) {
    if (!words || !bits) return;
    if (out_base < 0) {
        bits >>= (unsigned long long)(-out_base);
        out_base = 0;
    }
    if (lane == 0 && bits) {
        uint32_t sh = (uint32_t)(out_base & 63);
        unsigned long long lo = bits << sh, hi = sh ? bits >> (64 - sh) : 0;
        if (lo) atomicOr((unsigned long long *)&words[out_base >> 6], lo);
        if (hi) atomicOr((unsigned long long *)&words[(out_base >> 6) + 1], hi);
    }
}

template <class L>
struct LdsSrc {
    const L &s;
    uint64_t ptr_of_e0;
    const uint16_t *tabs;  // '\t' bitmap of the staged half (bit p = byte kWin + p)
    __device__ __forceinline__ uint32_t b(int e) const { return ldb(s, e); }
    __device__ __forceinline__ uint32_t u32(int e) const { return ldu32(s, e); }  // reads stay inside the LDS slack
    __device__ __forceinline__ void u96(int e, uint32_t *w0, uint32_t *w1, uint32_t *w2) const {  // 12 bytes, one read
        const lds_v3u w = *reinterpret_cast<const lds_v3u *>(s.bytes + e);
        *w0 = w.x, *w1 = w.y, *w2 = w.z;
    }
    // '\t' mask of the 64 bytes from extended offset e on, classified here: four 16-byte reads at any alignment
    __device__ __forceinline__ unsigned long long tabs64(int e) const {
        typedef uint32_t lds_v4u __attribute__((ext_vector_type(4), aligned(1)));
        unsigned long long bits = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const lds_v4u w = *reinterpret_cast<const lds_v4u *>(s.bytes + e + 16 * q);
            bits |= (unsigned long long)match16(make_uint4(w.x, w.y, w.z, w.w), 0x09090909u) << (16 * q);
        }
        return bits;
    }
    // tab bits of the 64 bytes starting at extended offset e out of the half's map (only for lines that start inside the half)
    __device__ __forceinline__ bool tab_bits(int e, unsigned long long *out) const {
        if (!L::kHasTabs) return false;
        const int p = e - kWin;
        if (p < 0) return false;
        const unsigned long long *w = reinterpret_cast<const unsigned long long *>(tabs) + (p >> 6);
        const uint32_t sh = (uint32_t)p & 63u;
        const unsigned long long lo = w[0], hi = w[1];
        *out = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
        return true;
    }
    __device__ __forceinline__ uint4 str(int e, uint32_t len) const { return make_string_lds(s, e, len, ptr_of_e0); }
};

struct GlobalSrc {
    const uint8_t *p;  // d_in (16-byte aligned)
    uint64_t base;     // offset added to the (int) positions
    uint64_t payload_base;
    uint64_t limit;  // n_bytes rounded up to 16: reads past it are not allowed
    // Round 5: aligned dword / 16-byte loads + a byte shift instead of a load per byte (u32 was four byte loads with a bound check
    // each, tabs64 sixty-four: the rows k_vcf_far and k_vcf_lines parse out of global memory cost ~2 us of dependent loads each —
    // a cohort VCF has one such row per half).  An aligned block that begins below `limit` lies inside the buffer; the last
    // bytes of the buffer take the former byte path.
    __device__ __forceinline__ uint32_t b(int i) const { return p[base + (uint64_t)(int64_t)i]; }
    __device__ __forceinline__ uint32_t u32_slow(uint64_t o) const {
        uint32_t w = 0;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (o + k < limit) w |= (uint32_t)p[o + k] << (8 * k);
        return w;
    }
    __device__ __forceinline__ uint32_t u32(int i) const {
        const uint64_t o = base + (uint64_t)(int64_t)i, al = o & ~3ull;
        if (al + 8 > limit) return u32_slow(o);
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p + al);
        return __builtin_amdgcn_alignbyte(q[1], q[0], (uint32_t)(o & 3));
    }
    __device__ __forceinline__ void u96(int i, uint32_t *w0, uint32_t *w1, uint32_t *w2) const {
        const uint64_t o = base + (uint64_t)(int64_t)i, al = o & ~3ull;
        if (al + 16 > limit) {
            *w0 = u32_slow(o), *w1 = u32_slow(o + 4), *w2 = u32_slow(o + 8);
            return;
        }
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p + al);
        const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], sh = (uint32_t)(o & 3);
        *w0 = __builtin_amdgcn_alignbyte(d1, d0, sh);
        *w1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
        *w2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
    }
    __device__ __forceinline__ uint4 str(int i, uint32_t len) const {
        const uint64_t o = base + (uint64_t)(int64_t)i;
        if (((o & ~3ull) + 16) > limit) return make_string_global(p, o, len, payload_base);
        uint32_t w0, w1, w2;
        u96(i, &w0, &w1, &w2);
        uint4 r;
        r.x = len;
        if (len <= EXG_INLINE_LENGTH) {  // the bytes behind the field are not the string's: zeros
            const uint32_t n0 = len < 4u ? len : 4u, n1 = len < 4u ? 0u : len - 4u < 4u ? len - 4u : 4u, n2 = len < 8u ? 0u : len - 8u;
            r.y = n0 == 4 ? w0 : w0 & ((1u << (8 * n0)) - 1u);
            r.z = n1 == 4 ? w1 : w1 & ((1u << (8 * n1)) - 1u);
            r.w = n2 == 4 ? w2 : w2 & ((1u << (8 * n2)) - 1u);
        } else {
            const uint64_t ptr = payload_base + o;
            r.y = w0;
            r.z = (uint32_t)ptr;
            r.w = (uint32_t)(ptr >> 32);
        }
        return r;
    }
    __device__ __forceinline__ bool tab_bits(int, unsigned long long *) const { return false; }
    __device__ __forceinline__ unsigned long long tabs64(int base_i) const {
        const uint64_t o = base + (uint64_t)(int64_t)base_i, al = o & ~15ull;
        if (al + 80 > limit) {
            unsigned long long bits = 0;
#pragma unroll
            for (int q = 0; q < 16; q++) bits |= (unsigned long long)nib4(match4(u32_slow(o + 4 * q), 0x09090909u)) << (4 * q);
            return bits;
        }
        const uint4 *q = reinterpret_cast<const uint4 *>(p + al);
        const uint4 v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3], v4 = q[4];  // (five loads in flight)
        const unsigned long long lo = (unsigned long long)match16(v0, 0x09090909u) | ((unsigned long long)match16(v1, 0x09090909u) << 16) |
                                      ((unsigned long long)match16(v2, 0x09090909u) << 32) | ((unsigned long long)match16(v3, 0x09090909u) << 48);
        const unsigned long long hi = match16(v4, 0x09090909u);
        const uint32_t sh = (uint32_t)(o & 15);
        return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
    }
};

}  // namespace exg
