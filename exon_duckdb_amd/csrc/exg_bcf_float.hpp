// exg_bcf_float.hpp — float32 -> decimal text for the BCF transcoder (exg_bcf.hip), in registers: at most 16 characters.
//
// The text is read back by the VCF path's parse_f32 (exg_parse.hpp), which is correctly rounded; what must hold is that the
// float comes back with the same bits, not a canonical spelling.  Nine significant digits of (double)f do that
// (FLT_DECIMAL_DIG): neighbouring floats are at least 2^-24 apart relatively, nine digits at most 10^-8, so a decimal within
// one unit of the ninth digit of f still lies nearer to f than to either neighbour — the scaling below (a few double
// multiplications, each within 2^-53) is far inside that.  Spelling: trailing zeros of the nine digits are dropped; a value
// whose digits fit is written plainly ("50", "0.0312": parse_f32's one-division path takes up to seven digits), the rest as
// <digits>e<exponent> ("123456789e-17").  Compiles for the device and for the host (tests/bcf_float_driver.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define EXG_BCF_HD __host__ __device__
#else
#define EXG_BCF_HD
#endif

namespace exg {
namespace bcf {

// up to 16 characters in two registers (a runtime-indexed byte array would live in scratch memory)
struct Txt {
    uint64_t lo = 0, hi = 0;
    uint32_t n = 0;
    EXG_BCF_HD void push(uint32_t c) {
        if (n < 8) lo |= (uint64_t)c << (8 * n);
        else if (n < 16) hi |= (uint64_t)c << (8 * (n - 8));
        n++;
    }
    EXG_BCF_HD uint32_t at(uint32_t i) const { return (uint32_t)((i < 8 ? lo >> (8 * i) : hi >> (8 * (i - 8))) & 0xFF); }
};

EXG_BCF_HD inline uint32_t ndigits64(uint64_t v) {
    uint32_t d = 1;
    while (v >= 10) v /= 10, d++;
    return d;
}
EXG_BCF_HD inline void push_uint(Txt &t, uint64_t v) {  // at most 10 digits here
    const uint32_t d = ndigits64(v);
    uint64_t div = 1;
    for (uint32_t i = 1; i < d; i++) div *= 10;
    for (uint32_t i = 0; i < d; i++) {
        t.push('0' + (uint32_t)(v / div % 10));
        div /= 10;
    }
}
EXG_BCF_HD inline Txt render_i64(int64_t v) {  // |v| < 10^15
    Txt t;
    uint64_t a = (uint64_t)v;
    if (v < 0) t.push('-'), a = 0 - a;
    push_uint(t, a);
    return t;
}

// 10^k for 0 <= k < 64 (10^1 .. 10^16 are exact doubles; the products above are within a few 2^-53)
EXG_BCF_HD inline double pow10_small(uint32_t k) {
    double p = 1.0, b = 10.0;
    for (uint32_t i = 0; i < 6; i++) {
        if ((k >> i) & 1) p *= b;
        b *= b;
    }
    return p;
}
EXG_BCF_HD inline double scale10(double x, int k) { return k >= 0 ? x * pow10_small((uint32_t)k) : x / pow10_small((uint32_t)-k); }

// any bit pattern (the caller has taken out BCF's two reserved ones: missing, end-of-vector)
EXG_BCF_HD inline Txt render_f32(uint32_t bits) {
    Txt t;
    const uint32_t a = bits & 0x7FFFFFFFu;
    if (a > 0x7F800000u) {
        t.push('n'), t.push('a'), t.push('n');
        return t;
    }
    if (bits >> 31) t.push('-');
    if (a == 0x7F800000u) {
        t.push('i'), t.push('n'), t.push('f');
        return t;
    }
    if (a == 0) {
        t.push('0');
        return t;
    }
    float f;
    __builtin_memcpy(&f, &a, 4);
    const double x = (double)f;  // exact, and a normal double whatever f is
    uint64_t xb;
    __builtin_memcpy(&xb, &x, 8);
    const int e2 = (int)((xb >> 52) & 0x7FF) - 1023;
    int e10 = (e2 * 1233) >> 12;  // floor(e2 log10 2), or one less
    uint64_t m = 0;
    for (int tries = 0; tries < 3; tries++) {  // nine digits: m in [10^8, 10^9)
        m = (uint64_t)(scale10(x, 8 - e10) + 0.5);
        if (m >= 1000000000ull) e10++;
        else if (m < 100000000ull) e10--;
        else break;
    }
    if (m >= 1000000000ull) m = 100000000ull;  // (999999999.6 rounded up behind the last try: e10 was raised for it)
    int E = e10 - 8;  // the value is m x 10^E
    while (m % 10 == 0) m /= 10, E++;
    const int k = (int)ndigits64(m);
    if (E >= 0 && k + E <= 10) {
        push_uint(t, m);
        for (int i = 0; i < E; i++) t.push('0');
    } else if (E < 0 && -E < k) {  // the point inside the digits
        uint64_t div = 1;
        for (int i = 0; i < -E; i++) div *= 10;
        push_uint(t, m / div);
        t.push('.');
        const uint64_t frac = m % div;
        for (int i = (int)ndigits64(frac); i < -E; i++) t.push('0');
        push_uint(t, frac);
    } else if (E < 0 && -E <= 12) {  // 0.000ddd
        t.push('0'), t.push('.');
        for (int i = k; i < -E; i++) t.push('0');
        push_uint(t, m);
    } else {
        push_uint(t, m);
        t.push('e');
        if (E < 0) t.push('-');
        push_uint(t, (uint64_t)(E < 0 ? -E : E));
    }
    return t;
}

}  // namespace bcf
}  // namespace exg
