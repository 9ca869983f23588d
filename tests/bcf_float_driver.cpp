// bcf_float_driver.cpp — the BCF transcoder's float renderer (csrc/exg_bcf_float.hpp) compiled for the host: every float32 bit
// pattern it is given is rendered and read back the way the VCF path's parse_f32 reads a literal — digits, at most one '.',
// an optional exponent, the decimal significand and exponent into el_f32_bits (csrc/exg_float_el.hpp) — and must come back
// with the same bits.  usage: bcf_float_driver <n_random> <seed>; the edges are always run.  Prints one line per failure and
// "checked <n> failures <k>" at the end; the exit status is 1 when k > 0.  (tests/test_bcf_host.py builds and runs it.)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "exg_bcf_float.hpp"
#include "exg_float_el.hpp"

static std::string text_of(const exg::bcf::Txt &t) {
    std::string s;
    for (uint32_t i = 0; i < t.n; i++) s.push_back((char)t.at(i));
    return s;
}

// 0: the same bits came back
static int check(uint32_t bits) {
    const exg::bcf::Txt t = exg::bcf::render_f32(bits);
    if (t.n == 0 || t.n > 16) return 1;
    const std::string s = text_of(t);
    const uint32_t a = bits & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return s == "nan" ? 0 : 2;
    if (a == 0x7F800000u) return s == ((bits >> 31) ? "-inf" : "inf") ? 0 : 3;
    size_t i = 0;
    bool neg = false;
    if (s[i] == '-') neg = true, i++;
    uint64_t m = 0;
    int e10 = 0, nd = 0, sig = 0;
    bool dot = false;
    for (; i < s.size(); i++) {
        const char c = s[i];
        if (c == '.') {
            if (dot) return 4;
            dot = true;
            continue;
        }
        if (c < '0' || c > '9') break;
        nd++;
        if (m || c != '0') m = m * 10 + (uint64_t)(c - '0'), sig++;
        if (dot) e10--;
    }
    if (nd == 0 || sig > 19) return 5;
    if (i < s.size()) {
        if (s[i] != 'e') return 6;
        i++;
        bool eneg = false;
        if (i < s.size() && s[i] == '-') eneg = true, i++;
        if (i >= s.size()) return 7;
        int ev = 0;
        for (; i < s.size(); i++) {
            if (s[i] < '0' || s[i] > '9') return 8;
            ev = ev * 10 + (s[i] - '0');
        }
        e10 += eneg ? -ev : ev;
    }
    const uint32_t back = (m ? exg::el_f32_bits(m, e10) : 0u) | (neg ? 0x80000000u : 0u);
    return back == bits ? 0 : 9;
}

int main(int argc, char **argv) {
    const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 0;
    uint64_t x = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    std::vector<uint32_t> edges = {0u, 0x80000000u, 1u, 0x80000001u, 0x007FFFFFu, 0x00800000u, 0x7F7FFFFFu, 0xFF7FFFFFu,
                                   0x7F800000u, 0xFF800000u, 0x7FC00000u, 0xFFC00000u, 0x7F800003u, 0x3F800000u, 0x3F7FFFFFu, 0x3F800001u};
    for (uint32_t e = 0; e < 255; e++) edges.push_back(e << 23), edges.push_back((e << 23) | 0x80000000u);  // powers of two (and 0)
    for (int p = -45; p <= 38; p++) {
        const float f = (float)pow(10.0, p);
        uint32_t b;
        memcpy(&b, &f, 4);
        edges.push_back(b), edges.push_back(b + 1), edges.push_back(b ? b - 1 : 0);
    }
    for (uint32_t i = 0; i < 100000; i++) {  // small integers and hundredths, as files hold them
        const float f = (float)i, g = (float)i / 100.0f;
        uint32_t b;
        memcpy(&b, &f, 4), edges.push_back(b);
        memcpy(&b, &g, 4), edges.push_back(b);
    }
    uint64_t checked = 0, failures = 0;
    auto run = [&](uint32_t bits) {
        if (bits == 0x7F800001u || bits == 0x7F800002u) return;  // BCF's missing / end-of-vector: never rendered as numbers
        checked++;
        const int rc = check(bits);
        if (rc) {
            if (failures < 20) printf("FAIL %08x rc %d text %s\n", bits, rc, text_of(exg::bcf::render_f32(bits)).c_str());
            failures++;
        }
    };
    for (uint32_t b : edges) run(b);
    for (uint64_t i = 0; i < n; i++) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;  // xorshift64
        run((uint32_t)(x >> 16));
    }
    printf("checked %llu failures %llu\n", (unsigned long long)checked, (unsigned long long)failures);
    return failures ? 1 : 0;
}
