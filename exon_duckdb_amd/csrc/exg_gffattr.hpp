// exg_gffattr.hpp — the rules of gff_parse_attributes(VARCHAR) -> MAP(VARCHAR, VARCHAR), stated ONCE for the device op
// (exg_gffattr.hip: exg_gff_attributes), the host scalar (exon_table_function.hpp, which the DuckDB shim registers) and the
// exception's text.  Plain C++: no HIP, no DuckDB; usable from host and device code.
//
// Reference: exon/src/exon/gff_functions/module.cpp:29-84 over DuckDB v0.8.1's StringUtil::Split(string, string) and
// StringUtil::Trim; test_gff_scan.test:79-99 pins four statements.  INTEGRATION.md, "GFF attributes", carries the same rules
// with what each one rests on.
//   R1 segments  the field is cut at every `;`; segments of zero bytes are dropped; if none is left (the empty string, or `;`
//                bytes only) the whole field is the one segment
//   R2 trim      a segment loses its leading and trailing bytes out of ' ' \t \n \v \f \r (bytes >= 0x80 are never blank:
//                DuckDB's Trim tests `ch > 0 && isspace(ch)` on a signed char, which lets them stand as well)
//   R3 pieces    the trimmed segment is cut at every `=`, pieces of zero bytes are dropped; exactly two must remain: key and
//                value.  Neither is trimmed on its own: `a = b` is ("a ", " b")
//   R4 entries   in field order; a repeated key is a second entry
//   R5 zero-copy keys and values are slices of the input; nothing is decoded
//   R6 errors    the leftmost failing segment of a row: error_offset = the offset in the field of the trimmed segment's first
//                byte (of the segment's first byte when nothing is left of it), error_length = the trimmed segment's length
//   R7 NULL      a NULL row gives a NULL row (the callers' business: nothing here sees a NULL)
//
// Two statements of the same rules live here, and tests/gffattr_host_driver.cpp holds one against the other:
//   parse_field  a left-to-right parser, segment by segment — the host scalar
//   walk_words   the field 64 bytes at a time as bit masks (`;`, `=`, blanks) with a few scalars carried from word to word —
//                what a wavefront of the device op does with lane = byte; on the host the masks come from a loop
#pragma once
#include <stdint.h>

#include "exon_gpu.h"

#if defined(__HIPCC__)
#define EXG_GFF_HD __host__ __device__ inline
#else
#define EXG_GFF_HD inline
#endif

namespace exg {
namespace gffattr {

// module.cpp:61: "Invalid attribute: '" + attribute + "' expected 'key=value;key2=value2'"
static constexpr const char *kInvalidHead = "Invalid attribute: '";
static constexpr const char *kInvalidTail = "' expected 'key=value;key2=value2'";

static constexpr uint32_t kNone = 0xFFFFFFFFu;

EXG_GFF_HD constexpr bool is_blank(uint32_t c) { return c == ' ' || c - 9u <= 4u; }  // ' ', \t \n \v \f \r

// what a segment turned out to be.  kEntry: a, b = the key's start and length, c, d = the value's.  kError: a, b = R6's offset
// and length
enum : uint32_t { kNothing = 0, kEntry = 1, kError = 2 };
struct Verdict {
    uint32_t kind, a, b, c, d;
};

// ---- left to right ---------------------------------------------------------------------------------------------------
// the segment s[b, e), e > b (no `;` inside, unless it is the whole field of R1's last clause)
EXG_GFF_HD Verdict judge_segment(const uint8_t *s, uint32_t b, uint32_t e) {
    uint32_t f = b, l = e;
    while (f < l && is_blank(s[f])) f++;
    while (l > f && is_blank(s[l - 1])) l--;
    uint32_t n = 0, start[2] = {0, 0}, len[2] = {0, 0};
    for (uint32_t i = f; i < l;) {
        if (s[i] == '=') {
            i++;
            continue;
        }
        const uint32_t p = i;
        while (i < l && s[i] != '=') i++;
        if (n < 2) start[n] = p, len[n] = i - p;
        n++;
    }
    if (n != 2) return Verdict{kError, f < l ? f : b, l - f, 0, 0};
    return Verdict{kEntry, start[0], len[0], start[1], len[1]};
}

// The entries of s[0, n) in order through emit(key_start, key_len, value_start, value_len).  Returns kEntry's verdict with a =
// the number of entries, or the error's.
template <class Emit>
EXG_GFF_HD Verdict parse_field(const uint8_t *s, uint32_t n, Emit &&emit) {
    uint32_t entries = 0;
    for (uint32_t b = 0; b < n;) {
        uint32_t e = b;
        while (e < n && s[e] != ';') e++;
        if (e > b) {
            const Verdict v = judge_segment(s, b, e);
            if (v.kind == kError) return v;
            emit(v.a, v.b, v.c, v.d);
            entries++;
        }
        b = e + 1;
    }
    if (!entries) return Verdict{kError, 0, n, 0, 0};  // no segment: the field is the segment, and it holds no `=`
    return Verdict{kEntry, entries, 0, 0, 0};
}

// ---- 64 bytes at a time ------------------------------------------------------------------------------------------------
EXG_GFF_HD uint32_t lo_bit(uint64_t m) { return (uint32_t)__builtin_ctzll(m); }
EXG_GFF_HD uint32_t hi_bit(uint64_t m) { return 63u - (uint32_t)__builtin_clzll(m); }
EXG_GFF_HD uint32_t bits_of(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }
EXG_GFF_HD uint64_t below(uint32_t b) { return (1ull << b) - 1ull; }     // bits < b, b < 64
EXG_GFF_HD uint64_t above(uint32_t b) { return ~((2ull << b) - 1ull); }  // bits > b, b < 64

// One word of the field: bit i = byte base + i.
//   sc   the `;` and the virtual one at the field's end
//   eq   the `=`
//   nb   the bytes that are neither `;` nor blank (`=` among them): what a trim stops at
//   ps   piece starts: a byte that is neither `;` nor `=` nor one of its segment's leading blanks, behind a `=`, a `;`, a
//        leading blank or the field's start.  (A piece that starts at a blank behind the segment's last `=` lies outside the
//        trimmed range when only blanks follow: close() takes it off again.)
//   tail the word's last byte belongs to a piece
struct Word {
    uint64_t sc, eq, nb, ps;
    bool tail;
};
// real: the bytes in front of the field's end; semi, eq, blank: bytes of those classes (within real); at_end: the position of
// the field's end, if it lies in this word.  fresh_open: the segment open at the word's start has shown no byte other than
// blanks; piece_open: the previous word's tail
EXG_GFF_HD Word make_word(uint64_t real, uint64_t semi, uint64_t eq, uint64_t blank, uint64_t at_end, bool fresh_open, bool piece_open) {
    Word w;
    w.sc = semi | at_end;
    w.eq = eq;
    w.nb = real & ~semi & ~blank;
    // a segment's leading blanks: the run of blanks that begins right behind a `;` (or at the word's start, in a fresh segment).
    // The run's lowest bit is the seed; the addition carries it through the run
    const uint64_t seeds = ((semi << 1) | (fresh_open ? 1ull : 0ull)) & blank;
    const uint64_t lead = ((blank + seeds) ^ blank) & blank;
    const uint64_t content = real & ~semi & ~eq & ~lead;
    w.ps = content & ~((content << 1) | (piece_open ? 1ull : 0ull));
    w.tail = (content >> 63) & 1ull;
    return w;
}

// a segment so far: its first byte, its first and last byte that is not blank (kNone: none yet), whether that last one is a
// `=`, the pieces begun, the first piece's start and the `=` that ends it, the second's start and the `=` that ends it (kNone:
// none yet)
struct Segment {
    uint32_t start, first, last, last_is_eq, pieces, k0, k1, v0, v1;
};
EXG_GFF_HD Segment fresh(uint32_t start) { return Segment{start, kNone, kNone, 0u, 0u, kNone, kNone, kNone, kNone}; }

// the bytes `mask` of word w at base join segment g
EXG_GFF_HD void absorb(Segment &g, uint32_t base, uint64_t mask, const Word &w) {
    const uint64_t n = w.nb & mask, p = w.ps & mask, q = w.eq & mask;
    if (n) {
        if (g.first == kNone) g.first = base + lo_bit(n);
        g.last = base + hi_bit(n);
        g.last_is_eq = (uint32_t)((w.eq >> hi_bit(n)) & 1ull);
    }
    const uint32_t old = g.pieces;
    g.pieces = old + bits_of(p);
    uint64_t kq = q, vq = q;  // the `=` behind the key's start / the value's
    if (old == 0 && p) {
        g.k0 = base + lo_bit(p);
        kq = q & above(lo_bit(p));
    }
    if (old < 2 && g.pieces >= 2) {
        const uint64_t p2 = old == 1 ? p : p & (p - 1ull);
        g.v0 = base + lo_bit(p2);
        vq = q & above(lo_bit(p2));
    }
    if (g.pieces >= 1 && g.k1 == kNone && kq) g.k1 = base + lo_bit(kq);
    if (g.pieces >= 2 && g.v1 == kNone && vq) g.v1 = base + lo_bit(vq);
}

// segment g ends at the `;` at pos
EXG_GFF_HD Verdict close(const Segment &g, uint32_t pos) {
    if (g.start == pos) return Verdict{kNothing, 0, 0, 0, 0};
    if (g.first == kNone) return Verdict{kError, g.start, 0, 0, 0};
    // blanks behind a closing `=` began a piece that the trim cuts off
    const uint32_t cut = (g.last_is_eq && g.last + 1 < pos) ? 1u : 0u;
    if (g.pieces - cut != 2) return Verdict{kError, g.first, g.last - g.first + 1, 0, 0};
    return Verdict{kEntry, g.k0, g.k1 - g.k0, g.v0, (g.v1 != kNone ? g.v1 : g.last + 1) - g.v0};
}

// the segment that ends at bit e of word w (a bit of w.sc); `open` is the segment open at the word's start
EXG_GFF_HD Verdict judge(const Segment &open, uint32_t base, uint32_t e, const Word &w) {
    const uint64_t m = w.sc & below(e);
    Segment g = m ? fresh(base + hi_bit(m) + 1u) : open;
    absorb(g, base, m ? below(e) & above(hi_bit(m)) : below(e), w);
    return close(g, base + e);
}

// the segment open behind word w
EXG_GFF_HD void advance(Segment &open, uint32_t base, const Word &w) {
    uint64_t mask = ~0ull;
    if (w.sc) {
        open = fresh(base + hi_bit(w.sc) + 1u);
        mask = above(hi_bit(w.sc));
    }
    absorb(open, base, mask, w);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// parse_field's contract by the word walk, the masks built by a loop: what the host driver holds against parse_field
template <class Emit>
inline Verdict walk_words(const uint8_t *s, uint32_t n, Emit &&emit) {
    Segment open = fresh(0);
    bool piece_open = false;
    uint32_t entries = 0;
    for (uint64_t base = 0; base <= n; base += 64) {
        uint64_t real = 0, semi = 0, eq = 0, blank = 0, at_end = 0;
        for (uint32_t i = 0; i < 64; i++) {
            const uint64_t pos = base + i, bit = 1ull << i;
            if (pos == n) at_end |= bit;
            if (pos >= n) continue;
            real |= bit;
            if (s[pos] == ';') semi |= bit;
            if (s[pos] == '=') eq |= bit;
            if (is_blank(s[pos])) blank |= bit;
        }
        const Word w = make_word(real, semi, eq, blank, at_end, open.first == kNone, piece_open);
        for (uint64_t m = w.sc; m; m &= m - 1ull) {
            const Verdict v = judge(open, (uint32_t)base, lo_bit(m), w);
            if (v.kind == kError) return v;
            if (v.kind == kEntry) emit(v.a, v.b, v.c, v.d), entries++;
        }
        if (n - base < 64) break;
        advance(open, (uint32_t)base, w);
        piece_open = w.tail;
    }
    if (!entries) return Verdict{kError, 0, n, 0, 0};
    return Verdict{kEntry, entries, 0, 0, 0};
}
#endif

}  // namespace gffattr
}  // namespace exg
