// exg_gtf.hpp — what the gene-annotation formats share: the eight leading columns of a GFF-family line (seqname, source, type,
// start, end, score, strand, frame — GTF and GFF3 agree on them) as row code for a row function of exg_line_rows.hpp, and the
// list of score literals the exact float parser decides behind the scan.  exg_gtf.hip is the GTF format on top of it; a GFF3
// format (read_gff: its own attribute grammar, percent-decoding, the ##FASTA section) can reuse gff_leading8 / gff_store8 with
// its own error codes.
#pragma once
#include "exg_line_src.hpp"
#include "exg_parse.hpp"

namespace exg {

// the tabs of a line in order, 64 bytes at a time (Src::tabs64): next() = the next tab's position, `e` when the line has no more
template <class Src>
struct LineTabs {
    const Src &src;
    int base, e;  // the word `bits` came from begins at base; the line ends at e
    unsigned long long bits;
    __device__ __forceinline__ LineTabs(const Src &src_, int s, int e_) : src(src_), base(s - 64), e(e_), bits(0) {}
    __device__ __forceinline__ int next() {
        while (!bits) {
            if ((long long)e - base <= 64) {  // no word left (base stays where it is: a line may be 0x7FFFFFF0 bytes long)
                base = e;
                return e;
            }
            base += 64;
            bits = src.tabs64(base);
            const int rem = e - base;
            if (rem < 64) bits &= (1ull << rem) - 1ull;
        }
        const int pos = base + __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        return pos;
    }
};

// score literals of more than 19 digits astride a float rounding boundary (exg_parse.hpp: status 2): noted by the row function,
// decided by the exact parser in a kernel behind the scan (exg_float_slow.hpp).  Lives at the end of the scan's workspace.
struct ScoreSlowList {
    static constexpr uint32_t kCap = 1024;
    unsigned int count;
    unsigned int pad[3];
    struct Lit {
        uint64_t off;  // of the literal in d_input
        uint32_t len;
        uint32_t row;
    } lit[kCap];
};

// offset in d_input of position i of a line source
template <class L>
__device__ __forceinline__ uint64_t src_offset(const LdsSrc<L> &src, int i, uint64_t payload_base) {
    return src.ptr_of_e0 + (uint64_t)(int64_t)i - payload_base;
}
__device__ __forceinline__ uint64_t src_offset(const GlobalSrc &src, int i, uint64_t) { return src.base + (uint64_t)(int64_t)i; }

// the error codes of a format of the family
struct GffCodes {
    uint32_t field_count, empty_field, position, score, strand, frame;
};

// what gff_leading8 found: t[k] = the tab that ends field k (k = 0 .. 7); valid bit 0 score, 1 strand, 2 frame
struct Gff8 {
    int t[8];
    long long start, end;
    float score;
    uint32_t valid;
    int slow_s, slow_len;  // slow_len != 0: the score literal [slow_s, slow_s + slow_len) is the exact parser's
};

// digits only, 1 .. 2^63 - 1
template <class Src>
__device__ __forceinline__ bool gff_position(const Src &src, int s, int e, long long *out) {
    if (s >= e || src.b(s) == '+') return false;  // (parse_pos reads usize::from_str, which takes a sign)
    return parse_pos(src, s, e, out) && *out >= 1;
}

// The eight leading fields of line [s, e): 0, or the first error left to right (the field count in front of them).  Nothing is
// stored.
template <class Src>
__device__ __forceinline__ uint32_t gff_leading8(const Src &src, int s, int e, const GffCodes &pe, Gff8 *f) {
    LineTabs<Src> tabs(src, s, e);
#pragma unroll
    for (int k = 0; k < 8; k++) f->t[k] = tabs.next();
    const int *t = f->t;
    if (t[7] >= e) return pe.field_count;  // fewer than eight tabs: fewer than nine fields (an empty line among them)
    if (t[0] == s || t[2] == t[1] + 1) return pe.empty_field;
    // (the score is parsed in front of the positions — the float parser is the row function's register peak, and start / end are
    // not live across it — and judged behind them: the errors keep their left-to-right order)
    const bool has_score = !(t[5] - t[4] == 2 && src.b(t[4] + 1) == '.');
    f->score = 0.f;
    int st = has_score ? parse_f32(src, t[4] + 1, t[5], &f->score) : 0;
    if (!gff_position(src, t[2] + 1, t[3], &f->start) || !gff_position(src, t[3] + 1, t[4], &f->end)) return pe.position;
    uint32_t valid = has_score ? 1u : 0u;
    f->slow_s = f->slow_len = 0;
    if (st == 2) {  // more than 19 digits astride a rounding boundary: the value comes from the fix-up kernel
        f->slow_s = t[4] + 1, f->slow_len = t[5] - (t[4] + 1);
        f->score = 0.f;
        st = 0;
    }
    if (st) return pe.score;
    const uint32_t sc = t[6] - t[5] == 2 ? src.b(t[5] + 1) : 0u;
    if (sc == '+' || sc == '-' || sc == '?') valid |= 2u;
    else if (sc != '.') return pe.strand;
    const uint32_t fc = t[7] - t[6] == 2 ? src.b(t[6] + 1) : 0u;
    if (fc == '0' || fc == '1' || fc == '2') valid |= 4u;
    else if (fc != '.') return pe.frame;
    f->valid = valid;
    return 0;
}

// the eight columns of row `out` (col[k] NULL: not produced).  Every store comes behind the last check of the line.
template <class Src>
__device__ __forceinline__ void gff_store8(const Src &src, int s, const Gff8 &f, void *const *col, unsigned long long out) {
    const int *t = f.t;
    const uint4 z = make_uint4(0, 0, 0, 0);
    if (col[0]) st_stream16(reinterpret_cast<uint4 *>(col[0]) + out, src.str(s, (uint32_t)(t[0] - s)));
    if (col[1]) st_stream16(reinterpret_cast<uint4 *>(col[1]) + out, src.str(t[0] + 1, (uint32_t)(t[1] - t[0] - 1)));
    if (col[2]) st_stream16(reinterpret_cast<uint4 *>(col[2]) + out, src.str(t[1] + 1, (uint32_t)(t[2] - t[1] - 1)));
    if (col[3]) __builtin_nontemporal_store(f.start, reinterpret_cast<long long *>(col[3]) + out);
    if (col[4]) __builtin_nontemporal_store(f.end, reinterpret_cast<long long *>(col[4]) + out);
    if (col[5]) __builtin_nontemporal_store(f.score, reinterpret_cast<float *>(col[5]) + out);
    if (col[6]) st_stream16(reinterpret_cast<uint4 *>(col[6]) + out, (f.valid & 2u) ? src.str(t[5] + 1, 1u) : z);
    if (col[7]) st_stream16(reinterpret_cast<uint4 *>(col[7]) + out, (f.valid & 4u) ? src.str(t[6] + 1, 1u) : z);
}

}  // namespace exg
