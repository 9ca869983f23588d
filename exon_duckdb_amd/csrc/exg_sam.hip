// exg_sam.hip — SAM record scan (read_sam_file_records): one row per alignment line, BAM's ten columns — name, flag,
// reference, start, end, mapping_quality, cigar, mate_reference, sequence, quality_score — every string a duckdb::string_t
// slice of the input (there is no side buffer), flag / start / end parsed to int32, `end` from a walk over the CIGAR text.
//
// Replaces the tokenising the reference gets from noodles-sam through exon 0.2.x (registered at
// exon/src/exon_extension.cpp:52; the ten columns pinned by test_sam_record_scan.test:6-17; the value rules are INTEGRATION.md's).
// The header (the leading '@' lines) is the reader's: it hands the scan the bytes behind it.
//
// The driver around the row function (SamRows::line<Src>) is exg_line_rows.hpp's: the fused any-shape scan — every line longer than
// a half is among those left to k_line_far — and the general path, its differential partner.
#include "exg_line_rows.hpp"

namespace exg {

// d_col: exg_string_t[] (0, 2, 5, 6, 7, 8, 9) / int32_t[] (1, 3, 4); RowInfo::valid bits 0 .. 4: columns 2, 3, 4, 5, 7 are not NULL
using SamRowsDev = LineRowsDev<EXG_SAM_COLUMNS>;

// ---- the format, for the driver (exg_line_rows.hpp) ----------------------------------------------------------
#ifndef EXG_SAM_HALVES_FULL
#define EXG_SAM_HALVES_FULL 2
#endif
#ifndef EXG_SAM_WAVES_FULL
#define EXG_SAM_WAVES_FULL 4
#endif
#ifndef EXG_SAM_NL_CAP
#define EXG_SAM_NL_CAP 1024
#endif
struct SamRows {
    static constexpr const char *kName = "exg_sam_scan", *kLabel = "SAM";
    static constexpr int kColumns = EXG_SAM_COLUMNS;
    static constexpr int kValidBits = 5;
    static constexpr int kKeepBit = -1;  // every line is a row
    __host__ __device__ static __forceinline__ constexpr int valid_col(int bit) { return bit == 0 ? 2 : bit == 1 ? 3 : bit == 2 ? 4 : bit == 3 ? 5 : 7; }
    static constexpr uint32_t kGeneralBytesPerLine = 64;
    static constexpr int kNlCap = EXG_SAM_NL_CAP;  // the densest valid line is 22 bytes with its LF: 744 per half
    static constexpr int kHalvesFull = EXG_SAM_HALVES_FULL, kWavesFull = EXG_SAM_WAVES_FULL;
    template <class Src>
    __device__ static RowInfo line(const Src &src, int s, int e, const SamRowsDev &a, unsigned long long out, bool store);  // the row function, below
};

static constexpr uint32_t kSamCigarLenMax = 268435455u;  // 2^28 - 1: what a BAM CIGAR operation holds

// the tabs of a line in order, 64 bytes at a time: next() = the next tab's position, `e` when the line has no more
template <class Src>
struct SamTabs {
    const Src &src;
    int base, e;  // the word `bits` came from begins at base; the line ends at e
    unsigned long long bits;
    __device__ __forceinline__ SamTabs(const Src &src_, int s, int e_) : src(src_), base(s - 64), e(e_), bits(0) {}
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

// one or more ASCII digits, nothing else, at most `max`
template <class Src>
__device__ __forceinline__ bool sam_uint(const Src &src, int s, int e, uint32_t max, uint32_t *out) {
    if (s >= e) return false;
    unsigned long long v = 0;
    for (int i = s; i < e; i++) {
        const uint32_t d = src.b(i) - '0';
        if (d > 9u) return false;
        v = v * 10u + d;
        if (v > max) return false;
    }
    *out = (uint32_t)v;
    return true;
}

// CIGAR text [s, e), not `*`: one or more of [digits, one of MIDNSHP=X], each length <= 2^28 - 1; *span = the reference bases
// M, D, N, = and X consume
template <class Src>
__device__ inline bool sam_cigar(const Src &src, int s, int e, unsigned long long *span) {
    unsigned long long sp = 0;
    int i = s;
    while (i < e) {
        const int d0 = i;
        uint32_t v = 0;
        uint32_t c = 0;
        for (; i < e; i++) {
            c = src.b(i);
            const uint32_t d = c - '0';
            if (d > 9u) break;
            if (v > kSamCigarLenMax / 10u) return false;  // (v * 10 stays below 2^32)
            v = v * 10u + d;
            if (v > kSamCigarLenMax) return false;
        }
        if (i == d0 || i >= e) return false;  // no digits, or no operation behind them
        const bool refc = c == 'M' || c == 'D' || c == 'N' || c == '=' || c == 'X';
        if (!refc && c != 'I' && c != 'S' && c != 'H' && c != 'P') return false;
        if (refc) sp += v;
        i++;
    }
    *span = sp;
    return i > s;
}

// One line [s, e) (CR already stripped), stored straight to row `out` (store == false: validate only).  Precedence of the
// errors: the field count, then the fields left to right (the caller checks UTF-8 behind them).  Every store comes behind
// the last check.
template <class Src>
__device__ __forceinline__ RowInfo SamRows::line(const Src &src, int s, int e, const SamRowsDev &a, unsigned long long out, bool store) {
    RowInfo r;
    r.code = 0;
    r.valid = 0;
    // t[k]: the tab that ends field k + 1 (QNAME .. SEQ: k = 0 .. 9); the first nine sit in the line's first word or two, SEQ's
    // end is searched
    SamTabs<Src> tabs(src, s, e);
    int t[10];
#pragma unroll
    for (int k = 0; k < 10; k++) t[k] = tabs.next();
    if (t[9] >= e) {  // fewer than ten tabs: fewer than eleven fields (an empty line among them)
        r.code = EXG_PE_SAM_FIELD_COUNT;
        return r;
    }
    uint32_t code = 0;
    uint32_t flag_v = 0, pos_v = 0, mapq_v = 0;
    unsigned long long span = 0;
    bool cigar_star = false;
    // QUAL [q0, qe): not searched — `*` apart, with SEQ of length L the byte L behind q0 is a tab or the line's end (the probe is
    // the length check too); on a miss SEQ is `*`, or the line is in error
    const int seq_s = t[8] + 1, L = t[9] - seq_s, q0 = t[9] + 1;
    int qe = q0;
    if (t[0] == s) code = EXG_PE_SAM_EMPTY_FIELD;
    else if (src.b(s) == '@') code = EXG_PE_SAM_HEADER_LINE;
    else if (t[1] == t[0] + 1) code = EXG_PE_SAM_EMPTY_FIELD;
    else if (!sam_uint(src, t[0] + 1, t[1], 65535u, &flag_v)) code = EXG_PE_SAM_FLAG;
    else if (t[2] == t[1] + 1) code = EXG_PE_SAM_EMPTY_FIELD;
    else if (t[3] == t[2] + 1) code = EXG_PE_SAM_EMPTY_FIELD;
    else if (!sam_uint(src, t[2] + 1, t[3], 0x7FFFFFFFu, &pos_v)) code = EXG_PE_SAM_POSITION;
    else if (t[4] == t[3] + 1) code = EXG_PE_SAM_EMPTY_FIELD;
    else if (!sam_uint(src, t[3] + 1, t[4], 255u, &mapq_v)) code = EXG_PE_SAM_MAPQ;
    else if (t[5] == t[4] + 1) code = EXG_PE_SAM_EMPTY_FIELD;
    else {
        cigar_star = t[5] - t[4] == 2 && src.b(t[4] + 1) == '*';
        if (!cigar_star && !sam_cigar(src, t[4] + 1, t[5], &span)) code = EXG_PE_SAM_CIGAR;
        else if (t[6] == t[5] + 1 || t[7] == t[6] + 1 || t[8] == t[7] + 1 || L == 0) code = EXG_PE_SAM_EMPTY_FIELD;
        else if (q0 >= e || src.b(q0) == '\t') code = EXG_PE_SAM_EMPTY_FIELD;
        else {
            // `*` is decided first — QUAL cannot hold a tab, so "*" in front of a tab or the line's end is unambiguous —: with
            // SEQ present the byte L behind q0 may well be an aux field's tab or the line's end
            const int room = e - q0;  // (> 0 here; the probe position q0 + L is formed only where it lies inside the line: a line may
                                      // be 0x7FFFFFF0 bytes long, and q0 + L of a line in error could pass 2^31)
            if (src.b(q0) == '*' && (room == 1 || src.b(q0 + 1) == '\t')) qe = q0 + 1;
            else if (L == room || (L < room && src.b(q0 + L) == '\t')) qe = q0 + L;
            else if (L == 1 && src.b(seq_s) == '*') qe = tabs.next();  // (SEQ absent, QUAL of any length: its end is searched)
            else code = EXG_PE_SAM_LENGTHS;
        }
    }
    if (code) {
        r.code = code;
        return r;
    }
    const bool ref_ok = !(t[2] - t[1] == 2 && src.b(t[1] + 1) == '*');
    const bool mate_eq = t[6] - t[5] == 2 && src.b(t[5] + 1) == '=';
    const bool mate_ok = mate_eq ? ref_ok : !(t[6] - t[5] == 2 && src.b(t[5] + 1) == '*');
    const bool start_ok = pos_v != 0;
    const long long end_v = (long long)pos_v + (long long)span - 1;
    const bool end_ok = start_ok && end_v >= 1 && end_v <= 0x7FFFFFFFll;
    const bool mapq_ok = mapq_v != 255u;
    r.valid = (ref_ok ? 1u : 0u) | (start_ok ? 2u : 0u) | (end_ok ? 4u : 0u) | (mapq_ok ? 8u : 0u) | (mate_ok ? 16u : 0u);
    if (store) {
        const uint4 z = make_uint4(0, 0, 0, 0);
        put_str(a.d_col[0], out, src.str(s, (uint32_t)(t[0] - s)));
        put_i32(a.d_col[1], out, (int)flag_v);
        const uint4 ref = ref_ok ? src.str(t[1] + 1, (uint32_t)(t[2] - t[1] - 1)) : z;
        put_str(a.d_col[2], out, ref);
        put_i32(a.d_col[3], out, (int)pos_v);
        put_i32(a.d_col[4], out, end_ok ? (int)end_v : 0);
        if (a.d_col[5]) {
            int ms = t[3] + 1;  // the canonical decimal text: the field's suffix behind its leading zeros
            while (ms < t[4] - 1 && src.b(ms) == '0') ms++;
            put_str(a.d_col[5], out, mapq_ok ? src.str(ms, (uint32_t)(t[4] - ms)) : z);
        }
        put_str(a.d_col[6], out, cigar_star ? z : src.str(t[4] + 1, (uint32_t)(t[5] - t[4] - 1)));
        put_str(a.d_col[7], out, mate_eq ? ref : mate_ok ? src.str(t[5] + 1, (uint32_t)(t[6] - t[5] - 1)) : z);
        if (a.d_col[8]) put_str(a.d_col[8], out, L == 1 && src.b(seq_s) == '*' ? z : src.str(seq_s, (uint32_t)L));
        if (a.d_col[9]) put_str(a.d_col[9], out, qe - q0 == 1 && src.b(q0) == '*' ? z : src.str(q0, (uint32_t)(qe - q0)));
    }
    return r;
}

}  // namespace exg

extern "C" int exg_sam_scan(const exg_sam_scan_args *a) { return exg::line_rows_scan<exg::SamRows>(a); }
