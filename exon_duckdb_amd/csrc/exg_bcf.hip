// exg_bcf.hip — BCF 2.2 records -> the VCF data lines they stand for (VCF 4.3 spec §6.3), on decoded bytes resident in HBM.
// The lines go through the VCF path as they are (exg_rd_bcf.cpp): this file is the one stage a BCF file needs of its own.
//
//   (exg_chain.hpp)  the records: record k + 1 begins at start_k + 8 + l_shared_k + l_indiv_k.  BCF's test for a plausible
//                    record: l_shared >= 24, CHROM inside the contig dictionary, POS >= -1, n_allele >= 1, n_sample the
//                    header's, a typed-string descriptor where the ID stands, and the successor passing the same test.
//   k_count          one wavefront per record: validation and the exact length of its line; for a record in error one lane
//                    walks it again left to right to say which error (first_error).
//   (prefix sum of the lengths -> the lines' offsets in the output)
//   k_finish         one thread: how many records fit the output capacity (a binary search in the offsets), the first
//                    error, where the caller goes on.
//   k_emit           one wavefront per record: the same walk again, writing.
//
// How a record is spread over the lanes — the same in both passes (render<EMIT>), so that a line is exactly as long as it was
// counted: the fixed fields are one lane's; strings (CHROM, ID, long alleles, long character values) are copied by all lanes;
// alleles, FILTER indices, INFO entries and FORMAT keys are taken 64 at a time, a lane each — a serial walk finds where each of
// the 64 begins (a typed value says how long it is, nothing says where the next but one begins), every lane measures its own,
// a wave prefix sum places them, every lane writes its own; an entry whose value has 15 elements or more (the descriptor's
// long form: a 300-element vector, a 70 000-byte string) is measured and written by all lanes instead, elements 64 at a time;
// samples are taken 64 at a time, a lane each, over all FORMAT fields (a 2 504-sample record is 40 rounds of a full wave).
// Lengths are 64-bit while counting — a line above 2 GiB is a record error, so 32 bits hold every offset while writing.
#include "exg_bcf.hpp"

#include "exg_bcf_float.hpp"
#include "exg_chain.hpp"
#include "exg_common.hpp"
#include "exg_scan.hpp"

namespace exg {
namespace bcf {

using chain::ld32;

struct Ws : chain::Tiles {
    uint64_t *ctl, *rec_off, *rec_len, *text_off, *scan_tmp;  // ctl: 0 the first error, 1 records found, 2 the chain's end, 3 tiles rewalked
    uint64_t cap, total;
};
static Ws layout(uint8_t *base, uint64_t n) {
    Ws w;
    w.tiles = chain::tiles_of(n);
    w.cap = n / kMinRecordBytes + 2;
    uint64_t off = 0;
    auto take = [&](uint64_t bytes) {
        uint8_t *p = base + off;
        off += (bytes + 255) & ~255ull;
        return p;
    };
    w.spec_entry = (uint64_t *)take(w.tiles * 8);
    w.spec_exit = (uint64_t *)take(w.tiles * 8);
    w.true_entry = (uint64_t *)take(w.tiles * 8);
    w.row_base = (uint64_t *)take(w.tiles * 8);
    w.spec_cnt = (uint32_t *)take(w.tiles * 4);
    w.spec_stop = (uint32_t *)take(w.tiles * 4);
    w.cnt = (uint32_t *)take(w.tiles * 4);
    w.ctl = (uint64_t *)take(64);
    w.rec_off = (uint64_t *)take(w.cap * 8);
    w.rec_len = (uint64_t *)take(w.cap * 8);
    w.text_off = (uint64_t *)take((w.cap + 1) * 8);
    w.scan_tmp = (uint64_t *)take(xscan_tmp_entries(w.cap) * 8);
    w.total = off;
    return w;
}
uint64_t workspace_bytes(uint64_t n_bytes) { return layout(nullptr, n_bytes).total; }

struct Dict {
    const uint8_t *bytes;
    const uint32_t *tab;  // {offset, length} pairs
    uint32_t n;
    __device__ __forceinline__ bool has(int64_t i) const { return i >= 0 && i < (int64_t)n && tab[2 * i + 1] != kNoEntry; }
    __device__ __forceinline__ uint32_t len(uint32_t i) const { return tab[2 * i + 1]; }
    __device__ __forceinline__ const uint8_t *str(uint32_t i) const { return bytes + tab[2 * i]; }
};
struct Ctx {
    Dict contig, str;
    uint32_t n_sample, gt;
};

// ---- the chain (exg_chain.hpp) -----------------------------------------------------------------------------------------------
struct BcfChain {
    int32_t n_contig;
    uint32_t n_sample;
    // 0: a complete record at s, 1: the tail, 2: l_shared < 24
    __device__ __forceinline__ int step(const uint8_t *in, uint64_t n, uint64_t s, uint64_t *next) const {
        if (s + 8 > n) return 1;
        const uint32_t ls = ld32(in + s), li = ld32(in + s + 4);
        if (ls < 24) return 2;
        const uint64_t end = s + 8 + (uint64_t)ls + (uint64_t)li;
        if (end > n) return 1;
        *next = end;
        return 0;
    }
    __device__ __forceinline__ uint64_t next(const uint8_t *in, uint64_t s) const { return s + 8 + (uint64_t)ld32(in + s) + (uint64_t)ld32(in + s + 4); }
    // s + 33 <= n.  whole: the record must end inside the buffer (a successor may be the tail)
    __device__ bool fields(const uint8_t *in, uint64_t n, uint64_t s, bool whole, uint64_t *end) const {
        const uint8_t *p = in + s;
        const uint32_t ls = ld32(p);
        if (ls < 24) return false;
        const int32_t chrom = (int32_t)ld32(p + 8), pos = (int32_t)ld32(p + 12);
        if (chrom < 0 || chrom >= n_contig || pos < -1) return false;
        if ((ld32(p + 24) >> 16) < 1 || (ld32(p + 28) & 0xFFFFFFu) != n_sample) return false;
        if ((p[32] & 15) != 7) return false;
        *end = s + 8 + (uint64_t)ls + (uint64_t)ld32(p + 4);
        return !(whole && *end > n);
    }
    __device__ bool plausible(const uint8_t *in, uint64_t n, uint64_t s) const {
        if (s + 33 > n) return false;
        uint64_t end = 0, end2 = 0;
        if (!fields(in, n, s, true, &end)) return false;
        if (end + 33 > n) return true;  // the end of the buffer, or a tail too short to judge
        return fields(in, n, end, false, &end2);
    }
};

// a tail at the end of the stream is a record that runs past it; an l_shared below 24 ends the chain where it stands
struct BcfStitched {
    uint32_t flags;
    uint64_t *ctl;
    exg_bcf_to_vcf_result *res;
    __device__ void operator()(uint64_t rows, uint64_t cur, uint64_t rewalked, uint32_t stopped) const {
        uint64_t err = kNoError;
        if (stopped == 2) err = (rows << 8) | EXG_PE_BCF_RECORD_LENGTH;
        else if (stopped == 1 && (flags & EXG_F_EOF)) err = (rows << 8) | EXG_PE_BCF_TRUNCATED;
        ctl[0] = err, ctl[1] = rows, ctl[2] = cur, ctl[3] = rewalked;
        res->n_records = rows;  // (records found: what the host sizes the next launches by; k_finish writes the block)
    }
};

// ---- typed values ---------------------------------------------------------------------------------------------------------------
template <bool EMIT>
struct LenT {
    typedef uint64_t T;
};
template <>
struct LenT<true> {
    typedef uint32_t T;
};

template <class T>
__device__ __forceinline__ T wave_incl(T v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d, 64);
        if ((int)lane_id() >= d) v += o;
    }
    return v;
}
template <class T>
__device__ __forceinline__ T wave_last(T v) { return __shfl(v, 63, 64); }

__device__ __forceinline__ uint32_t esize(uint32_t t) { return t == 1 || t == 7 ? 1u : t == 2 ? 2u : t == 3 || t == 5 ? 4u : 0u; }
__device__ __forceinline__ bool type_ok(uint32_t t) { return t <= 3 || t == 5 || t == 7; }
__device__ __forceinline__ int32_t ld_int(const uint8_t *q, uint32_t t) {
    return t == 1 ? (int32_t)(int8_t)q[0] : t == 2 ? (int32_t)(int16_t)((uint32_t)q[0] | ((uint32_t)q[1] << 8)) : (int32_t)ld32(q);
}
// 0 a number, 1 missing, 2 end-of-vector, 3 reserved
__device__ __forceinline__ uint32_t int_kind(int32_t v, uint32_t t) {
    const int64_t lo = t == 1 ? -128 : t == 2 ? -32768 : -2147483648ll, d = (int64_t)v - lo;
    return d == 0 ? 1u : d == 1 ? 2u : d < 8 ? 3u : 0u;
}
__device__ __noinline__ Txt f32_text(uint32_t bits) { return render_f32(bits); }
__device__ __noinline__ Txt i64_text(int64_t v) { return render_i64(v); }
__device__ __forceinline__ void put_txt(uint8_t *dst, const Txt &t) {
    for (uint32_t i = 0; i < t.n; i++) dst[i] = (uint8_t)t.at(i);
}
// one element of a numeric vector: its kind, and for a number its text
__device__ __forceinline__ uint32_t elem(const uint8_t *q, uint32_t type, Txt *t) {
    if (type == 5) {
        const uint32_t bits = ld32(q);
        if (bits == 0x7F800001u) return 1;
        if (bits == 0x7F800002u) return 2;
        *t = f32_text(bits);
        return 0;
    }
    const int32_t v = ld_int(q, type);
    const uint32_t k = int_kind(v, type);
    if (!k) *t = i64_text(v);
    return k;
}

// a typed integer scalar (a key, a long form's length) at o; 0 or the error
__device__ __forceinline__ uint32_t rd_typed_int(const uint8_t *p, uint64_t &o, uint64_t lim, int32_t *v) {
    if (o + 1 > lim) return EXG_PE_BCF_OVERRUN;
    const uint32_t b = p[o], t = b & 15;
    if ((b >> 4) != 1 || t < 1 || t > 3) return EXG_PE_BCF_TYPE;
    const uint32_t sz = esize(t);
    if (o + 1 + sz > lim) return EXG_PE_BCF_OVERRUN;
    *v = ld_int(p + o + 1, t);
    o += 1 + sz;
    return 0;
}
__device__ __forceinline__ uint32_t rd_desc(const uint8_t *p, uint64_t &o, uint64_t lim, uint32_t *type, uint32_t *cnt) {
    if (o + 1 > lim) return EXG_PE_BCF_OVERRUN;
    const uint32_t b = p[o++];
    *type = b & 15, *cnt = b >> 4;
    if (!type_ok(*type)) return EXG_PE_BCF_TYPE;
    if (*cnt == 15) {
        int32_t v = 0;
        if (const uint32_t e = rd_typed_int(p, o, lim, &v)) return e;
        if (v < 0) return EXG_PE_BCF_TYPE;
        *cnt = (uint32_t)v;
    }
    return 0;
}
struct Val {
    uint32_t type, cnt;
    uint64_t data;
};
__device__ __forceinline__ uint32_t rd_value(const uint8_t *p, uint64_t &o, uint64_t lim, Val *v) {
    if (const uint32_t e = rd_desc(p, o, lim, &v->type, &v->cnt)) return e;
    const uint64_t bytes = (uint64_t)v->cnt * esize(v->type);
    if (o + bytes > lim) return EXG_PE_BCF_OVERRUN;
    v->data = o;
    o += bytes;
    return 0;
}

// a vector by ONE lane: its elements up to the first end-of-vector joined by ',', a missing one '.', none at all '.';
// characters: the bytes up to the first NUL, none '.'.  The length; with EMIT the text goes to dst
template <bool EMIT>
__device__ typename LenT<EMIT>::T lane_vec(const uint8_t *q, uint32_t type, uint32_t cnt, uint8_t *dst, uint32_t &err) {
    typedef typename LenT<EMIT>::T L;
    if (type == 7) {
        uint32_t n = 0;
        while (n < cnt && q[n]) n++;
        if (!n) {
            if (EMIT) dst[0] = '.';
            return 1;
        }
        if (EMIT)
            for (uint32_t i = 0; i < n; i++) dst[i] = q[i];
        return (L)n;
    }
    const uint32_t sz = esize(type);
    L len = 0;
    uint32_t k = 0;
    for (uint32_t i = 0; sz && i < cnt; i++) {
        Txt t;
        const uint32_t kind = elem(q + (uint64_t)i * sz, type, &t);
        if (kind == 2) break;
        if (kind == 3) {
            err = EXG_PE_BCF_RESERVED_VALUE;
            break;
        }
        if (k) {
            if (EMIT) dst[len] = ',';
            len++;
        }
        if (kind == 1) {
            if (EMIT) dst[len] = '.';
            len++;
        } else {
            if (EMIT) put_txt(dst + len, t);
            len += t.n;
        }
        k++;
    }
    if (!k) {
        if (EMIT) dst[len] = '.';
        len++;
    }
    return len;
}

// a genotype by one lane: v -> allele (v >> 1) - 1, '.' when v >> 1 == 0 or v is the missing value; from the second on '|' in
// front when v & 1, else '/'; end-of-vector ends it; none '.'
template <bool EMIT>
__device__ typename LenT<EMIT>::T lane_gt(const uint8_t *q, uint32_t type, uint32_t cnt, uint8_t *dst, uint32_t &err) {
    typedef typename LenT<EMIT>::T L;
    const uint32_t sz = esize(type);
    L len = 0;
    uint32_t k = 0;
    for (uint32_t i = 0; i < cnt; i++) {
        const int32_t v = ld_int(q + (uint64_t)i * sz, type);
        const uint32_t kind = int_kind(v, type);
        if (kind == 2) break;
        if (kind == 3 || (kind == 0 && v < 0)) {
            err = EXG_PE_BCF_RESERVED_VALUE;
            break;
        }
        const bool dot = kind == 1 || (v >> 1) == 0;
        if (k) {
            if (EMIT) dst[len] = kind == 0 && (v & 1) ? '|' : '/';
            len++;
        }
        if (dot) {
            if (EMIT) dst[len] = '.';
            len++;
        } else {
            const Txt t = i64_text((v >> 1) - 1);
            if (EMIT) put_txt(dst + len, t);
            len += t.n;
        }
        k++;
    }
    if (!k) {
        if (EMIT) dst[len] = '.';
        len++;
    }
    return len;
}

// a vector by ALL lanes (the same rules): elements 64 at a time.  The same answer in every lane
template <bool EMIT>
__device__ typename LenT<EMIT>::T wave_vec(const uint8_t *q, uint32_t type, uint32_t cnt, uint8_t *dst, uint32_t lane, uint32_t &err) {
    typedef typename LenT<EMIT>::T L;
    if (type == 7) {
        uint32_t n = cnt;
        for (uint32_t base = 0; base < cnt; base += 64) {
            const uint32_t i = base + lane;
            const unsigned long long m = __ballot(i < cnt && q[i] == 0);
            if (m) {
                n = base + (uint32_t)__builtin_ctzll(m);
                break;
            }
        }
        if (!n) {
            if (EMIT && !lane) dst[0] = '.';
            return 1;
        }
        if (EMIT)
            for (uint32_t i = lane; i < n; i += 64) dst[i] = q[i];
        return (L)n;
    }
    const uint32_t sz = esize(type);
    L total = 0;
    uint64_t nelem = 0;
    for (uint32_t base = 0; sz && base < cnt; base += 64) {
        const uint32_t i = base + lane;
        const bool in = i < cnt;
        Txt t;
        const uint32_t kind = in ? elem(q + (uint64_t)i * sz, type, &t) : 0;
        const unsigned long long m = __ballot(in && kind == 2);
        const uint32_t first = m ? (uint32_t)__builtin_ctzll(m) : 64;
        const bool active = in && lane < first;
        if (active && kind == 3) err = EXG_PE_BCF_RESERVED_VALUE;
        const L l = active ? (L)((kind == 0 ? t.n : 1u) + (i ? 1u : 0u)) : (L)0;
        const L incl = wave_incl<L>(l);
        if (EMIT && active) {
            uint8_t *d = dst + total + incl - l;
            if (i) *d++ = ',';
            if (kind == 0) put_txt(d, t);
            else *d = '.';
        }
        total += wave_last<L>(incl);
        nelem += (uint64_t)__popcll(__ballot(active));
        if (m) break;
    }
    if (!nelem) {
        if (EMIT && !lane) dst[total] = '.';
        total += 1;
    }
    return total;
}

// ---- a record ---------------------------------------------------------------------------------------------------------------------
// up to 64 entries, a lane each: [pre] [key [=]] [value].  key ~0: none (an allele); a key with a value of type 0 is a flag
struct Ent {
    uint32_t pre, key, type, cnt;
    uint64_t data;
};
template <bool EMIT>
__device__ void put_entries(const Ctx &c, const uint8_t *p, uint8_t *out, typename LenT<EMIT>::T &off, const Ent &e, bool have, uint32_t lane, uint32_t &lerr) {
    typedef typename LenT<EMIT>::T L;
    const bool keyed = e.key != ~0u;
    const bool hasval = have && !(keyed && e.type == 0);
    const bool large = hasval && e.cnt >= 15;
    const uint32_t kl = have && keyed ? c.str.len(e.key) : 0;
    const L head = have ? (L)((e.pre ? 1u : 0u) + kl + (keyed && hasval ? 1u : 0u)) : (L)0;
    L body = 0;
    if (hasval && !large) body = (L)lane_vec<false>(p + e.data, e.type, e.cnt, nullptr, lerr);
    const unsigned long long lm = __ballot(large);
    for (unsigned long long m = lm; m; m &= m - 1) {
        const int j = __builtin_ctzll(m);
        const uint32_t type = __shfl(e.type, j, 64), cnt = __shfl(e.cnt, j, 64);
        const uint64_t data = __shfl((unsigned long long)e.data, j, 64);
        const L l = (L)wave_vec<false>(p + data, type, cnt, nullptr, lane, lerr);
        if ((int)lane == j) body = l;
    }
    const L l = head + body, incl = wave_incl<L>(l), my = off + incl - l;
    if (EMIT) {
        if (have) {
            uint8_t *d = out + my;
            if (e.pre) *d++ = (uint8_t)e.pre;
            if (keyed) {
                const uint8_t *ks = c.str.str(e.key);
                for (uint32_t i = 0; i < kl; i++) d[i] = ks[i];
                d += kl;
                if (hasval) *d++ = '=';
            }
            if (hasval && !large) lane_vec<true>(p + e.data, e.type, e.cnt, d, lerr);
        }
        for (unsigned long long m = lm; m; m &= m - 1) {
            const int j = __builtin_ctzll(m);
            const uint32_t type = __shfl(e.type, j, 64), cnt = __shfl(e.cnt, j, 64);
            const uint64_t data = __shfl((unsigned long long)e.data, j, 64);
            const L at = __shfl(my + head, j, 64);
            wave_vec<true>(p + data, type, cnt, out + at, lane, lerr);
        }
    }
    off += wave_last<L>(incl);
}

// one sample by one lane: '\t', then its value of every FORMAT field joined by ':' (the fields were validated by the caller)
template <bool EMIT>
__device__ typename LenT<EMIT>::T put_sample(const Ctx &c, const uint8_t *p, uint64_t lim_s, uint64_t lim_i, uint32_t n_fmt, uint32_t n_sample, uint32_t s,
                                            bool have, uint8_t *dst, uint32_t &lerr) {
    typedef typename LenT<EMIT>::T L;
    uint64_t o = lim_s;
    L len = 0;
    if (have) {
        if (EMIT) dst[0] = '\t';
        len = 1;
    }
    for (uint32_t f = 0; f < n_fmt; f++) {
        int32_t key = 0;
        uint32_t type = 0, cnt = 0;
        if (rd_typed_int(p, o, lim_i, &key) || rd_desc(p, o, lim_i, &type, &cnt)) break;
        const uint32_t sz = esize(type);
        const uint64_t bytes = (uint64_t)n_sample * cnt * sz;
        if (o + bytes > lim_i) break;
        if (have) {
            if (f) {
                if (EMIT) dst[len] = ':';
                len++;
            }
            const uint8_t *q = p + o + (uint64_t)s * cnt * sz;
            len += (uint32_t)key == c.gt && type >= 1 && type <= 3 ? lane_gt<EMIT>(q, type, cnt, dst + len, lerr) : lane_vec<EMIT>(q, type, cnt, dst + len, lerr);
        }
        o += bytes;
    }
    return len;
}

__device__ __forceinline__ uint32_t wave_first_error(uint32_t e) {  // the lowest code any lane holds (0: none)
    e = e ? e : ~0u;
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const uint32_t o = __shfl_xor(e, d, 64);
        e = o < e ? o : e;
    }
    return e == ~0u ? 0 : e;
}

// the line of the record at p (complete inside the buffer: the chain says so); its length, the same in every lane.  *code: the
// record's error (what is counted behind one is not used)
template <bool EMIT>
__device__ typename LenT<EMIT>::T render(const Ctx &c, const uint8_t *p, uint8_t *out, uint32_t lane, uint32_t *code) {
    typedef typename LenT<EMIT>::T L;
#define BCF_FAIL(e)      \
    do {                 \
        *code = (e);     \
        return (L)0;     \
    } while (0)
    uint32_t lerr = 0;
    const uint32_t ls = ld32(p), li = ld32(p + 4);
    const int32_t chrom = (int32_t)ld32(p + 8), pos = (int32_t)ld32(p + 12);
    const uint32_t qual = ld32(p + 20), nai = ld32(p + 24), nfs = ld32(p + 28);
    const uint32_t n_allele = nai >> 16, n_info = nai & 0xFFFF, n_fmt = nfs >> 24, n_sample = nfs & 0xFFFFFF;
    const uint64_t lim_s = 8 + (uint64_t)ls, lim_i = lim_s + li;
    if (!c.contig.has(chrom)) BCF_FAIL(EXG_PE_BCF_CHROM);
    if (!n_allele) BCF_FAIL(EXG_PE_BCF_NO_ALLELE);
    if (n_sample != c.n_sample) BCF_FAIL(EXG_PE_BCF_SAMPLE_COUNT);
    L off = 0;
    auto put_char = [&](uint32_t ch) {
        if (EMIT && !lane) out[off] = (uint8_t)ch;
        off += 1;
    };
    {  // CHROM, POS
        const uint32_t cl = c.contig.len((uint32_t)chrom);
        const uint8_t *cs = c.contig.str((uint32_t)chrom);
        if (EMIT)
            for (uint32_t i = lane; i < cl; i += 64) out[off + i] = cs[i];
        off += cl;
        put_char('\t');
        const Txt t = i64_text((int64_t)pos + 1);
        if (EMIT && !lane) put_txt(out + off, t);
        off += t.n;
        put_char('\t');
    }
    uint64_t o = 32;
    {  // ID
        Val v;
        if (const uint32_t e = rd_value(p, o, lim_s, &v)) BCF_FAIL(e);
        if (v.type != 7 && v.type != 0) BCF_FAIL(EXG_PE_BCF_TYPE);
        off += (L)wave_vec<EMIT>(p + v.data, v.type, v.cnt, out + off, lane, lerr);
        put_char('\t');
    }
    for (uint32_t base = 0; base < n_allele; base += 64) {  // REF \t ALT,ALT
        const uint32_t nn = n_allele - base < 64 ? n_allele - base : 64;
        Ent e = {0, ~0u, 0, 0, 0};
        for (uint32_t j = 0; j < nn; j++) {
            Val v;
            if (const uint32_t er = rd_value(p, o, lim_s, &v)) BCF_FAIL(er);
            if (v.type != 7 && v.type != 0) BCF_FAIL(EXG_PE_BCF_TYPE);
            if (lane == j) e.type = v.type, e.cnt = v.cnt, e.data = v.data;
        }
        const uint32_t idx = base + lane;
        e.pre = idx == 0 ? 0u : idx == 1 ? (uint32_t)'\t' : (uint32_t)',';
        put_entries<EMIT>(c, p, out, off, e, lane < nn, lane, lerr);
    }
    if (n_allele == 1) put_char('\t'), put_char('.');
    put_char('\t');
    {  // QUAL
        Txt t;
        const uint32_t kind = elem(p + 20, 5, &t);
        (void)qual;
        if (kind) {
            put_char('.');
        } else {
            if (EMIT && !lane) put_txt(out + off, t);
            off += t.n;
        }
        put_char('\t');
    }
    {  // FILTER
        Val v;
        if (const uint32_t e = rd_value(p, o, lim_s, &v)) BCF_FAIL(e);
        if (v.type > 3) BCF_FAIL(EXG_PE_BCF_TYPE);
        if (v.type == 0 || v.cnt == 0) {
            put_char('.');
        } else {
            const uint32_t sz = esize(v.type);
            for (uint32_t base = 0; base < v.cnt; base += 64) {
                const uint32_t i = base + lane;
                const bool in = i < v.cnt;
                const int32_t idx = in ? ld_int(p + v.data + (uint64_t)i * sz, v.type) : 0;
                const bool ok = in && c.str.has(idx);
                if (in && !ok) lerr = EXG_PE_BCF_DICT_INDEX;
                const uint32_t kl = ok ? c.str.len((uint32_t)idx) : 0;
                const L l = ok ? (L)(kl + (i ? 1u : 0u)) : (L)0, incl = wave_incl<L>(l);
                if (EMIT && ok) {
                    uint8_t *d = out + off + incl - l;
                    if (i) *d++ = ';';
                    const uint8_t *ks = c.str.str((uint32_t)idx);
                    for (uint32_t k = 0; k < kl; k++) d[k] = ks[k];
                }
                off += wave_last<L>(incl);
            }
        }
        put_char('\t');
    }
    if (!n_info) put_char('.');
    for (uint32_t base = 0; base < n_info; base += 64) {  // INFO: key[=value];...
        const uint32_t nn = n_info - base < 64 ? n_info - base : 64;
        Ent e = {0, 0, 0, 0, 0};
        for (uint32_t j = 0; j < nn; j++) {
            int32_t key = 0;
            Val v;
            if (const uint32_t er = rd_typed_int(p, o, lim_s, &key)) BCF_FAIL(er);
            if (!c.str.has(key)) BCF_FAIL(EXG_PE_BCF_DICT_INDEX);
            if (const uint32_t er = rd_value(p, o, lim_s, &v)) BCF_FAIL(er);
            if (lane == j) e.key = (uint32_t)key, e.type = v.type, e.cnt = v.cnt, e.data = v.data;
        }
        e.pre = base + lane ? (uint32_t)';' : 0u;
        put_entries<EMIT>(c, p, out, off, e, lane < nn, lane, lerr);
    }
    if (n_fmt && n_sample) {
        put_char('\t');
        o = lim_s;
        for (uint32_t base = 0; base < n_fmt; base += 64) {  // FORMAT: the keys; every field is validated here
            const uint32_t nn = n_fmt - base < 64 ? n_fmt - base : 64;
            uint32_t my_key = 0;
            for (uint32_t j = 0; j < nn; j++) {
                int32_t key = 0;
                uint32_t type = 0, cnt = 0;
                if (const uint32_t er = rd_typed_int(p, o, lim_i, &key)) BCF_FAIL(er);
                if (!c.str.has(key)) BCF_FAIL(EXG_PE_BCF_DICT_INDEX);
                if (const uint32_t er = rd_desc(p, o, lim_i, &type, &cnt)) BCF_FAIL(er);
                const uint64_t bytes = (uint64_t)n_sample * cnt * esize(type);
                if (o + bytes > lim_i) BCF_FAIL(EXG_PE_BCF_OVERRUN);
                o += bytes;
                if (lane == j) my_key = (uint32_t)key;
            }
            const bool have = lane < nn;
            const uint32_t kl = have ? c.str.len(my_key) : 0;
            const L l = have ? (L)(kl + (base + lane ? 1u : 0u)) : (L)0, incl = wave_incl<L>(l);
            if (EMIT && have) {
                uint8_t *d = out + off + incl - l;
                if (base + lane) *d++ = ':';
                const uint8_t *ks = c.str.str(my_key);
                for (uint32_t k = 0; k < kl; k++) d[k] = ks[k];
            }
            off += wave_last<L>(incl);
        }
        for (uint32_t sb = 0; sb < n_sample; sb += 64) {  // the samples, a lane each
            const uint32_t s = sb + lane;
            const bool have = s < n_sample;
            const L l = (L)put_sample<false>(c, p, lim_s, lim_i, n_fmt, n_sample, s, have, nullptr, lerr), incl = wave_incl<L>(l);
            if (EMIT) put_sample<true>(c, p, lim_s, lim_i, n_fmt, n_sample, s, have, out + off + incl - l, lerr);
            off += wave_last<L>(incl);
        }
    }
    put_char('\n');
    *code = wave_first_error(lerr);
    return off;
#undef BCF_FAIL
}

// ---- which error a record reports ------------------------------------------------------------------------------------------------
// The first one a reader meets going left to right through the record.  render<> says WHETHER a record has an
// error, in the order that suits 64 lanes: descriptors 64 at a time before any of their values, deferred lane errors by their
// code.  For a record that has one — and only then — one lane walks it again in the reader's order: the fixed fields, ID, the
// alleles, FILTER and its indices, every INFO entry (key, descriptor, then its elements), every FORMAT field's key and
// descriptor, then the samples in order and within a sample the fields in order.

// a reserved value (for a genotype also a negative one) among the integers in front of the first end-of-vector
__device__ uint32_t vec_error(const uint8_t *q, uint32_t type, uint32_t cnt, bool gt) {
    if (type < 1 || type > 3) return 0;
    const uint32_t sz = esize(type);
    for (uint32_t i = 0; i < cnt; i++) {
        const int32_t v = ld_int(q + (uint64_t)i * sz, type);
        const uint32_t kind = int_kind(v, type);
        if (kind == 2) break;
        if (kind == 3 || (gt && kind == 0 && v < 0)) return EXG_PE_BCF_RESERVED_VALUE;
    }
    return 0;
}

__device__ __noinline__ uint32_t first_error(const Ctx c, const uint8_t *p) {
    const uint32_t ls = ld32(p), li = ld32(p + 4), nai = ld32(p + 24), nfs = ld32(p + 28);
    const uint32_t n_allele = nai >> 16, n_info = nai & 0xFFFF, n_fmt = nfs >> 24, n_sample = nfs & 0xFFFFFF;
    const uint64_t lim_s = 8 + (uint64_t)ls, lim_i = lim_s + li;
    if (!c.contig.has((int32_t)ld32(p + 8))) return EXG_PE_BCF_CHROM;
    if (!n_allele) return EXG_PE_BCF_NO_ALLELE;
    if (n_sample != c.n_sample) return EXG_PE_BCF_SAMPLE_COUNT;
    uint64_t o = 32;
    Val v;
    for (uint32_t j = 0; j <= n_allele; j++) {  // ID, the alleles
        if (const uint32_t e = rd_value(p, o, lim_s, &v)) return e;
        if (v.type != 7 && v.type != 0) return EXG_PE_BCF_TYPE;
    }
    if (const uint32_t e = rd_value(p, o, lim_s, &v)) return e;  // FILTER
    if (v.type > 3) return EXG_PE_BCF_TYPE;
    for (uint32_t i = 0; v.type && i < v.cnt; i++)
        if (!c.str.has(ld_int(p + v.data + (uint64_t)i * esize(v.type), v.type))) return EXG_PE_BCF_DICT_INDEX;
    for (uint32_t j = 0; j < n_info; j++) {
        int32_t key = 0;
        if (const uint32_t e = rd_typed_int(p, o, lim_s, &key)) return e;
        if (!c.str.has(key)) return EXG_PE_BCF_DICT_INDEX;
        if (const uint32_t e = rd_value(p, o, lim_s, &v)) return e;
        if (const uint32_t e = vec_error(p + v.data, v.type, v.cnt, false)) return e;
    }
    if (!n_fmt || !n_sample) return 0;
    o = lim_s;
    for (uint32_t f = 0; f < n_fmt; f++) {
        int32_t key = 0;
        uint32_t type = 0, cnt = 0;
        if (const uint32_t e = rd_typed_int(p, o, lim_i, &key)) return e;
        if (!c.str.has(key)) return EXG_PE_BCF_DICT_INDEX;
        if (const uint32_t e = rd_desc(p, o, lim_i, &type, &cnt)) return e;
        const uint64_t bytes = (uint64_t)n_sample * cnt * esize(type);
        if (o + bytes > lim_i) return EXG_PE_BCF_OVERRUN;
        o += bytes;
    }
    for (uint32_t s = 0; s < n_sample; s++) {
        o = lim_s;
        for (uint32_t f = 0; f < n_fmt; f++) {  // (the fields were validated above)
            int32_t key = 0;
            uint32_t type = 0, cnt = 0;
            (void)rd_typed_int(p, o, lim_i, &key);
            (void)rd_desc(p, o, lim_i, &type, &cnt);
            const uint64_t one = (uint64_t)cnt * esize(type);
            if (const uint32_t e = vec_error(p + o + s * one, type, cnt, (uint32_t)key == c.gt)) return e;
            o += n_sample * one;
        }
    }
    return 0;
}

__global__ __launch_bounds__(256) void k_count(const uint8_t *__restrict__ in, uint64_t n_rows, Ctx c, Ws w) {
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t code = 0;
    const uint64_t len = render<false>(c, in + w.rec_off[r], nullptr, lane, &code);
    if (lane) return;
    if (code) {  // which of the record's errors: the leftmost
        const uint32_t first = first_error(c, in + w.rec_off[r]);
        code = first ? first : code;
    } else if (len > 0x7FFFFFFFull) {
        code = EXG_PE_FIELD_TOO_LONG;
    }
    w.rec_len[r] = code ? 0 : len;
    if (code) atomicMin((unsigned long long *)&w.ctl[0], (unsigned long long)((r << 8) | code));
}

struct LenOf {
    const uint64_t *len;
    __device__ uint64_t operator()(uint64_t i) const { return len[i]; }
};

// how many records fit, the first error, where the caller goes on
__global__ void k_finish(Ws w, exg_bcf_to_vcf_result *res, uint64_t capacity) {
    const uint64_t e = w.ctl[0], found = w.ctl[1], chain_end = w.ctl[2];
    const uint64_t ord = e == kNoError ? ~0ull : e >> 8;
    const uint64_t good = ord < found ? ord : found;  // records in front of the first error
    uint64_t lo = 0, hi = good;                       // the most records whose text fits: text_off is ascending
    while (found && lo < hi) {
        const uint64_t mid = (lo + hi + 1) / 2;
        if (w.text_off[mid] <= capacity) lo = mid;
        else hi = mid - 1;
    }
    const uint64_t k = found ? lo : 0;
    res->n_records = k;
    res->text_bytes_needed = found ? w.text_off[good] : 0;
    res->text_bytes = found ? w.text_off[k] : 0;
    res->consumed_bytes = k < found ? w.rec_off[k] : chain_end;
    res->error_record = 0, res->error_offset = ~0ull, res->error_code = 0;
    res->flags = k < good ? EXG_RF_CAPACITY : 0;
    res->tiles_rewalked = w.ctl[3];
    if (e != kNoError && k == good) {
        res->error_code = (uint32_t)(e & 0xFF);
        res->error_record = ord;
        res->error_offset = ord < found ? w.rec_off[ord] : chain_end;
        res->consumed_bytes = res->error_offset;
    }
}

__global__ __launch_bounds__(256) void k_emit(const uint8_t *__restrict__ in, Ctx c, Ws w, uint8_t *__restrict__ out, const exg_bcf_to_vcf_result *res) {
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= res->n_records) return;  // (the launch covers the records found; those that fit are written)
    uint32_t code = 0;
    (void)render<true>(c, in + w.rec_off[r], out + w.text_off[r], threadIdx.x & 63, &code);
}

int to_vcf(const exg_bcf_to_vcf_args *a, exg_bcf_to_vcf_result *out) {
    if (!a || !a->d_result || !a->d_workspace || ((uintptr_t)a->d_workspace & 255) || (a->n_bytes && !a->d_input) ||
        (a->n_contigs && (!a->d_contig_bytes || !a->d_contig_table)) || (a->n_strings && (!a->d_string_bytes || !a->d_string_table)) ||
        (a->output_capacity && !a->d_output) || a->n_contigs > 0x7FFFFFFFu || a->n_samples > 0xFFFFFFu) {
        set_error("exg_bcf_to_vcf: bad arguments (null pointer, unaligned workspace, or a dictionary without its table)");
        return EXG_E_INVALID_ARG;
    }
    if (a->flags & ~EXG_F_EOF) {
        set_error("exg_bcf_to_vcf: unknown flag bits 0x%x", a->flags & ~EXG_F_EOF);
        return EXG_E_INVALID_ARG;
    }
    if (a->workspace_bytes < workspace_bytes(a->n_bytes)) {
        set_error("exg_bcf_to_vcf: workspace too small (%llu < %llu)", (unsigned long long)a->workspace_bytes, (unsigned long long)workspace_bytes(a->n_bytes));
        return EXG_E_INVALID_ARG;
    }
    hipStream_t st = (hipStream_t)a->stream;
    const Ws w = layout((uint8_t *)a->d_workspace, a->n_bytes);
    const uint8_t *in = (const uint8_t *)a->d_input;
    Ctx c;
    c.contig = Dict{a->d_contig_bytes, a->d_contig_table, a->n_contigs};
    c.str = Dict{a->d_string_bytes, a->d_string_table, a->n_strings};
    c.n_sample = a->n_samples, c.gt = a->gt_index;
    const BcfChain f{(int32_t)a->n_contigs, a->n_samples};
    EXG_HIP_CHECK(chain::find(in, a->n_bytes, f, w, BcfStitched{a->flags, w.ctl, a->d_result}, st));
    EXG_HIP_CHECK(hipMemcpyAsync(out, a->d_result, sizeof *out, hipMemcpyDeviceToHost, st));
    EXG_HIP_CHECK(hipStreamSynchronize(st));
    const uint64_t found = out->n_records;
    if (found) {
        chain::index(in, f, w, w.rec_off, st);
        hipLaunchKernelGGL(k_count, dim3((uint32_t)((found + 3) / 4)), dim3(256), 0, st, in, found, c, w);
        launch_xscan(LenOf{w.rec_len}, found, w.text_off, w.scan_tmp, st);
    }
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(1), 0, st, w, a->d_result, a->output_capacity);
    if (found) hipLaunchKernelGGL(k_emit, dim3((uint32_t)((found + 3) / 4)), dim3(256), 0, st, in, c, w, a->d_output, a->d_result);
    EXG_HIP_CHECK(hipMemcpyAsync(out, a->d_result, sizeof *out, hipMemcpyDeviceToHost, st));
    EXG_HIP_CHECK(hipStreamSynchronize(st));
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

}  // namespace bcf
}  // namespace exg

extern "C" uint64_t exg_bcf_workspace_bytes(uint64_t n_bytes, uint32_t n_samples) {
    (void)n_samples;  // (a record is never shorter than its fixed fields, whatever the sample count)
    return exg::bcf::workspace_bytes(n_bytes);
}

extern "C" int exg_bcf_to_vcf(const exg_bcf_to_vcf_args *a) {
    exg_bcf_to_vcf_result res;
    return exg::bcf::to_vcf(a, &res);
}

extern "C" int exg_bcf_result(const exg_bcf_to_vcf_result *d_result, void *stream, exg_bcf_to_vcf_result *out) {
    using namespace exg;
    if (!d_result || !out) {
        set_error("exg_bcf_result: null pointer");
        return EXG_E_INVALID_ARG;
    }
    EXG_HIP_CHECK(hipMemcpyAsync(out, d_result, sizeof *out, hipMemcpyDeviceToHost, (hipStream_t)stream));
    EXG_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return EXG_OK;
}
