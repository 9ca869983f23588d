// exg_bam.hip — BAM records (SAM v1 §4.2) -> the ten columns of read_bam_file_records, on decoded bytes resident in HBM.
//
// A BAM record has no delimiter: record k + 1 begins at start_k + 4 + block_size_k, one dependent load per record.  The records
// are found by exg_chain.hpp (speculation per 32 KiB tile, a stitch from byte 0, an index of the offsets); what is BAM's own
// there is the test for a plausible record: header fields in range, a printable NUL-terminated name, the declared lengths fit
// block_size, and the successor at + 4 + block_size passes the field test too.  Then:
//
//   k_rows       one wavefront per record: validation, reference span of the CIGAR (-> end), length of its text, whether the
//                qualities are absent, the validity bits, the bytes the row needs in the side buffer.
//   (prefix sum of those -> the rows' offsets in the side buffer)
//   k_emit       one wavefront per record, lanes spread over the OUTPUT bytes (coalesced stores for 150 bp and for 5 Mb
//                reads alike): name copied, CIGAR rendered (a lane per operation, placed by a wave prefix sum of the text
//                lengths), sequence unpacked two characters per packed byte, qualities + 33; lane 0 writes the string_t /
//                INTEGER values.  Strings of at most 12 bytes are inlined and take no side bytes.
//   k_validity   the validity words of columns 2, 3, 4, 5, 7 (a ballot per 64 rows).
//
// A read name or an aux value that holds a plausible record costs a second walk, not a row.
#include "exg_bam.hpp"
#include "exg_chain.hpp"
#include "exg_common.hpp"
#include "exg_scan.hpp"

namespace exg {
namespace bam {

using chain::kNone;
using chain::ld32;

struct Ws : chain::Tiles {
    uint64_t *ctl, *rec_off, *side_off, *scan_tmp;
    uint32_t *rec_meta, *rec_side;
    int32_t *rec_end;
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
    w.rec_meta = (uint32_t *)take(w.cap * 4);
    w.rec_side = (uint32_t *)take(w.cap * 4);
    w.rec_end = (int32_t *)take(w.cap * 4);
    w.side_off = (uint64_t *)take((w.cap + 1) * 8);
    w.scan_tmp = (uint64_t *)take(xscan_tmp_entries(w.cap) * 8);
    w.total = off;
    return w;
}
uint64_t workspace_bytes(uint64_t n_bytes) { return layout(nullptr, n_bytes).total; }

struct Rec {
    uint32_t bs, l_name, mapq, n_cig, flag;
    int32_t ref, pos, l_seq, nref, npos;
};
__device__ __forceinline__ Rec ld_rec(const uint8_t *p) {
    Rec r;
    r.bs = ld32(p);
    r.ref = (int32_t)ld32(p + 4);
    r.pos = (int32_t)ld32(p + 8);
    const uint32_t a = ld32(p + 12), b = ld32(p + 16);
    r.l_name = a & 0xFF;
    r.mapq = (a >> 8) & 0xFF;
    r.n_cig = b & 0xFFFF;
    r.flag = b >> 16;
    r.l_seq = (int32_t)ld32(p + 20);
    r.nref = (int32_t)ld32(p + 24);
    r.npos = (int32_t)ld32(p + 28);
    return r;
}
__device__ __forceinline__ uint64_t fields_bytes(const Rec &r) {  // what block_size must hold at least (l_seq >= 0)
    return 32ull + r.l_name + 4ull * r.n_cig + ((uint64_t)r.l_seq + 1) / 2 + (uint64_t)r.l_seq;
}

// ---- speculation -------------------------------------------------------------------------------------------------------------
// s + 36 <= n.  whole: the record must end inside the buffer (a successor may be the tail)
__device__ bool fields_plausible(const uint8_t *in, uint64_t n, uint64_t s, int32_t n_ref, bool whole, uint64_t *end) {
    const Rec r = ld_rec(in + s);
    if (r.bs < 32) return false;
    if (r.ref < -1 || r.ref >= n_ref || r.nref < -1 || r.nref >= n_ref) return false;
    if (r.pos < -1 || r.npos < -1 || r.l_name < 1 || r.l_seq < 0) return false;
    if (fields_bytes(r) > r.bs) return false;
    *end = s + 4 + (uint64_t)r.bs;
    if (whole && *end > n) return false;
    const uint64_t name_end = s + 36 + r.l_name, lim = name_end < n ? name_end : n;
    for (uint64_t i = s + 36; i < lim; i++) {
        const uint32_t c = in[i];
        if (i + 1 == name_end ? c != 0 : (c < 0x21 || c > 0x7E)) return false;
    }
    return true;
}
__device__ bool plausible(const uint8_t *in, uint64_t n, uint64_t s, int32_t n_ref) {
    if (s + 36 > n) return false;
    uint64_t end = 0, end2 = 0;
    if (!fields_plausible(in, n, s, n_ref, true, &end)) return false;
    if (end + 36 > n) return true;  // the end of the buffer, or a tail too short to judge
    return fields_plausible(in, n, end, n_ref, false, &end2);
}

// ---- the chain (exg_chain.hpp) -----------------------------------------------------------------------------------------------
struct BamChain {
    int32_t n_ref;
    // 0: a complete record at s (*next = the one behind it), 1: the tail (no complete record at s), 2: block_size < 32
    __device__ __forceinline__ int step(const uint8_t *in, uint64_t n, uint64_t s, uint64_t *next) const {
        if (s + 4 > n) return 1;
        const uint32_t bs = ld32(in + s);
        if (bs < 32) return 2;
        if (s + 4 + (uint64_t)bs > n) return 1;
        *next = s + 4 + (uint64_t)bs;
        return 0;
    }
    __device__ __forceinline__ uint64_t next(const uint8_t *in, uint64_t s) const { return s + 4 + (uint64_t)ld32(in + s); }
    __device__ __forceinline__ bool plausible(const uint8_t *in, uint64_t n, uint64_t s) const { return bam::plausible(in, n, s, n_ref); }
};

// a tail at the end of the stream is a record that runs past it; a block_size below 32 ends the chain where it stands
struct BamStitched {
    uint32_t flags;
    uint64_t *ctl;
    uint64_t tiles;
    exg_bam_scan_result *res;
    __device__ void operator()(uint64_t rows, uint64_t cur, uint64_t rewalked, uint32_t stopped) const {
        uint64_t err = kNoError;
        if (stopped == 2) err = (rows << 8) | EXG_PE_BAM_BLOCK_SIZE;
        else if (stopped == 1 && (flags & EXG_F_EOF)) err = (rows << 8) | EXG_PE_BAM_TRUNCATED;
        ctl[0] = err;
        res->n_records = rows;
        res->consumed_bytes = cur;
        res->side_bytes = 0;
        res->error_record = 0, res->error_offset = ~0ull, res->error_code = 0, res->flags = 0;
        res->tiles = tiles, res->tiles_rewalked = rewalked;
    }
};

// ---- rows ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ndigits(uint32_t v) {
    return v < 10 ? 1 : v < 100 ? 2 : v < 1000 ? 3 : v < 10000 ? 4 : v < 100000 ? 5 : v < 1000000 ? 6 : v < 10000000 ? 7 : v < 100000000 ? 8 : 9;
}
__device__ __forceinline__ uint32_t out_of_line(uint32_t len) { return len > EXG_INLINE_LENGTH ? len : 0; }

static constexpr uint32_t kMetaAbsent = 1u << 24, kMetaValidShift = 25;  // rec_meta: bits 0..23 the CIGAR text's length

__global__ __launch_bounds__(256) void k_rows(const uint8_t *__restrict__ in, uint64_t n_rows, int32_t n_ref, uint64_t cols, Ws w) {
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint8_t *p = in + w.rec_off[r];
    const Rec rec = ld_rec(p);
    uint32_t code = 0, text = 0, absent = 0;
    uint64_t span = 0;
    if (rec.l_name == 0) {
        code = EXG_PE_BAM_READ_NAME;
    } else if (rec.l_seq < 0 || fields_bytes(rec) > rec.bs) {
        code = EXG_PE_BAM_FIELD_LENGTHS;
    } else if (p[36 + rec.l_name - 1] != 0) {
        code = EXG_PE_BAM_READ_NAME;
    } else if (rec.ref < -1 || rec.ref >= n_ref || rec.nref < -1 || rec.nref >= n_ref) {
        code = EXG_PE_BAM_REFERENCE_ID;
    } else {
        const uint8_t *cig = p + 36 + rec.l_name;
        bool bad = false;
        for (uint32_t i = lane; i < rec.n_cig; i += 64) {
            const uint32_t wd = ld32(cig + 4 * i), op = wd & 15, len = wd >> 4;
            bad |= op > 8;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += len;  // M D N = X consume the reference
            text += ndigits(len) + 1;
        }
        const uint8_t *qual = cig + 4ull * rec.n_cig + ((uint64_t)rec.l_seq + 1) / 2;
        bool all_ff = true, over = false;
        for (uint32_t i = lane; i < (uint32_t)rec.l_seq; i += 64) {
            const uint32_t q = qual[i];
            all_ff &= q == 0xFF;
            over |= q > 93;
        }
#pragma unroll
        for (int d = 32; d; d >>= 1) {
            span += __shfl_xor((unsigned long long)span, d, 64);
            text += __shfl_xor(text, d, 64);
        }
        all_ff = __all(all_ff);
        if (__any(bad)) code = EXG_PE_BAM_CIGAR_OP;
        else if (!all_ff && __any(over)) code = EXG_PE_BAM_QUALITY;
        absent = all_ff;
    }
    if (lane) return;
    if (code) {
        atomicMin((unsigned long long *)&w.ctl[0], (unsigned long long)((r << 8) | code));
        w.rec_meta[r] = 0, w.rec_side[r] = 0, w.rec_end[r] = 0;
        return;
    }
    // end = start + span - 1; NULL without a start, below 1, or outside INTEGER
    const int64_t end = (int64_t)rec.pos + 1 + (int64_t)span - 1;
    const bool end_ok = rec.pos >= 0 && end >= 1 && end <= 0x7FFFFFFFll;
    const uint32_t valid = (rec.ref >= 0 ? 1u : 0u) | (rec.pos >= 0 ? 2u : 0u) | (end_ok ? 4u : 0u) | (rec.mapq != 255 ? 8u : 0u) | (rec.nref >= 0 ? 16u : 0u);
    uint32_t side = 0;
    if (cols & 1) side += out_of_line(rec.l_name - 1);
    if (cols & 64) side += out_of_line(text);
    if (cols & 256) side += out_of_line((uint32_t)rec.l_seq);
    if ((cols & 512) && !absent) side += out_of_line((uint32_t)rec.l_seq);
    w.rec_meta[r] = text | (absent ? kMetaAbsent : 0) | (valid << kMetaValidShift);
    w.rec_side[r] = side;
    w.rec_end[r] = end_ok ? (int32_t)end : 0;
}

struct SideLen {
    const uint32_t *len;
    __device__ uint64_t operator()(uint64_t i) const { return len[i]; }
};

__global__ void k_finish(Ws w, exg_bam_scan_result *res, int with_side) {
    const uint64_t e = w.ctl[0], found = res->n_records;
    uint64_t rows = found;
    if (e != kNoError) {
        const uint64_t ord = e >> 8;
        res->error_code = (uint32_t)(e & 0xFF);
        res->error_record = ord;
        if (ord < found) {
            rows = ord;
            res->error_offset = w.rec_off[ord];
            res->consumed_bytes = w.rec_off[ord];
        } else {
            res->error_offset = res->consumed_bytes;
        }
    }
    res->n_records = rows;
    res->side_bytes = with_side && found ? w.side_off[rows] : 0;
}

// ---- columns ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 str_inline(const uint8_t *b, uint32_t len) {
    uint32_t wd[3] = {0, 0, 0};
    for (uint32_t i = 0; i < len; i++) wd[i >> 2] |= (uint32_t)b[i] << (8 * (i & 3));
    return make_uint4(len, wd[0], wd[1], wd[2]);
}
__device__ __forceinline__ uint4 str_pointer(const uint8_t *first4, uint32_t len, uint64_t ptr) {
    return make_uint4(len, (uint32_t)first4[0] | ((uint32_t)first4[1] << 8) | ((uint32_t)first4[2] << 16) | ((uint32_t)first4[3] << 24), (uint32_t)ptr,
                      (uint32_t)(ptr >> 32));
}
// <len><op> of one CIGAR operation -> dst; the characters written
__device__ __forceinline__ uint32_t render_op(uint32_t wd, uint8_t *dst) {
    uint32_t len = wd >> 4;
    const uint32_t d = ndigits(len);
    for (uint32_t i = d; i; i--) {
        dst[i - 1] = (uint8_t)('0' + len % 10);
        len /= 10;
    }
    dst[d] = (uint8_t)"MIDNSHP=X???????"[wd & 15];
    return d + 1;
}
__device__ __forceinline__ uint8_t base_of(uint32_t code) { return (uint8_t)"=ACMGRSVTWYHKDBN"[code & 15]; }

struct EmitArgs {
    const uint8_t *in;
    uint64_t n_rows, cols;
    const uint8_t *ref_names;
    const uint64_t *ref_off;
    uint64_t ref_base;
    void *col[EXG_BAM_COLUMNS];
    uint8_t *side;
    uint64_t side_base;
};

__device__ __forceinline__ uint4 ref_string(const EmitArgs &a, int32_t id) {
    if (id < 0) return make_uint4(0, 0, 0, 0);
    const uint64_t o = a.ref_off[id];
    return make_string_global(a.ref_names, o, a.ref_off[id + 1] - o, a.ref_base);
}

__global__ __launch_bounds__(256) void k_emit(EmitArgs a, Ws w) {
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.n_rows) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint8_t *p = a.in + w.rec_off[r];
    const Rec rec = ld_rec(p);
    const uint32_t meta = w.rec_meta[r], text = meta & 0xFFFFFF;
    const bool absent = meta & kMetaAbsent;
    uint64_t off = w.side_off[r];
    const uint8_t *name = p + 36, *cig = name + rec.l_name, *seq = cig + 4ull * rec.n_cig, *qual = seq + ((uint64_t)rec.l_seq + 1) / 2;
    const uint32_t l_seq = (uint32_t)rec.l_seq;
    uint8_t buf[24];

    if (a.cols & 1) {  // name: as stored, without its NUL
        const uint32_t len = rec.l_name - 1;
        if (len > EXG_INLINE_LENGTH) {
            for (uint32_t i = lane; i < len; i += 64) a.side[off + i] = name[i];
            if (!lane) ((uint4 *)a.col[0])[r] = str_pointer(name, len, a.side_base + off);
            off += len;
        } else if (!lane) {
            ((uint4 *)a.col[0])[r] = str_inline(name, len);
        }
    }
    if (!lane) {
        if (a.cols & 2) ((int32_t *)a.col[1])[r] = (int32_t)rec.flag;
        if (a.cols & 4) ((uint4 *)a.col[2])[r] = ref_string(a, rec.ref);
        if (a.cols & 8) ((int32_t *)a.col[3])[r] = rec.pos >= 0 ? rec.pos + 1 : 0;
        if (a.cols & 16) ((int32_t *)a.col[4])[r] = w.rec_end[r];
        if (a.cols & 32) {  // mapping_quality: decimal text, at most three digits; 255 = NULL
            uint4 v = make_uint4(0, 0, 0, 0);
            if (rec.mapq != 255) {
                const uint32_t d = ndigits(rec.mapq);
                uint32_t q = rec.mapq;
                for (uint32_t i = d; i; i--) buf[i - 1] = (uint8_t)('0' + q % 10), q /= 10;
                v = str_inline(buf, d);
            }
            ((uint4 *)a.col[5])[r] = v;
        }
        if (a.cols & 128) ((uint4 *)a.col[7])[r] = ref_string(a, rec.nref);
    }
    if (a.cols & 64) {  // cigar
        if (!lane) {  // the first operations, by one lane: the whole text when it is inlined, else its 4-byte prefix
            const uint32_t need = text > EXG_INLINE_LENGTH ? 4 : text;
            uint32_t k = 0;
            for (uint32_t i = 0; i < rec.n_cig && k < need; i++) k += render_op(ld32(cig + 4 * i), buf + k);
            ((uint4 *)a.col[6])[r] = text > EXG_INLINE_LENGTH ? str_pointer(buf, text, a.side_base + off) : str_inline(buf, text);
        }
        if (text > EXG_INLINE_LENGTH) {
            uint64_t base = off;
            for (uint32_t c0 = 0; c0 < rec.n_cig; c0 += 64) {
                const uint32_t i = c0 + lane;
                const uint32_t wd = i < rec.n_cig ? ld32(cig + 4 * i) : 0;
                const uint32_t l = i < rec.n_cig ? ndigits(wd >> 4) + 1 : 0;
                const uint32_t incl = wave_incl_sum(l);
                if (l) render_op(wd, a.side + base + incl - l);
                base += __shfl(incl, 63, 64);
            }
            off += text;
        }
    }
    if (a.cols & 256) {  // sequence: a packed byte is two characters
        if (l_seq > EXG_INLINE_LENGTH) {
            const uint32_t n_packed = (l_seq + 1) / 2;
            for (uint32_t j = lane; j < n_packed; j += 64) {
                const uint32_t b = seq[j];
                a.side[off + 2ull * j] = base_of(b >> 4);
                if (2 * j + 1 < l_seq) a.side[off + 2ull * j + 1] = base_of(b);
            }
            if (!lane) {
                for (uint32_t i = 0; i < 4; i++) buf[i] = base_of(i & 1 ? seq[i >> 1] : seq[i >> 1] >> 4);
                ((uint4 *)a.col[8])[r] = str_pointer(buf, l_seq, a.side_base + off);
            }
            off += l_seq;
        } else if (!lane) {
            for (uint32_t i = 0; i < l_seq; i++) buf[i] = base_of(i & 1 ? seq[i >> 1] : seq[i >> 1] >> 4);
            ((uint4 *)a.col[8])[r] = str_inline(buf, l_seq);
        }
    }
    if (a.cols & 512) {  // quality_score: + 33; absent (all 0xFF) = the empty string
        const uint32_t len = absent ? 0 : l_seq;
        if (len > EXG_INLINE_LENGTH) {
            for (uint32_t i = lane; i < len; i += 64) a.side[off + i] = (uint8_t)(qual[i] + 33);
            if (!lane) {
                for (uint32_t i = 0; i < 4; i++) buf[i] = (uint8_t)(qual[i] + 33);
                ((uint4 *)a.col[9])[r] = str_pointer(buf, len, a.side_base + off);
            }
        } else if (!lane) {
            for (uint32_t i = 0; i < len; i++) buf[i] = (uint8_t)(qual[i] + 33);
            ((uint4 *)a.col[9])[r] = str_inline(buf, len);
        }
    }
}

struct ValidityArgs {
    uint64_t *v[5];  // columns 2, 3, 4, 5, 7
};
__global__ __launch_bounds__(256) void k_validity(const uint32_t *__restrict__ meta, uint64_t n_rows, ValidityArgs va) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;  // (the grid covers whole words)
    const uint32_t bits = j < n_rows ? meta[j] >> kMetaValidShift : 0;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const unsigned long long m = __ballot((bits >> k) & 1);
        if ((threadIdx.x & 63) == 0 && j < n_rows && va.v[k]) va.v[k][j >> 6] = m;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static uint64_t selected(const exg_bam_scan_args *a) {
    const uint64_t all = (1ull << EXG_BAM_COLUMNS) - 1;
    return a->columns ? a->columns & all : all;
}

int discover(const exg_bam_scan_args *a, exg_bam_scan_result *out) {
    hipStream_t st = (hipStream_t)a->stream;
    const Ws w = layout((uint8_t *)a->d_workspace, a->n_bytes);
    const uint8_t *in = (const uint8_t *)a->d_input;
    const BamChain f{a->n_ref};
    EXG_HIP_CHECK(chain::find(in, a->n_bytes, f, w, BamStitched{a->flags, w.ctl, w.tiles, a->d_result}, st));
    EXG_HIP_CHECK(hipMemcpyAsync(out, a->d_result, sizeof *out, hipMemcpyDeviceToHost, st));
    EXG_HIP_CHECK(hipStreamSynchronize(st));
    const uint64_t found = out->n_records;
    const bool with_side = !(a->flags & EXG_F_NO_STORE);
    if (found) {
        chain::index(in, f, w, w.rec_off, st);
        hipLaunchKernelGGL(k_rows, dim3((uint32_t)((found + 3) / 4)), dim3(256), 0, st, in, found, a->n_ref, selected(a), w);
        if (with_side) launch_xscan(SideLen{w.rec_side}, found, w.side_off, w.scan_tmp, st);
    }
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(1), 0, st, w, a->d_result, with_side ? 1 : 0);
    EXG_HIP_CHECK(hipMemcpyAsync(out, a->d_result, sizeof *out, hipMemcpyDeviceToHost, st));
    EXG_HIP_CHECK(hipStreamSynchronize(st));
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

int emit(const exg_bam_scan_args *a, const exg_bam_scan_result *res) {
    if (!res->n_records) return EXG_OK;
    hipStream_t st = (hipStream_t)a->stream;
    const Ws w = layout((uint8_t *)a->d_workspace, a->n_bytes);
    EmitArgs e;
    e.in = (const uint8_t *)a->d_input;
    e.n_rows = res->n_records;
    e.cols = selected(a);
    e.ref_names = a->d_ref_names, e.ref_off = a->d_ref_offsets, e.ref_base = a->ref_names_base;
    for (int c = 0; c < EXG_BAM_COLUMNS; c++) e.col[c] = a->d_columns[c];
    e.side = a->d_side, e.side_base = a->side_base;
    hipLaunchKernelGGL(k_emit, dim3((uint32_t)((e.n_rows + 3) / 4)), dim3(256), 0, st, e, w);
    static const int vcol[5] = {2, 3, 4, 5, 7};
    ValidityArgs va;
    bool any = false;
    for (int k = 0; k < 5; k++) any |= (va.v[k] = ((e.cols >> vcol[k]) & 1) ? a->d_validity[vcol[k]] : nullptr) != nullptr;
    if (any) hipLaunchKernelGGL(k_validity, dim3((uint32_t)((e.n_rows + 255) / 256)), dim3(256), 0, st, w.rec_meta, e.n_rows, va);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

}  // namespace bam
}  // namespace exg

extern "C" int exg_bam_scan(const exg_bam_scan_args *a) {
    using namespace exg;
    if (!a || !a->d_result || !a->d_workspace || ((uintptr_t)a->d_workspace & 255) || (a->n_bytes && !a->d_input) || a->n_ref < 0 ||
        (a->n_ref && (!a->d_ref_names || !a->d_ref_offsets))) {
        set_error("exg_bam_scan: bad arguments (null pointer, unaligned workspace, or references without their table)");
        return EXG_E_INVALID_ARG;
    }
    if (a->flags & ~(EXG_F_EOF | EXG_F_NO_STORE)) {
        set_error("exg_bam_scan: unknown flag bits 0x%x", a->flags & ~(EXG_F_EOF | EXG_F_NO_STORE));
        return EXG_E_INVALID_ARG;
    }
    if (a->workspace_bytes < bam::workspace_bytes(a->n_bytes)) {
        set_error("exg_bam_scan: workspace too small (%llu < %llu)", (unsigned long long)a->workspace_bytes, (unsigned long long)bam::workspace_bytes(a->n_bytes));
        return EXG_E_INVALID_ARG;
    }
    const bool store = !(a->flags & EXG_F_NO_STORE);
    exg_bam_scan_args b = *a;
    b.columns = 0;
    for (int c = 0; c < EXG_BAM_COLUMNS; c++) {  // a column is produced when it is selected and has somewhere to go
        const bool sel = !a->columns || ((a->columns >> c) & 1);
        if (store && sel && a->d_columns[c]) b.columns |= 1ull << c;
        const bool nullable = c == 2 || c == 3 || c == 4 || c == 5 || c == 7;
        if (store && sel && a->d_columns[c] && nullable && !a->d_validity[c]) {
            set_error("exg_bam_scan: column %d is nullable and has no validity words", c);
            return EXG_E_INVALID_ARG;
        }
    }
    if (!b.columns) b.columns = 1ull << 63;  // (nothing to produce; 0 would mean all)
    exg_bam_scan_result res;
    int rc = bam::discover(&b, &res);
    if (rc) return rc;
    if (store) {
        if (res.n_records > a->capacity_records || res.side_bytes > a->side_capacity || (res.side_bytes && !a->d_side)) {
            res.flags |= EXG_RF_CAPACITY;
            EXG_HIP_CHECK(hipMemcpy(a->d_result, &res, sizeof res, hipMemcpyHostToDevice));
            return EXG_OK;
        }
        if ((rc = bam::emit(&b, &res))) return rc;
        EXG_HIP_CHECK(hipStreamSynchronize((hipStream_t)a->stream));
    }
    return EXG_OK;
}
