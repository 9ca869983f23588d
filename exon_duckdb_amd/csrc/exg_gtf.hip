// exg_gtf.hip — GTF record scan (read_gtf) and the attributes column's MAP children.
//
// exg_gtf_scan: one row per feature line, nine columns — seqname, source, type, start, end, score, strand, frame and the raw ninth
// field — the strings as duckdb::string_t slices of the input, start / end parsed to int64, score to float32 (VCF QUAL's
// parser).  Replaces the tokenising the reference gets from noodles-gtf through exon 0.2.x (test_gtf_scan.test:6-16 pins a row and
// the count; the value rules are INTEGRATION.md's).  The driver around the row function (GtfRows::line<Src>) is exg_line_rows.hpp's:
// the fused any-shape scan and the general path.  The skeleton numbers rows by lines, so a `#` line keeps its row number: its slot
// stays unwritten, its bit in d_keep stays clear (d_keep is one more validity word array of the driver's: R::kKeepBit) and the
// result flag EXG_RF_ROWS_SKIPPED tells the caller to gather through d_keep.
//
// exg_gtf_attributes: the ninth field -> list entries + key / value string_t, count -> prefix sum -> emit as exg_cigar_op does it.
// A wavefront takes a row, 64 bytes a step, lane = byte.  The quote state is what makes the grammar serial: the in-quote mask of a
// word is the prefix XOR of its `"` ballot (six shift-XORs on the 64-bit mask, the parity carried into the next word), everything
// else — token starts, their ordinal in the entry, the `;` that end entries, every error — is bit arithmetic on ballots with a
// handful of scalars carried from word to word.  Rows are not cut by bytes: an attributes field is a few hundred bytes (Ensembl:
// 150 .. 700), five to eleven steps of one wave; a field of megabytes is one wave's walk.
#include <string.h>

#include "exg_gtf.hpp"
#include "exg_line_rows.hpp"

#include "exg_float_slow.hpp"
#include "exg_scan.hpp"
#include "exg_strcol.hpp"

namespace exg {

// d_col: exg_string_t[] (0, 1, 2, 6, 7, 8) / int64_t[] (3, 4) / float[] (5); column 9 is not a column: d_col[9] is the
// ScoreSlowList, d_valid[9] the keep words.  RowInfo::valid bits 0 .. 2: columns 5, 6, 7 are not NULL; bit 3: the line is a row
static constexpr int kGtfDevColumns = EXG_GTF_COLUMNS + 1;
using GtfRowsDev = LineRowsDev<kGtfDevColumns>;

// ---- the format, for the driver (exg_line_rows.hpp) ----------------------------------------------------------
#ifndef EXG_GTF_HALVES_FULL
#define EXG_GTF_HALVES_FULL 2
#endif
#ifndef EXG_GTF_WAVES_FULL
#define EXG_GTF_WAVES_FULL 4
#endif
#ifndef EXG_GTF_NL_CAP
#define EXG_GTF_NL_CAP 1024
#endif
struct GtfRows {
    static constexpr const char *kName = "exg_gtf_scan", *kLabel = "GTF";
    static constexpr int kColumns = kGtfDevColumns;
    static constexpr int kValidBits = 4;
    static constexpr int kKeepBit = 3;
    __host__ __device__ static __forceinline__ constexpr int valid_col(int bit) { return bit == 3 ? 9 : 5 + bit; }
    static constexpr uint32_t kGeneralBytesPerLine = 64;
    static constexpr int kNlCap = EXG_GTF_NL_CAP;  // a feature line is 18 bytes and more; halves of `#` lines go in passes
    static constexpr int kHalvesFull = EXG_GTF_HALVES_FULL, kWavesFull = EXG_GTF_WAVES_FULL;
    template <class Src>
    __device__ static RowInfo line(const Src &src, int s, int e, const GtfRowsDev &a, unsigned long long out, bool store);  // the row function, below
};

// One line [s, e) (CR already stripped), stored straight to row `out` (store == false: validate only).  Precedence of the
// errors: the field count, then the fields left to right (the caller checks UTF-8 behind them).  Every store comes behind
// the last check.
template <class Src>
__device__ __forceinline__ RowInfo GtfRows::line(const Src &src, int s, int e, const GtfRowsDev &a, unsigned long long out, bool store) {
    RowInfo r;
    r.code = 0;
    r.valid = 0;
    if (e > s && src.b(s) == '#') return r;  // a comment or a `#!` directive, wherever it stands: no row
    const GffCodes pe = {EXG_PE_GTF_FIELD_COUNT, EXG_PE_GTF_EMPTY_FIELD, EXG_PE_GTF_POSITION, EXG_PE_GTF_SCORE, EXG_PE_GTF_STRAND, EXG_PE_GTF_FRAME};
    Gff8 f;
    r.code = gff_leading8(src, s, e, pe, &f);
    if (r.code) return r;
    if (store) {
        if (f.slow_len && a.d_col[5]) {
            ScoreSlowList *list = reinterpret_cast<ScoreSlowList *>(a.d_col[9]);
            const unsigned int k = atomicAdd(&list->count, 1u);
            if (k >= ScoreSlowList::kCap || out > 0xFFFFFFFFull) {
                r.code = EXG_PE_GTF_SCORE;
                return r;
            }
            list->lit[k].off = src_offset(src, f.slow_s, a.payload_base);
            list->lit[k].len = (uint32_t)f.slow_len;
            list->lit[k].row = (uint32_t)out;
        }
        gff_store8(src, s, f, a.d_col, out);
        put_str(a.d_col[8], out, src.str(f.t[7] + 1, (uint32_t)(e - f.t[7] - 1)));
    }
    r.valid = f.valid | 8u;
    return r;
}

// the score literals the scan left to the exact parser (one block; the arrays of f32_parse_exact live here, not in the scan)
__global__ __launch_bounds__(64) void k_gtf_score_fix(const ScoreSlowList *list, const uint8_t *d_in, float *score, uint64_t capacity) {
    const uint32_t n = list->count < ScoreSlowList::kCap ? list->count : ScoreSlowList::kCap;
    for (uint32_t k = threadIdx.x; k < n; k += 64) {
        const ScoreSlowList::Lit lit = list->lit[k];
        uint32_t bits = 0;
        if (lit.row < capacity && f32_parse_exact(d_in + lit.off, (int)lit.len, &bits) == 0) score[lit.row] = __uint_as_float(bits);
    }
}

// exg_gtf_scan_args with the driver's tenth column (the slow list / the keep words): what line_rows_scan reads
struct GtfDriverArgs {
    const void *d_input;
    uint64_t n_bytes, lead, payload_base;
    uint32_t flags, algo;
    void *d_columns[kGtfDevColumns];
    uint64_t *d_validity[kGtfDevColumns];
    uint64_t capacity_records;
    void *d_workspace;
    uint64_t workspace_bytes;
    exg_scan_result *d_result;
    void *stream;
};

static constexpr uint64_t kGtfSlowBytes = (sizeof(ScoreSlowList) + 255) & ~255ull;
uint64_t gtf_slow_list_bytes() { return kGtfSlowBytes; }

// ---- exg_gtf_attributes ------------------------------------------------------------------------------------------------
namespace gtfattr {

static constexpr uint32_t kGrid = 4096;  // workgroups of four waves that take the rows in turn

// workspace: ent (n + 1 u64) | scan scratch | err (u64) | cnt (u32 x n)
struct Ws {
    uint64_t *ent, *tmp, *err;
    uint32_t *cnt;
    uint64_t bytes;
};
static Ws ws_layout(uint64_t n, void *base) {
    Ws w;
    uint64_t *p = (uint64_t *)base;
    w.ent = p, p += n + 1;
    w.tmp = p, p += xscan_tmp_entries(n);
    w.err = p, p += 1;
    w.cnt = (uint32_t *)p, p += (n + 1) / 2;
    w.bytes = (uint64_t)((uint8_t *)p - (uint8_t *)base) + 64;
    return w;
}
struct CntF {
    const uint32_t *cnt;
    __device__ __forceinline__ uint64_t operator()(uint64_t r) const { return cnt[r]; }
};

// a token [start, start + len) of the row at s as a string_t: up to 12 bytes inlined, else its prefix and the row's pointer + start
__device__ __forceinline__ uint4 token_string(const uint8_t *s, uint64_t row_ptr, uint32_t start, uint32_t len) {
    uint32_t o[3] = {0, 0, 0};
    const uint32_t take = len > EXG_INLINE_LENGTH ? 4u : len;
#pragma unroll
    for (uint32_t i = 0; i < EXG_INLINE_LENGTH; i++)
        if (i < take) put_byte(o, i, s[start + i]);
    return len > EXG_INLINE_LENGTH ? long_string(len, o[0], row_ptr + start) : inline_string(len, o);
}

// One row, one wave: the entries of field s[0, len).  Returns the entries (value tokens) found; *err = the offset a left-to-right
// parser stops at (kNoError: none).  kEmit: entry k of the row goes to keys[k] / vals[k] for k < room.
// Classes of a byte, from the inclusive prefix parity x of the quote ballot q: opening quote q & x, closing quote q & ~x, quoted
// content ~q & x; outside of quotes space, `;` (position len is a virtual one: the field's end closes the last entry) and the
// rest, "word" bytes.  A token starts at a word byte or an opening quote behind a separator; T = the tokens of the entry that
// start in front of a position.  The rules, each a mask: an opening quote behind a word byte or a closing quote; a word byte
// behind a closing quote; a key (T = 0) that begins with a quote; a third token; a `;` or the end behind a lone key (T = 1).
template <bool kEmit>
__device__ __forceinline__ uint32_t walk_row(const uint8_t *s, uint32_t len, uint64_t row_ptr, uint32_t lane, uint64_t *err, uint4 *keys, uint4 *vals,
                                             uint64_t room) {
    const unsigned long long lower = (1ull << lane) - 1ull;
    unsigned long long carry_sep = 1, carry_w = 0, carry_qe = 0, qpar = 0;
    uint32_t carry_tok = 0, carry_start = 0, last_open = 0, nk = 0, nv = 0;
    *err = kNoError;
#pragma unroll 1
    for (uint64_t base = 0; base <= len; base += 64) {
        const uint64_t pos = base + lane;
        const bool real = pos < len;
        const uint32_t ch = real ? s[pos] : 0u;
        const unsigned long long rm = __ballot(real), vm = __ballot(pos == len);
        const unsigned long long q = __ballot(ch == '"');
        unsigned long long x = q;
        x ^= x << 1, x ^= x << 2, x ^= x << 4, x ^= x << 8, x ^= x << 16, x ^= x << 32;
        if (qpar) x = ~x;
        const unsigned long long QO = q & x, QE = q & ~x, outside = ~q & ~x;
        const unsigned long long SP = __ballot(ch == ' ') & outside;
        const unsigned long long SE = (__ballot(ch == ';') & outside) | (vm & ~x);
        const unsigned long long W = rm & outside & ~SP & ~SE;
        const unsigned long long prev_sep = ((SP | SE) << 1) | carry_sep, prev_w = (W << 1) | carry_w, prev_qe = (QE << 1) | carry_qe;
        const unsigned long long S = (W | QO) & prev_sep;
        const unsigned long long m = SE & lower;
        const uint32_t T = m ? (uint32_t)__popcll(S & lower & ~((2ull << (63 - __clzll((long long)m))) - 1ull)) : carry_tok + (uint32_t)__popcll(S & lower);
        const bool is_s = (S >> lane) & 1ull;
        const unsigned long long S1 = __ballot(is_s && T == 0), S2 = __ballot(is_s && T == 1);
        const unsigned long long E = (QO & ~prev_sep) | (W & prev_qe) | (S1 & QO) | __ballot(is_s && T >= 2) | __ballot(((SE >> lane) & 1ull) && T == 1);
        if (kEmit && ((rm | vm) >> lane) & 1ull) {
            // the lane behind a word token, or on a closing quote, writes the token: its start is the last start in front
            const unsigned long long sm = S & lower;
            const uint32_t start = sm ? (uint32_t)base + 63u - (uint32_t)__clzll((long long)sm) : carry_start;
            const bool word_end = ((prev_w & ~W) >> lane) & 1ull, quote_end = (QE >> lane) & 1ull;
            if (!(E & (lower | (1ull << lane)))) {  // (nothing behind the row's error is written)
                if (word_end && T == 1) {
                    const uint64_t k = (uint64_t)nk + __popcll(S1 & lower) - 1;
                    if (k < room) keys[k] = token_string(s, row_ptr, start, (uint32_t)pos - start);
                } else if ((word_end || quote_end) && T == 2) {
                    const uint64_t k = (uint64_t)nv + __popcll(S2 & lower) - 1;
                    const uint32_t v0 = start + (quote_end ? 1u : 0u);
                    if (k < room) vals[k] = token_string(s, row_ptr, v0, (uint32_t)pos - v0);
                }
            }
        }
        nk += (uint32_t)__popcll(S1), nv += (uint32_t)__popcll(S2);
        if (QO) last_open = (uint32_t)base + 63u - (uint32_t)__clzll((long long)QO);
        if (E) {
            *err = base + (uint64_t)(__ffsll((long long)E) - 1);
            break;
        }
        if (len - base < 64) {  // the word of the field's end: a quote that is still open is the row's error, where it opened
            if ((x >> (len - base)) & 1ull) *err = last_open;
            break;
        }
        carry_sep = ((SP | SE) >> 63) & 1ull, carry_w = (W >> 63) & 1ull, carry_qe = (QE >> 63) & 1ull, qpar = (x >> 63) & 1ull;
        carry_tok = SE ? (uint32_t)__popcll(S & ~((2ull << (63 - __clzll((long long)SE))) - 1ull)) : carry_tok + (uint32_t)__popcll(S);
        if (S) carry_start = (uint32_t)base + 63u - (uint32_t)__clzll((long long)S);
    }
    return nv;
}

// row j of the call: its field's bytes, length and pointer
struct RowRef {
    const uint8_t *s;
    uint32_t len;
    uint64_t ptr;
};
__device__ __forceinline__ RowRef row_of(const Col &c, const uint32_t *row_map, uint64_t j) {
    const uint64_t r = row_map ? (uint64_t)row_map[j] : j;
    const uint4 v = c.rows[r];
    return {src_of(c, r, v), v.x, (uint64_t)v.z | ((uint64_t)v.w << 32)};
}

// a wave per row: counting pass (every row validated, cnt[j] = its entries) and emit pass (the children and the list entries)
template <bool kEmit>
__global__ __launch_bounds__(256) void k_rows(Col c, const uint32_t *row_map, uint64_t n, Ws w, uint64_t cap, uint64_t chunk_rows, uint64_t *entries,
                                              uint64_t *chunk_base, uint4 *keys, uint4 *vals) {
    const uint32_t lane = lane_id();
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const bool fits = kEmit && w.ent[n] <= cap;
    uint64_t key = kNoError;
    for (uint64_t j = wave; j < n; j += n_waves) {
        const RowRef row = row_of(c, row_map, j);
        uint64_t err;
        if (!kEmit) {
            const uint32_t cnt = walk_row<false>(row.s, row.len, row.ptr, lane, &err, nullptr, nullptr, 0);
            if (lane == 0) w.cnt[j] = cnt;
            if (err != kNoError) {
                const uint64_t k = (j << 32) | (err + 1);
                key = k < key ? k : key;
            }
        } else {
            const uint64_t e0 = w.ent[j], cnt = w.cnt[j];
            if (lane == 0 && entries) {
                const uint64_t first = chunk_rows ? j / chunk_rows * chunk_rows : 0;
                entries[2 * j] = chunk_rows ? e0 - w.ent[first] : e0;
                entries[2 * j + 1] = cnt;
                if (chunk_rows && j == first) chunk_base[j / chunk_rows] = e0;
            }
            if (fits && cnt) walk_row<true>(row.s, row.len, row.ptr, lane, &err, keys + e0, vals + e0, cnt);
        }
    }
    if (!kEmit && lane == 0 && key != kNoError) atomicMin((unsigned long long *)w.err, (unsigned long long)key);
}

__global__ void k_finish(Col c, const uint32_t *row_map, uint64_t n, Ws w, uint64_t cap, uint64_t chunk_rows, uint64_t *chunk_base,
                         struct exg_gtf_attributes_result *res) {
    if (threadIdx.x || blockIdx.x) return;
    struct exg_gtf_attributes_result r;
    memset(&r, 0, sizeof r);
    r.n_rows = n;
    r.total_entries = w.ent[n];
    if (r.total_entries > cap) r.flags = EXG_RF_CAPACITY;
    if (chunk_rows && chunk_base) chunk_base[(n + chunk_rows - 1) / chunk_rows] = w.ent[n];
    const uint64_t key = *w.err;
    if (key != kNoError) {
        const RowRef row = row_of(c, row_map, key >> 32);
        r.error_code = EXG_PE_GTF_ATTRIBUTES;
        r.error_row = key >> 32;
        r.error_offset = (uint32_t)key - 1;
        if (r.error_offset < row.len) r.error_byte = row.s[r.error_offset];
    }
    *res = r;
}

}  // namespace gtfattr
}  // namespace exg

using namespace exg;

static_assert(sizeof(struct exg_gtf_attributes_result) == 64, "exg_gtf_attributes_result is 64 bytes");

extern "C" int exg_gtf_scan(const exg_gtf_scan_args *a) {
    if (!a || !a->d_workspace || a->workspace_bytes <= kGtfSlowBytes) {
        set_error("exg_gtf_scan: bad arguments (null pointer, or a workspace below exg_scan_workspace_bytes(EXG_FMT_GTF, n_bytes))");
        return EXG_E_INVALID_ARG;
    }
    if (!(a->flags & EXG_F_NO_STORE) && a->capacity_records && !a->d_keep) {
        set_error("exg_gtf_scan: d_keep is required unless EXG_F_NO_STORE is set");
        return EXG_E_INVALID_ARG;
    }
    // the end of the workspace is the list of score literals for the exact parser; the driver gets what is in front of it
    const uint64_t ws_main = (a->workspace_bytes - kGtfSlowBytes) & ~255ull;
    ScoreSlowList *list = reinterpret_cast<ScoreSlowList *>((uint8_t *)a->d_workspace + ws_main);
    GtfDriverArgs d;
    memset(&d, 0, sizeof d);
    d.d_input = a->d_input, d.n_bytes = a->n_bytes, d.lead = a->lead, d.payload_base = a->payload_base;
    d.flags = a->flags, d.algo = a->algo;
    for (int c = 0; c < EXG_GTF_COLUMNS; c++) d.d_columns[c] = a->d_columns[c], d.d_validity[c] = a->d_validity[c];
    d.d_columns[EXG_GTF_COLUMNS] = list;
    d.d_validity[EXG_GTF_COLUMNS] = a->d_keep;
    d.capacity_records = a->capacity_records;
    d.d_workspace = a->d_workspace, d.workspace_bytes = ws_main;
    d.d_result = a->d_result, d.stream = a->stream;
    hipStream_t stream = (hipStream_t)a->stream;
    EXG_HIP_CHECK(hipMemsetAsync(list, 0, 16, stream));
    const int rc = line_rows_scan<GtfRows>(&d);
    if (rc) return rc;
    if (!(a->flags & EXG_F_NO_STORE) && a->d_columns[5])
        hipLaunchKernelGGL(k_gtf_score_fix, dim3(1), dim3(64), 0, stream, list, (const uint8_t *)a->d_input, (float *)a->d_columns[5], a->capacity_records);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

extern "C" uint64_t exg_gtf_attributes_workspace_bytes(uint64_t n_rows) { return gtfattr::ws_layout(n_rows, nullptr).bytes; }

extern "C" int exg_gtf_attributes(const exg_gtf_attributes_args *a) {
    using namespace exg::gtfattr;
    if (!a || !a->d_result || ((uintptr_t)a->d_result & 7) || !a->d_workspace || ((uintptr_t)a->d_workspace & 7) || (a->n_rows && !a->d_strings) ||
        ((uintptr_t)a->d_strings & 15)) {
        set_error("exg_gtf_attributes: bad arguments (null or unaligned column, workspace or result)");
        return EXG_E_INVALID_ARG;
    }
    if (a->n_rows >= 0xFFFFFFFFull) {
        set_error("exg_gtf_attributes: %llu rows (at most 2^32 - 2 a call)", (unsigned long long)a->n_rows);
        return EXG_E_INVALID_ARG;
    }
    if ((a->entries_capacity && (!a->d_out_keys || !a->d_out_values || (a->n_rows && !a->d_out_entries))) || ((uintptr_t)a->d_out_keys & 15) ||
        ((uintptr_t)a->d_out_values & 15) || ((uintptr_t)a->d_out_entries & 7) || (a->chunk_rows && !a->d_out_chunk_base)) {
        set_error("exg_gtf_attributes: bad arguments (null or unaligned output)");
        return EXG_E_INVALID_ARG;
    }
    const uint64_t n = a->n_rows;
    if (a->workspace_bytes < ws_layout(n, nullptr).bytes) {
        set_error("exg_gtf_attributes: workspace too small (%llu bytes, need %llu)", (unsigned long long)a->workspace_bytes,
                  (unsigned long long)ws_layout(n, nullptr).bytes);
        return EXG_E_INVALID_ARG;
    }
    const Ws w = ws_layout(n, a->d_workspace);
    hipStream_t s = (hipStream_t)a->stream;
    if (!n) {
        EXG_HIP_CHECK(hipMemsetAsync(a->d_result, 0, sizeof(struct exg_gtf_attributes_result), s));
        if (a->chunk_rows) EXG_HIP_CHECK(hipMemsetAsync(a->d_out_chunk_base, 0, 8, s));
        return EXG_OK;
    }
    const Col c{(const uint4 *)a->d_strings, (const uint8_t *)a->d_payload, a->payload_base};
    const uint32_t grid = (uint32_t)((n + 3) / 4 < kGrid ? (n + 3) / 4 : kGrid);
    EXG_HIP_CHECK(hipMemsetAsync(w.err, 0xFF, 8, s));
    hipLaunchKernelGGL(k_rows<false>, dim3(grid), dim3(256), 0, s, c, a->d_row_map, n, w, 0ull, 0ull, (uint64_t *)nullptr, (uint64_t *)nullptr,
                       (uint4 *)nullptr, (uint4 *)nullptr);
    launch_xscan(CntF{w.cnt}, n, w.ent, w.tmp, s);
    hipLaunchKernelGGL(k_rows<true>, dim3(grid), dim3(256), 0, s, c, a->d_row_map, n, w, a->entries_capacity, a->chunk_rows,
                       (uint64_t *)a->d_out_entries, a->d_out_chunk_base, (uint4 *)a->d_out_keys, (uint4 *)a->d_out_values);
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(64), 0, s, c, a->d_row_map, n, w, a->entries_capacity, a->chunk_rows, a->d_out_chunk_base, a->d_result);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

extern "C" int exg_gtf_attributes_result(const struct exg_gtf_attributes_result *d_result, void *stream, struct exg_gtf_attributes_result *out) {
    if (const int rc = fetch_result("exg_gtf_attributes_result", d_result, stream, out)) return rc;
    if (out->error_code) {
        set_error("Invalid GTF attributes in row %llu at byte %llu", (unsigned long long)out->error_row, (unsigned long long)out->error_offset);
        return EXG_E_PARSE;
    }
    return EXG_OK;
}
