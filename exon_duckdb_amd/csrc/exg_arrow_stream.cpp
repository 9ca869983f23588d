// exg_arrow_stream.cpp — `new_reader`, the reference's own FFI entry point (exon/include/rust.hpp:41-46,
// rust/src/arrow_reader.rs:38-166), on top of the device reader: an ArrowArrayStream whose record batches
// (<= batch_size rows) carry the reference's schema
//     FASTA  id, description, sequence                       (Utf8)
//     FASTQ  name, description, sequence, quality_scores     (Utf8)
//     VCF    chrom Utf8, pos Int64, id List<Utf8>, ref Utf8, alt List<Utf8>, qual Float32,
//            filter List<Utf8>, info Struct<##INFO keys>, formats List<Struct<##FORMAT keys>>
// so the unchanged C++ glue of the reference (WTArrowTableFunction::FileTypeBind / InitGlobal / Scan,
// module.cpp:75-294) can sit on top of it.  Every Arrow buffer is produced on the device (exg_arrow.hip,
// exg_vcf_nested.hip; the nested VCF columns by build_nested, exg_vcf_nested_build.cpp); this file parses the `filters`
// text, sizes the buffers, copies them back (arrow_emit) and hands them out as a stream (the structs: exg_arrow_export.hpp).
#include <errno.h>
#include <time.h>

#include "exg_emit.hpp"
#include "exg_filter.hpp"
#include "exg_rd_region.hpp"
#include "exg_vcf_header.hpp"

namespace exg_rd {

// ---- Arrow buffers of one batch: the conversions over Emit (exg_emit.hpp) --------------------------------------------------
uint64_t Emit::fetch_u64(const uint64_t *d) {
    uint64_t v = 0;
    if (hipMemcpyAsync(&v, d, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        if (!rc) rc = fail(r, EXG_E_HIP, "device read failed in the Arrow emitter");
    }
    return v;
}
// copies back run on their own stream, behind an event on the kernels' stream: the next column's scans and copies
// on the device overlap with this column's bytes crossing PCIe
const uint8_t *Emit::to_host(const void *d, size_t bytes) {
    // (round 6) the big buffers leave by a kernel's 16-byte stores (exg::stream_to_host), not by a copy engine: a text file's
    // next batch is uploaded beside them in slices that each take whichever engine is free — every other batch they queued
    // behind these copies and the upload landed 5 ms late (FASTQ at this boundary: batches of 5.4 and 11 ms in turn).
    // EXG_ARROW_D2H_ENGINE=1: hipMemcpyAsync as before (A/B)
    static const bool by_engine = getenv("EXG_ARROW_D2H_ENGINE") != nullptr;
    // (only beside a text file's uploads: a decoded stream sends up a fraction of the bytes, on its producer's streams, and the
    // engine's 57 GB/s beat the kernel's 50 there — bgzip FASTQ at this boundary 144 ms by kernel, 122 by engine)
    const bool by_kernel = !by_engine && bytes >= (64u << 10) && !r->src;
    void *h = halloc(by_kernel ? (bytes + 15) & ~(size_t)15 : bytes);
    if (h && bytes && lazy && !st->arena().owns(d)) {
        // (the scan's own vectors — POS, QUAL, validity words —: the next batch's scan writes them while this copy may still read)
        void *g = dalloc(bytes + 16);
        if (!g) return (const uint8_t *)h;
        if (hipMemcpyAsync(g, d, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess && !rc) rc = fail(r, EXG_E_HIP, "device copy failed in the Arrow emitter");
        d = g;
    }
    if (h && bytes) {
        hipError_t e = hipEventRecord(st->copy_ev, s);
        if (e == hipSuccess) e = hipStreamWaitEvent(st->copy_stream, st->copy_ev, 0);
        if (e == hipSuccess) {
            if (by_kernel && !(((uintptr_t)h | (uintptr_t)d) & 15)) {
                if (exg::stream_to_host(h, d, bytes, st->copy_stream) != EXG_OK) e = hipErrorUnknown;
            } else {
                e = hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st->copy_stream);
            }
        }
        if (e != hipSuccess && !rc) rc = fail(r, EXG_E_HIP, "D2H copy failed in the Arrow emitter");
    }
    return (const uint8_t *)h;
}
// validity of a row-space column whose source bitmap is indexed by scan rows
const uint8_t *Emit::row_validity(const uint64_t *d_src) {
    if (!d_src) return nullptr;
    if (!d_row_map) return to_host(d_src, bitmap_bytes(n));
    uint64_t *d = (uint64_t *)dalloc(bitmap_bytes(n));
    if (!d) return nullptr;
    ea::gather_bits(d_src, d_row_map, n, d, s);
    return to_host(d, bitmap_bytes(n));
}
// the int32 offsets of a list column over m entries (d_goff: its m + 1 offsets on the device)
const uint8_t *Emit::off32_of(const uint64_t *d_goff, uint64_t m) {
    if (!d_goff || !m) {  // (no element at all: one zero offset per entry)
        void *h = halloc((m + 1) * 4);
        if (h) memset(h, 0, (m + 1) * 4);
        return (const uint8_t *)h;
    }
    int32_t *d = (int32_t *)dalloc((m + 1) * 4);
    if (rc) return nullptr;
    ea::narrow_offsets(d_goff, m, d, s);
    return to_host(d, (m + 1) * 4);
}
bool Emit::too_long(uint64_t total) {
    if (total >= (1ull << 31) && !rc) rc = fail(r, EXG_E_CAPACITY, "a list column exceeds Arrow's int32 offsets in one device batch");
    return rc != 0;
}

// m strings of a column closed up on the device: their bytes (returned), m + 1 offsets (*d_goff) and size (*total < limit)
uint8_t *Emit::utf8_values(const ea::StrCol &c, const uint32_t *d_map, uint64_t m, uint64_t limit, uint64_t **d_goff, uint64_t *total) {
    *d_goff = (uint64_t *)dalloc((m + 1) * 8);
    uint64_t *d_tmp = (uint64_t *)dalloc(ea::scan_tmp_entries(m) * 8);
    if (rc) return nullptr;
    ea::utf8_goff_from_col(c, d_map, m, *d_goff, d_tmp, s);
    *total = fetch_u64(*d_goff + m);
    if (*total >= limit && !rc) rc = fail(r, EXG_E_CAPACITY, "a nested string column exceeds Arrow's int32 offsets in one device batch");
    if (*total >= limit) return nullptr;
    const uint32_t big_cap = (uint32_t)(*total / 8192 + 1);
    uint8_t *d_values = (uint8_t *)dalloc(*total + 16);
    uint32_t *d_big = (uint32_t *)dalloc(4 * ((size_t)big_cap + 1));
    if (rc) return nullptr;
    ea::utf8_copy_from_col(c, d_map, m, *d_goff, d_values, d_big, big_cap, s);
    return d_values;
}
// a row-space string column -> Utf8 whose int32 offsets begin anew with every record batch (a chunk's 2 GiB: checked when it lands)
AColumn Emit::utf8_top(const ea::StrCol &c, const uint64_t *d_valid_src) {
    AColumn col;
    col.kind = AColumn::kUtf8Top;
    col.length = (int64_t)n;
    const uint64_t B = r->batch_rows, n_chunks = (n + B - 1) / B;
    uint64_t *d_goff, total;
    uint8_t *d_values = utf8_values(c, d_row_map, n, ~0ull, &d_goff, &total);
    int32_t *d_off32 = (int32_t *)dalloc(n_chunks * (B + 1) * 4);
    uint64_t *d_cbase = (uint64_t *)dalloc(n_chunks * 8 + 8);
    if (rc) return col;
    ea::rebase_offsets(d_goff, n, B, d_off32, d_cbase, s);
    col.offsets = to_host(d_off32, n_chunks * (B + 1) * 4);
    col.data = to_host(d_values, total);
    col.chunk_base.resize(n_chunks + 1);
    if (n_chunks && hipMemcpyAsync(col.chunk_base.data(), d_cbase, n_chunks * 8, hipMemcpyDeviceToHost, s) != hipSuccess && !rc)
        rc = fail(r, EXG_E_HIP, "D2H copy failed in the Arrow emitter");
    col.chunk_base[n_chunks] = total;
    col.validity = row_validity(d_valid_src);
    return col;
}
// a string_t array on the device (the children the nested kernels write) -> Utf8 with absolute int32 offsets
AColumn Emit::utf8_abs(const exg_string_t *d_col, const uint8_t *d_base, uint64_t payload_base, uint64_t m, const uint8_t *h_validity) {
    AColumn col;
    col.kind = AColumn::kUtf8Abs;
    col.length = (int64_t)m;
    col.validity = h_validity;
    uint64_t *d_goff, total;
    uint8_t *d_values = utf8_values(ea::StrCol{d_col, d_base, payload_base}, nullptr, m, 1ull << 31, &d_goff, &total);
    int32_t *d_off32 = (int32_t *)dalloc((m + 1) * 4);
    if (rc) return col;
    ea::narrow_offsets(d_goff, m, d_off32, s);
    col.offsets = to_host(d_off32, (m + 1) * 4);
    col.data = to_host(d_values, total);
    return col;
}

// a row-space column of numbers the scan made (POS, QUAL)
AColumn Emit::prim(const void *d_src, int es, const uint64_t *d_valid_src) {
    AColumn col;
    col.kind = AColumn::kPrim;
    col.elem_size = es;
    col.length = (int64_t)n;
    const void *d = d_src;
    if (d_row_map) {
        void *g = dalloc(n * es);
        if (rc) return col;
        if (es == 8)
            ea::gather_u64((const uint64_t *)d_src, d_row_map, n, (uint64_t *)g, s);
        else
            ea::gather_u32((const uint32_t *)d_src, d_row_map, n, (uint32_t *)g, s);
        d = g;
    }
    col.data = to_host(d, n * es);
    col.validity = row_validity(d_valid_src);
    return col;
}

}  // namespace exg_rd

using namespace exg_rd;

namespace {

Field key_field(const KeyDef &k) {
    Field f, item;
    f.name = k.id;
    item.name = "item";
    f.format = item.format = key_type_info(k.type).arrow;
    if (k.is_list) f.format = "+l", f.children.push_back(item);
    return f;
}

static double em_now() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + ts.tv_nsec * 1e-9;
}
#define EM_TRACE(label)                                                                          \
    do {                                                                                         \
        if (getenv("EXG_TRACE")) {                                                               \
            (void)hipStreamSynchronize(r->stream);                                               \
            double _t = em_now();                                                                \
            fprintf(stderr, "[exg]   emit %-18s %.1f ms\n", label, (_t - em_t0) * 1e3);          \
            em_t0 = _t;                                                                          \
        }                                                                                        \
    } while (0)

ea::StrCol str_col(exg_reader *r, const ScanCtx &ctx, int c) {
    ea::StrCol sc{(const exg_string_t *)r->d_cols[c], (const uint8_t *)ctx.d_input, (uint64_t)(uintptr_t)ctx.h};
    if (r->format == EXG_FMT_FASTA && c == 2) {
        sc.d_base = (const uint8_t *)r->d_payload;
        sc.payload_base = (uint64_t)(uintptr_t)ctx.h_seq_payload;
    }
    return sc;
}

// the `filters` program over the scan's rows: em.n becomes the rows that pass, em.d_row_map where they are.  A region reader
// (vcf_query_reader): the rows that overlap the region, ANDed with the program when there is one
int select_rows(Emit &em, const ScanCtx &ctx) {
    exg_reader *r = em.r;
    ea::FilterCols fc;
    memset(&fc, 0, sizeof fc);
    const FormatDesc &f = format_desc(r->format);
    for (int c = 0; c < f.n_columns; c++) {
        const ea::StrCol sc = str_col(r, ctx, c);
        fc.kind[c] = filter_col_kind(f.col[c]);
        fc.data[c] = r->column_data(c).data;
        fc.d_base[c] = sc.d_base;
        fc.payload_base[c] = sc.payload_base;
        fc.validity[c] = (const uint64_t *)r->d_col_valid[c];
    }
    uint64_t *d_goff = (uint64_t *)em.dalloc((em.n + 1) * 8);
    uint64_t *d_tmp = (uint64_t *)em.dalloc(ea::scan_tmp_entries(em.n) * 8);
    uint32_t *d_map = (uint32_t *)em.dalloc(em.n * 4 + 4);
    if (em.rc) return em.rc;
    ea::FilterCols *d_fc = (ea::FilterCols *)em.dalloc(sizeof fc);
    uint64_t *d_keep = r->region ? (uint64_t *)em.dalloc((em.n + 63) / 64 * 8) : nullptr;
    if (em.rc) return em.rc;
    if (d_keep)
        if (int rc = exg_rd::region_keep(r, ctx.d_input, (uint64_t)(uintptr_t)ctx.h, ctx.n_records, d_keep)) return rc;
    EM_HIP(ea::select_rows(fc, em.st->has_filter ? (const ea::FilterProgram *)em.st->d_prog : nullptr, (const uint8_t *)em.st->d_consts, ctx.n_records, d_goff,
                           d_tmp, d_map, d_fc, r->stream, &em.n, d_keep));
    em.d_row_map = d_map;
    return EXG_OK;
}

// FASTQ / FASTA: every column is a flat string
int flat_columns(Emit &em, const ScanCtx &ctx, std::vector<AColumn> *cols) {
    exg_reader *r = em.r;
    for (int c = 0; c < format_desc(r->format).n_columns && !em.rc; c++)
        cols->push_back(em.utf8_top(str_col(r, ctx, c), (const uint64_t *)r->d_col_valid[c]));
    return em.rc;
}

// ---- VCF: the nested columns, made on the device in DuckDB's layouts (exg_vcf_nested.hpp), converted here to Arrow's
// (absolute int32 list offsets, Utf8 values closed up, Boolean bits)
struct VcfText {  // the text the nested kernels' string_t values point into
    const uint8_t *d_base;
    uint64_t pb;
};
// m values of a key's type at d (DuckDB's layout) with their validity on the host
AColumn value_col(Emit &em, const VcfText &t, uint8_t type, const char *d, uint64_t m, const uint8_t *valid) {
    AColumn col;
    col.length = (int64_t)m;
    col.validity = valid;
    if (type == vn::kInt || type == vn::kFloat) {
        col.kind = AColumn::kPrim;
        col.elem_size = 4;
        col.data = em.to_host(d, m * 4);
    } else if (type == vn::kFlag) {
        uint64_t *d_bits = (uint64_t *)em.dalloc(bitmap_bytes(m));
        if (em.rc) return col;
        vn::bytes_to_bits((const uint8_t *)d, m, d_bits, em.s);
        col.kind = AColumn::kBool;
        col.data = em.to_host(d_bits, bitmap_bytes(m));
    } else {
        col = em.utf8_abs((const exg_string_t *)d, t.d_base, t.pb, m, valid);
    }
    return col;
}
AColumn list_utf8(Emit &em, const VcfText &t, const NestedOut &no, int c) {
    AColumn col;
    col.kind = AColumn::kList;
    col.length = (int64_t)em.n;
    if (em.too_long(no.l_total[c])) return col;
    col.offsets = em.off32_of(no.d_goff + (uint64_t)c * (em.n + 1), em.n);
    col.children.push_back(em.utf8_abs((const exg_string_t *)(no.g[c].d + no.l_elems[c]), t.d_base, t.pb, no.l_total[c], nullptr));
    return col;
}
// the children of a struct over m elements: one column per key (goffs: the list keys' m + 1 offsets each, header order)
std::vector<AColumn> key_cols(Emit &em, const VcfText &t, const std::vector<KeyDef> &defs, const std::vector<NKeyBuf> &bufs, const char *base, uint64_t m,
                              const uint64_t *goffs) {
    std::vector<AColumn> kids;
    uint64_t li = 0;
    for (size_t q = 0; q < defs.size() && !em.rc; q++) {
        const NKeyBuf &kb = bufs[q];
        const KeyDef &kd = defs[q];
        const uint8_t *valid = em.to_host(base + kb.valid, bitmap_bytes(m));
        if (!kd.is_list) {
            kids.push_back(value_col(em, t, kd.type, base + kb.vals, m, valid));
            continue;
        }
        if (em.too_long(kb.total)) break;
        AColumn col;
        col.length = (int64_t)m;
        col.kind = AColumn::kList;
        col.offsets = em.off32_of(goffs ? goffs + li * (m + 1) : nullptr, m);
        col.validity = valid;
        const uint8_t *cv = em.to_host(base + kb.child_valid, bitmap_bytes(kb.total));
        col.children.push_back(value_col(em, t, kd.type, base + kb.child_vals, kb.total, cv));
        li++;
        kids.push_back(std::move(col));
    }
    return kids;
}

int vcf_columns(Emit &em, const ScanCtx &ctx, std::vector<AColumn> *cols, uint64_t *err, double &em_t0) {
    exg_reader *r = em.r;
    StreamState *st = em.st;
    const uint64_t n = em.n;
    const VcfText t{(const uint8_t *)ctx.d_input, (uint64_t)(uintptr_t)ctx.h};
    cols->push_back(em.utf8_top(str_col(r, ctx, 0), nullptr));                        // chrom
    const exg_reader::ColumnData pos = r->column_data(1), qual = r->column_data(5);
    cols->push_back(em.prim(pos.data, (int)pos.elem, nullptr));                       // pos
    AColumn c_ref = em.utf8_top(str_col(r, ctx, 3), nullptr);
    AColumn c_qual = em.prim(qual.data, (int)qual.elem, (const uint64_t *)r->d_col_valid[5]);
    if (em.rc) return em.rc;
    EM_TRACE("flat");
    const bool want_all[5] = {true, true, true, true, true};
    NestedOut no;
    if (int nrc = build_nested(em, ctx, r->batch_rows, want_all, false, &no)) return nrc;
    *err = no.err;
    EM_TRACE("nested kernels");
    cols->push_back(list_utf8(em, t, no, 0));  // id
    cols->push_back(std::move(c_ref));
    cols->push_back(list_utf8(em, t, no, 1));  // alt
    cols->push_back(std::move(c_qual));
    cols->push_back(list_utf8(em, t, no, 2));  // filter
    AColumn info;
    info.kind = AColumn::kStruct;
    info.length = (int64_t)n;
    info.children = key_cols(em, t, st->info_keys, no.info, no.g[3].d, n, no.d_goff + (uint64_t)vn::kColInfo0 * (n + 1));
    cols->push_back(std::move(info));
    AColumn fl, item;
    fl.kind = AColumn::kList;
    fl.length = (int64_t)n;
    if (em.too_long(no.S)) return em.rc;
    fl.offsets = em.off32_of(no.d_goff + (uint64_t)vn::kColSamples * (n + 1), n);
    item.kind = AColumn::kStruct;
    item.length = (int64_t)no.S;
    item.children = key_cols(em, t, st->format_keys, no.format, no.g[4].d, no.S, no.d_fgoff);
    fl.children.push_back(std::move(item));
    cols->push_back(std::move(fl));
    return em.rc;
}

// The batch's buffers are on their way: it waits for them, or takes an event behind them along; then what the consumer gets of it
int land(Emit &em, const std::shared_ptr<ABatch> &batch, uint64_t err, double &em_t0) {
    exg_reader *r = em.r;
    StreamState *st = em.st;
    EM_HIP(hipStreamSynchronize(r->stream));
    if (em.lazy) {
        const int arena_idx = st->arena_idx();
        if (!st->arena_done[arena_idx]) EM_HIP(hipEventCreateWithFlags(&st->arena_done[arena_idx], hipEventDisableTiming));
        EM_HIP(hipEventCreateWithFlags(&batch->landed, hipEventDisableTiming));
        EM_HIP(hipEventRecord(batch->landed, st->copy_stream));
        EM_HIP(hipEventRecord(st->arena_done[arena_idx], st->copy_stream));
        st->arena_busy[arena_idx] = true;
    } else {
        EM_HIP(hipStreamSynchronize(st->copy_stream));  // every buffer has landed
    }
    uint64_t n_rows = em.n;
    stop_at_value_error(r, err, &n_rows);
    for (AColumn &c : batch->root.children)
        if (c.kind == AColumn::kUtf8Top) {
            const uint64_t B = r->batch_rows;
            for (size_t k = 0; k + 1 < c.chunk_base.size(); k++)
                if (c.chunk_base[k + 1] - c.chunk_base[k] >= (1ull << 31) && k * B < n_rows)
                    return fail(r, EXG_E_CAPACITY, "a record batch holds more than 2 GiB of one string column (Arrow Utf8 offsets are int32)");
        }
    if (getenv("EXG_TRACE"))
        fprintf(stderr, "[exg] arrow emit: arena %zu of %zu MiB, %zu extra allocations (%zu MiB), %zu pinned blocks\n",
                st->arena().used >> 20, st->arena().cap >> 20, st->arena().extra.size(), st->arena().extra_bytes >> 20,
                batch->host.blocks.size());
    EM_TRACE("drain");
    st->host_hint = batch->host.total + batch->host.total / 8 + (1u << 20);
    batch->n_rows = n_rows;
    st->produced = n_rows ? batch : nullptr;
    EM_TRACE("swap batch");
    return EXG_OK;
}

// Called by next_batch with the scan's columns still in HBM.
int arrow_emit(exg_reader *r, const ScanCtx &ctx) {
    StreamState *st = (StreamState *)r->arrow_state.get();
    double em_t0 = em_now();
    // Round 6: the batch leaves this function while its buffers still cross PCIe (ABatch::landed), the batch behind it is scanned and
    // emitted beside them out of the OTHER arena — an arena is reset only when the last copy out of it has landed (arena_done).  A
    // text file: FASTQ at this boundary 111 -> 101 ms (A/B in one box).  NOT a decoded stream: its decoder's kernels run ahead on the
    // producer's streams all the time, and the emitter's kernels beside the copies AND the decoder measured slower (bgzip VCF 72 -> 86 ms,
    // bgzip FASTQ 118 -> 127).  Not under a memory cap (one arena).  EXG_ARROW_EAGER_LANDING=1: as before (A/B)
    static const bool eager_landing = getenv("EXG_ARROW_EAGER_LANDING") != nullptr;
    const bool lazy = !eager_landing && !r->mem_cap && !r->src;
    if (int rc = begin_batch(r, st, lazy)) return rc;
    EM_TRACE("arena");
    auto batch = std::make_shared<ABatch>();
    StreamDrain drain(st->copy_stream);
    batch->host.reserve(st->host_hint);
    Emit em(r, st, &batch->host, ctx.n_records, nullptr);
    em.lazy = lazy;
    if (st->has_filter || r->region)
        if (int rc = select_rows(em, ctx)) return rc;
    if (em.n == 0) {
        st->produced.reset();
        return EXG_OK;
    }
    uint64_t err = ~0ull;  // (row << 8) | code of the first typed VCF value that does not parse
    const bool flat = r->format == EXG_FMT_FASTQ || r->format == EXG_FMT_FASTA;
    if (int rc = flat ? flat_columns(em, ctx, &batch->root.children) : vcf_columns(em, ctx, &batch->root.children, &err, em_t0)) return rc;
    EM_TRACE("formats / columns");
    if (int rc = land(em, batch, err, em_t0)) return rc;
    if (lazy) drain.release();  // (the batch carries its landing event; a batch that is dropped waits for it itself: ~ABatch)
    return EXG_OK;
}

// ---- the stream -----------------------------------------------------------------------------------------------------------
int stream_get_schema(ArrowArrayStream *s, ArrowSchema *out) {
    StreamState *st = (StreamState *)s->private_data;
    Field root;
    root.format = "+s";
    root.nullable = false;
    root.children = st->schema;
    export_field(root, out);
    return 0;
}

static void produce_failed(StreamState *st, const std::string &msg) {
    st->last_error = msg;
    st->produced_state = 3;
}
// the next device batch with rows (st->produced), the end of the stream, or an error: everything that touches the reader
static void produce(StreamState *st) {
    exg_reader *r = st->r;
    DeviceGuard guard(r->device);
    st->produced.reset();
    for (;;) {
        if (r->pending_error) {
            const std::string msg = std::string(exg_parse_error_string(r->pending_error)) + " in " + r->files[r->file_idx - 1];
            r->pending_error = 0;
            r->file_done = true;
            r->file_idx = r->files.size();
            return produce_failed(st, msg);
        }
        if (r->file_done) {
            if (r->finish_source()) return produce_failed(st, r->error);
            if (r->file_idx >= r->files.size()) {
                st->produced_state = 2;
                return;
            }
            if (open_next_file(r)) return produce_failed(st, r->error);
        }
        uint64_t k;
        if (next_batch(r, false, &k)) return produce_failed(st, r->error);
        if (st->produced && st->produced->n_rows) {
            st->produced_state = 1;
            return;
        }
    }
}

int stream_get_next(ArrowArrayStream *s, ArrowArray *out) {
    StreamState *st = (StreamState *)s->private_data;
    exg_reader *r = st->r;
    memset(out, 0, sizeof *out);
    for (;;) {
        if (st->batch && st->batch_row < st->batch->n_rows) {
            // the first record batch of a device batch: the next device batch starts being made
            if (st->batch_row == 0 && !st->fan && !st->producer.joinable() && st->produced_state == 0) st->producer = std::thread(produce, st);
            if (st->batch_row == 0) st->batch->wait_landed();  // (behind the start of the next batch: its kernels run beside these copies)
            const uint64_t row0 = st->batch_row, B = r->batch_rows;
            const uint64_t len = std::min<uint64_t>(B, st->batch->n_rows - row0);
            export_rows(st->batch->root, row0, len, B, st->batch, out);
            st->batch_row += len;
            return 0;
        }
        st->batch.reset();
        if (st->fan) {
            if (st->produced_state == 3) return EIO;
            FanItem item;
            std::string msg;
            if (st->fan->next(&item, &msg)) {
                produce_failed(st, msg);
                return EIO;
            }
            if (!item.batch) return 0;  // out->release == NULL: end of stream
            st->batch = std::static_pointer_cast<ABatch>(item.batch);
            st->batch_row = 0;
            continue;
        }
        if (st->producer.joinable()) st->producer.join();
        if (st->produced_state == 0) produce(st);  // (the first batch of the stream: nothing is under way yet)
        const int state = st->produced_state;
        if (state == 3) return EIO;                // (sticky: the stream is over)
        if (state == 2) return 0;                  // out->release == NULL: end of stream
        st->produced_state = 0;
        st->batch = std::move(st->produced);
        st->batch_row = 0;
    }
}

const char *stream_last_error(ArrowArrayStream *s) {
    StreamState *st = (StreamState *)s->private_data;
    return st->last_error.empty() ? nullptr : st->last_error.c_str();
}

void stream_release(ArrowArrayStream *s) {
    if (!s || !s->release) return;
    StreamState *st = (StreamState *)s->private_data;
    if (st->producer.joinable()) st->producer.join();
    DeviceGuard guard(st->r->device);
    st->batch.reset();
    st->produced.reset();
    std::shared_ptr<void> last = std::move(st->r->arrow_state);
    last.reset();  // deletes st, and the reader with it
    s->release = nullptr;
}

ReaderResult result_error(const std::string &msg) {
    ReaderResult rr;
    rr.error = strdup(msg.c_str());
    return rr;
}

// A reader in Arrow mode + its stream state: schema (VCF: from the first file's header), the `filters` program, the
// emitter.  shard_index / shard_count / device of `oa` make it the reader of one stripe of a fan-out.  region (NULL: none): the
// reader is a region reader (exg_open_region)
int build_stream(const exg_open_args &oa, const char *filters, std::shared_ptr<StreamState> *out, std::string *err, const char *region = nullptr) {
    exg_reader *r = nullptr;
    int rc = region ? exg_open_region(&oa, region, &r) : exg_open(&oa, &r);
    if (rc) {
        std::string m = exg_last_error_message();
        // arrow_reader.rs:93-102 / :118-123
        if (m.rfind("could not", 0) != 0) m = "could not register table: " + m;
        *err = m;
        return rc;
    }
    DeviceGuard guard(r->device);
    MeterScope meter_scope(&r->meter);
    auto st = std::make_shared<StreamState>();
    st->r = r;
    // The VCF schema needs the first file's header, like register_exon_table (arrow_reader.rs:118-123).  The file
    // is let go again right after: the reference's bind opens a stream only for its schema and never releases
    // it (module.cpp:82-155), so a stream that was not read must not pin a mapping or inflated bytes in HBM.
    if (r->format == EXG_FMT_VCF && open_next_file(r)) {
        *err = "could not register table: " + r->error;
        return EXG_E_IO;
    }
    // the flat fields as the table has them (Arrow's format strings are the parser's kinds: "u" Utf8, "l" Int64, "f" Float32)
    const FormatDesc &fd = format_desc(r->format);
    for (int c = 0; c < fd.n_columns; c++) {
        Field f;
        f.name = fd.col[c].name;
        f.nullable = fd.col[c].nullable;
        if (!fd.col[c].nested) f.format = std::string(1, filter_kind(fd.col[c]));
        st->schema.push_back(f);
    }
    if (r->format == EXG_FMT_VCF) {
        // ... and the nested VCF fields by hand: id, alt, filter are lists of strings, info a struct of the header's INFO keys,
        // formats a list of structs of its FORMAT keys
        parse_vcf_header((const char *)r->file->p, (size_t)r->vcf_header_bytes, &st->info_keys, &st->format_keys);
        Field item, sample;
        item.name = sample.name = "item";
        item.format = "u";
        sample.format = "+s";
        for (auto &k : st->format_keys) sample.children.push_back(key_field(k));
        for (int c : {2, 4, 6}) st->schema[c].format = "+l", st->schema[c].children.push_back(item);  // id, alt, filter
        st->schema[7].format = "+s";                                                                     // info
        for (auto &k : st->info_keys) st->schema[7].children.push_back(key_field(k));
        st->schema[8].format = "+l", st->schema[8].children.push_back(sample);                          // formats
        if ((rc = upload_keys(r, st->info_keys, &st->nk_info)) || (rc = upload_keys(r, st->format_keys, &st->nk_format))) {
            *err = "could not register table: " + r->error;
            return rc;
        }
        r->file.reset();
        r->src.reset();  // (the decoder of a compressed file stops: it reads through the descriptor that closes next)
        r->fd_keep.reset();
        r->file_idx = 0;
        r->file_pos = 0;
        r->file_done = true;
    }
    if (filters && *filters) {
        // `SELECT * FROM exon_table WHERE <filters>` (arrow_reader.rs:125-141)
        std::string text = filters;
        const std::vector<exg_rd::FilterColumn> fcols = exg_rd::filter_columns(fd);
        exg_rd::FilterParser fp(text, fcols);
        bool parsed = false;
        try {
            parsed = fp.parse();
        } catch (const std::exception &e) {
            fp.err = e.what();
        }
        if (!parsed) {
            *err = "could not execute sql: " + fp.err;
            return EXG_E_INVALID_ARG;
        }
        st->has_filter = true;
        st->prog = fp.prog;
        st->consts = fp.consts;
        if (hipMalloc(&st->d_consts, st->consts.size() + 16) != hipSuccess ||
            hipMalloc(&st->d_prog, sizeof(ea::FilterProgram)) != hipSuccess ||
            hipMemcpy(st->d_prog, &st->prog, sizeof(ea::FilterProgram), hipMemcpyHostToDevice) != hipSuccess ||
            (!st->consts.empty() &&
             hipMemcpy(st->d_consts, st->consts.data(), st->consts.size(), hipMemcpyHostToDevice) != hipSuccess)) {
            *err = "could not execute sql: device allocation failed";
            return EXG_E_HIP;
        }
    }
    r->arrow_emit = arrow_emit;
    // the reader is owned by the stream state from here on
    r->arrow_state = std::shared_ptr<void>(st, st.get());
    *out = st;
    return EXG_OK;
}

// ---- several devices: one stripe of the input, read by a stream of its own (exg_rd_fanout.hpp) -----------------------------
struct StripeStream : FanSub {
    std::shared_ptr<StreamState> st;
    ~StripeStream() override {
        if (!st) return;
        DeviceGuard guard(st->r->device);  // (no MeterScope: the reader, and its meter, go away in here)
        st->produced.reset();
        std::shared_ptr<void> last = std::move(st->r->arrow_state);
        st.reset();
        last.reset();  // deletes the state, and the reader with it
    }
    int next(FanItem *item, std::string *e) override {
        MeterScope meter_scope(&st->r->meter);
        st->produced_state = 0;
        produce(st.get());
        if (st->produced_state == 3) {
            *e = st->last_error;
            return EXG_E_PARSE;
        }
        if (st->produced_state == 1) {
            item->rows = st->produced->n_rows;
            item->batch = std::move(st->produced);
        }
        return EXG_OK;
    }
    int count(uint64_t *, std::string *e) override {
        *e = "an Arrow stream is not counted";
        return EXG_E_UNSUPPORTED;
    }
};
struct StripeOpen {  // (FanOpen) new_reader's arguments, kept for the workers that open the stripes
    std::string format, comp, flt;
    bool has_comp;
    uint64_t rows;
    int operator()(const Stripe &s, std::unique_ptr<FanSub> *sub, std::string *e) const {
        exg_open_args a;
        memset(&a, 0, sizeof a);
        a.path = s.path.c_str();
        a.file_format = format.c_str();
        a.compression = has_comp ? comp.c_str() : nullptr;
        a.batch_rows = rows;
        a.device = s.device;
        a.shard_index = s.shard_index;
        a.shard_count = s.shard_count ? s.shard_count : 1;
        std::unique_ptr<StripeStream> x(new StripeStream());
        const int rc = build_stream(a, flt.empty() ? nullptr : flt.c_str(), &x->st, e);
        if (rc) {
            x->st.reset();
            return rc;
        }
        *sub = std::move(x);
        return EXG_OK;
    }
};

}  // namespace

extern "C" ReaderResult new_reader(ArrowArrayStream *stream_ptr, const char *uri, uintptr_t batch_size, const char *compression,
                                   const char *file_format, const char *filters) {
    if (!stream_ptr || !uri || !file_format) return result_error("new_reader: null argument");
    if (strcasecmp(file_format, "bam") == 0)
        return result_error("new_reader: BAM is served at the chunk boundary only (exg_open / read_bam_file_records); the Arrow boundary for BAM is not built");
    if (strcasecmp(file_format, "bed") == 0)
        return result_error("new_reader: BED is served at the chunk boundary only (exg_open / read_bed_file); the Arrow boundary for BED is not built");
    if (strcasecmp(file_format, "gtf") == 0)
        return result_error("new_reader: GTF is served at the chunk boundary only (exg_open / read_gtf); the Arrow boundary for GTF is not built");
    if (strcasecmp(file_format, "sam") == 0)
        return result_error("new_reader: SAM is served at the chunk boundary only (exg_open / read_sam_file_records); the Arrow boundary for SAM is not built");
    exg_open_args oa;
    memset(&oa, 0, sizeof oa);
    oa.path = uri;
    oa.file_format = file_format;
    oa.compression = compression;
    oa.batch_rows = batch_size;
    oa.shard_count = 1;  // (the front reader itself reads the whole input unless it fans out below)
    std::shared_ptr<StreamState> st;
    std::string err;
    if (build_stream(oa, filters, &st, &err)) return result_error(err);
    // The reference's FFI has no shard argument and its glue pulls the stream from one thread (rust.hpp:41-46,
    // module.cpp:36): with several devices the stream fans out by itself — stripes of the input are read by streams of
    // their own, one worker thread and one device each, and their record batches are handed out here in file order.
    std::vector<Stripe> stripes;
    unsigned workers = 1;
    if (plan_stripes(st->r->files, st->r->compression, &oa, &stripes, &workers) == EXG_OK && stripes.size() > st->r->files.size()) {
        StripeOpen open{file_format, compression ? compression : "", filters ? filters : "", compression != nullptr, batch_size};
        st->fan.reset(new FanOut(std::move(stripes), workers, std::move(open), 2));
    }
    stream_ptr->get_schema = stream_get_schema;
    stream_ptr->get_next = stream_get_next;
    stream_ptr->get_last_error = stream_last_error;
    stream_ptr->release = stream_release;
    stream_ptr->private_data = st.get();
    ReaderResult ok;
    ok.error = nullptr;
    return ok;
}

// what vcf_query_reader (include/exon_gpu.h; exon/include/rust.hpp:60-63, rust/src/vcf_query_reader.rs:31-36) calls: new_reader's
// VCF stream over a region reader.  One reader, one device: the members an index selects are not worth a fan-out
extern "C" const char *exg_vcf_query_reader(ArrowArrayStream *stream_ptr, const char *uri, const char *query, uintptr_t batch_size) {
    auto failed = [&](const std::string &msg) -> const char * { return strdup(msg.c_str()); };
    if (!stream_ptr || !uri || !query) return failed("vcf_query_reader: null argument");
    exg_open_args oa;
    memset(&oa, 0, sizeof oa);
    oa.path = uri;
    oa.file_format = "vcf";
    oa.batch_rows = batch_size;
    oa.shard_count = 1;
    std::shared_ptr<StreamState> st;
    std::string err;
    if (build_stream(oa, nullptr, &st, &err, query)) return failed(err.rfind("could not register table: ", 0) == 0 ? "could not read VCF file: " + err.substr(26) : err);
    stream_ptr->get_schema = stream_get_schema;
    stream_ptr->get_next = stream_get_next;
    stream_ptr->get_last_error = stream_last_error;
    stream_ptr->release = stream_release;
    stream_ptr->private_data = st.get();
    return nullptr;
}
