// exg_rd_rows_out.cpp — reader level, chunk boundary: the way the rows of a scanned batch take out of HBM.  The predicate (and
// GTF's keep words) -> the row map (select_rows); the flat columns and their validity words, gathered through it -> the batch's
// pinned vectors (flat_columns_to_host); the batch -> r->batch (publish_batch): these three are also exg_rd_bam.cpp's.  A text
// format's batch (RowsOut, made by next_batch — exg_rd_batch.cpp — from the scan's result and what the declaration lists of
// the attempt) adds what its strings point into: the decoded bytes or their mirror, or a side buffer of the selected columns'
// out-of-line strings; the stream the vectors travel on; VCF's nested columns, GTF's attributes, FASTA's joined sequences.
// Only 64 B/record of string_t + validity cross PCIe where the strings are zero-copy slices of a mapped file.
#include <string.h>

#include <algorithm>
#include <memory>

#include "exg_filter.hpp"
#include "exg_rd_source.hpp"

namespace exg_rd {

// compact: the selected string columns' out-of-line bytes, closed up per column into ONE side buffer
struct SideBuf {
    struct Col {
        uint64_t *d_goff = nullptr;
        uint64_t total = 0, off = 0;
    } col[12];
    uint8_t *h = nullptr;
};

int alloc_row_selection(exg_reader *r) {
    int rc;
    if ((rc = r->dev_alloc(&r->d_row_map, r->cap_records * 4 + 64))) return rc;
    if ((rc = r->dev_alloc(&r->d_gather, std::max<uint64_t>(r->cap_records * 16, sizeof(ea::FilterCols))))) return rc;
    return r->dev_alloc(&r->d_filter_tmp, (r->cap_records + 1 + ea::scan_tmp_entries(r->cap_records)) * 8);
}

int select_rows(exg_reader *r, ea::FilterCols *fc, const uint64_t *d_keep, uint64_t *k, const uint32_t **row_map) {
    const FormatDesc &f = format_desc(r->format);
    for (int c = 0; c < f.n_columns && r->has_filter; c++) {
        fc->kind[c] = filter_col_kind(f.col[c]);
        fc->data[c] = r->column_data(c).data;
        fc->validity[c] = (const uint64_t *)r->d_col_valid[c];
    }
    uint64_t *d_goff = (uint64_t *)r->d_filter_tmp, *d_tmp = d_goff + r->cap_records + 1;
    ea::FilterCols *d_fc = (ea::FilterCols *)r->d_gather;  // the scratch column is free until the gathers
    RD_HIP(r, ea::select_rows(*fc, r->has_filter ? (const ea::FilterProgram *)r->d_filter_prog : nullptr, (const uint8_t *)r->d_filter_consts, *k, d_goff,
                              d_tmp, (uint32_t *)r->d_row_map, d_fc, r->stream, k, d_keep));
    *row_map = (const uint32_t *)r->d_row_map;
    return EXG_OK;
}

int flat_columns_to_host(exg_reader *r, Batch *b, uint64_t k, const uint32_t *row_map, hipStream_t cs, const SideBuf *side) {
    const FormatDesc &f = format_desc(r->format);
    b->n_rows = k;
    b->n_cols = f.n_columns;  // schema order (exg_schema_of): VCF exposes parsed POS / QUAL in place of their raw text
    for (int c = 0; c < b->n_cols; c++) {
        b->elem[c] = 0;
        b->cols[c] = nullptr;
        if (f.col[c].nested || !r->want(c)) continue;  // (VCF id, alt, filter, info, formats: built by nested_emit — vcf_nested_columns)
        const void *src = r->column_data(c).data;
        const uint32_t es = r->column_data(c).elem;
        b->elem[c] = es;
        int rc;
        if (side && es == 16 && side->col[c].d_goff) {
            // (gathers through the row map itself; in place without one: the column is the scan's scratch from here on)
            void *dst = row_map ? r->d_gather : r->d_cols[c];
            ea::repoint_strings((const exg_string_t *)r->d_cols[c], row_map, k, side->col[c].d_goff, (uint64_t)(uintptr_t)(side->h + side->col[c].off),
                                (exg_string_t *)dst, r->stream);
            rc = column_to_host(r, b, c, dst, es, nullptr, k, nullptr, nullptr, r->stream);
        } else {
            rc = column_to_host(r, b, c, src, es, nullptr, k, row_map, r->d_gather, cs);
        }
        // the validity words of a nullable column
        if (!rc && f.col[c].validity) rc = column_to_host(r, b, c, nullptr, 0, r->d_col_valid[c], k, row_map, r->d_gather, cs);
        if (rc) return rc;
    }
    return EXG_OK;
}

void publish_batch(exg_reader *r, const std::shared_ptr<Batch> &b) {
    r->host_hint = b->host.total + b->host.total / 8 + (1u << 20);
    b->seq = r->batch_seq++;
    r->batch = b;
}

int RowsOut::columns_to_host() {
    TraceRange d2h_range("exg: columns -> host");
    const uint64_t k = scan.n_records;
    if (!b) b = std::make_shared<Batch>();
    b->host.reserve(r->host_hint);
    b->file = gz_payload ? gz_payload : r->file;
    // the projection (exg_open_args.columns): every column was parsed and validated above, only the wanted ones travel.
    // A decoded input's bytes are what its strings point into: they travel when any string column does
    const FormatDesc &f = format_desc(r->format);
    const bool any_strings = (r->want_cols & (f.string_mask() | f.nested_mask())) != 0;  // (a nested column's elements are strings too)
    if (gz_payload && any_strings && !gz_mirror) RD_HIP(r, hipMemcpyAsync(gz_payload->p, scan.d_input, n, hipMemcpyDeviceToHost, r->stream));
    if (gz_mirror && gz_front) RD_HIP(r, hipMemcpyAsync(const_cast<uint8_t *>(scan.h), scan.d_input, gz_front, hipMemcpyDeviceToHost, r->stream));
    SideBuf side;
    SideScratch side_scratch{r->device, r->stream, {}};
    int rc;
    if (compact && (rc = side_buffer(&side, &side_scratch))) return rc;
    ColDrain col_drain;
    hipStream_t cs = r->stream;
    if ((rc = columns_stream(&cs, &col_drain))) return rc;
    // (a nested column's validity is the emitter's)
    if ((rc = flat_columns_to_host(r, b.get(), k, row_map, cs, compact ? &side : nullptr))) return rc;
    if (r->format == EXG_FMT_VCF && (rc = vcf_nested_columns(cs, &col_drain))) return rc;
    if (r->format == EXG_FMT_GTF && r->want(8) && (rc = gtf_attributes(&side_scratch))) return rc;
    if (r->format == EXG_FMT_FASTA && scan.res.payload_bytes && r->want(2) && (rc = fasta_sequences(cs))) return rc;
    const double t_cols = now_s();
    RD_HIP(r, hipStreamSynchronize(r->stream));
    if (r->col_stream && !b->landed) RD_HIP(r, hipStreamSynchronize(r->col_stream));
    col_drain.cs = nullptr;
    TRACE("wait(columns -> host)", t_cols);
    const double t_mir = now_s();
    if (gz_mirror) RD_HIP(r, hipEventSynchronize(gz_mirror->ev));  // the segment's own bytes have arrived
    if (gz_mirror) TRACE("wait(host mirror of the segment)", t_mir);
    trace_at("C batch-done", r->n_batches);
    publish_batch(r, b);
    return EXG_OK;
}
// compact: the selected string columns' out-of-line bytes, closed up per column into ONE side buffer
int RowsOut::side_buffer(SideBuf *side, SideScratch *scratch) {
    const uint64_t k = scan.n_records;
    const FormatDesc &f = format_desc(r->format);
    const int ns = f.n_columns;
    const uint64_t into_input = f.string_mask() & f.payload_mask();  // the flat strings that point into the input
    uint64_t *d_tmp = (uint64_t *)scratch->take((ea::scan_tmp_entries(k) + 2) * 8);
    if (!d_tmp) return fail(r, EXG_E_HIP, "out of device memory");
    for (int c = 0; c < ns; c++) {
        if (!r->want(c) || !((into_input >> c) & 1ull)) continue;
        if (!(side->col[c].d_goff = (uint64_t *)scratch->take((k + 2) * 8))) return fail(r, EXG_E_HIP, "out of device memory");
        const ea::StrCol sc{(const exg_string_t *)r->d_cols[c], (const uint8_t *)scan.d_input, (uint64_t)(uintptr_t)scan.h};
        ea::payload_goff_from_col(sc, row_map, k, side->col[c].d_goff, d_tmp, r->stream);
        RD_HIP(r, hipMemcpyAsync(&side->col[c].total, side->col[c].d_goff + k, 8, hipMemcpyDeviceToHost, r->stream));
    }
    RD_HIP(r, hipStreamSynchronize(r->stream));
    uint64_t side_total = 0;
    for (int c = 0; c < ns; c++) side->col[c].off = side_total, side_total += (side->col[c].total + 15) & ~15ull;
    if (!side_total) return EXG_OK;
    if (!(side->h = (uint8_t *)b->host.alloc(side_total + 64))) return fail(r, EXG_E_HIP, "out of pinned host memory");
    const uint32_t big_cap = (uint32_t)(side_total / 8192 + 1);
    uint32_t *d_big = (uint32_t *)scratch->take(4 * ((size_t)big_cap + 1));
    uint8_t *d_side = (uint8_t *)scratch->take(side_total + 64);
    if (!d_side || !d_big) return fail(r, EXG_E_HIP, "out of device memory");
    for (int c = 0; c < ns; c++) {
        if (!side->col[c].d_goff || !side->col[c].total) continue;
        const ea::StrCol sc{(const exg_string_t *)r->d_cols[c], (const uint8_t *)scan.d_input, (uint64_t)(uintptr_t)scan.h};
        ea::payload_copy_from_col(sc, row_map, k, side->col[c].d_goff, d_side + side->col[c].off, d_big, big_cap, r->stream);
    }
    RD_HIP(r, hipMemcpyAsync(side->h, d_side, side_total, hipMemcpyDeviceToHost, r->stream));
    return EXG_OK;
}
// the stream the vectors travel on (*cs: the scan's when this returns without a word), and whether the batch is handed on while
// they still do (r->lazy_landing)
int RowsOut::columns_stream(hipStream_t *cs, ColDrain *col_drain) {
    // read_vcf: behind the flat columns come the nested ones' kernels (nested_emit: dozens of small launches that build — or,
    // for columns the projection leaves out, only validate — id / alt / filter / info / formats).  In one stream the
    // 200 MB of flat vectors (3.7 ms of the link) stood in front of them; on a stream of their own the copies run beside
    // them (chrom, pos, ref of a 2 GB file: 70.6 -> 49.4 ms = 42 GB/s, COUNT(*) 47 ms: A/B in one box, EXG_VCF_ONE_STREAM)
    // (FASTA, round 6: its joined sequences are as many bytes as the batch itself — on the scan's stream they shared a copy
    // engine with the next batch's upload, which landed 5 ms behind them: 9.7 ms per 256 MiB batch where the two directions
    // should overlap)
    // (EXG_VCF_ONE_STREAM is read per batch: the tests switch it inside one process)
    if ((r->format == EXG_FMT_VCF || r->format == EXG_FMT_FASTA || (!r->src && !switches().fastq_one_stream)) && !compact &&
        !getenv("EXG_VCF_ONE_STREAM")) {
        if (!r->col_stream) {
            RD_HIP(r, stream_pool()->take_d2h(r->device, &r->col_stream, /*calibrate=*/r->file && r->file->n >= (512ull << 20) && !r->mem_cap));
            RD_HIP(r, hipEventCreateWithFlags(&r->col_ev, hipEventDisableTiming));
            RD_HIP(r, hipEventCreateWithFlags(&r->flat_ev, hipEventDisableTiming));
        }
        RD_HIP(r, hipEventRecord(r->col_ev, r->stream));  // (the scan, the predicate's row map)
        RD_HIP(r, hipStreamWaitEvent(r->col_stream, r->col_ev, 0));
        *cs = col_drain->cs = r->col_stream;
    }
    // read_vcf hands its batch on while the vectors are still travelling (Batch::landed): the batch behind it — upload wait,
    // scan, the nested columns' kernels — is made beside them, and the link back to the host does not idle between batches
    r->lazy_landing = r->format == EXG_FMT_VCF && *cs == r->col_stream && *cs != r->stream && !switches().vcf_eager_landing;
    return EXG_OK;
}
// read_vcf: behind the flat columns (QUAL's validity the last of them), the hand-over to the nested columns' emitter (id, alt,
// filter, info, formats)
int RowsOut::vcf_nested_columns(hipStream_t cs, ColDrain *col_drain) {
    int rc;
    if (r->lazy_landing) {
        RD_HIP(r, hipEventRecord(r->flat_ev, cs));  // (the scan's columns are free again behind this)
        r->flat_pending = true;
    }
    if (!r->nested_state && (rc = nested_prepare(r))) return rc;
    uint64_t deliver = scan.n_records;
    const double t_ne = now_s();
    trace_at("N nested begins", r->n_batches);
    if ((rc = nested_emit(r, scan, b.get(), row_map, &deliver))) return rc;
    trace_at("N nested landed", r->n_batches);
    TRACE("nested columns (kernels + their way back)", t_ne);
    b->n_rows = deliver;
    if (r->lazy_landing) {
        RD_HIP(r, hipEventCreateWithFlags(&b->landed, hipEventDisableTiming));
        RD_HIP(r, hipEventRecord(b->landed, cs));
        col_drain->cs = nullptr;
    }
    return EXG_OK;
}
// read_gtf: `attributes` — the ninth field of the rows that leave (through the row map) -> list entries relative to their
// DataChunk + key / value strings that point into the input's bytes (exg_gtf_attributes), on the scan's stream.  The children
// are provisioned for an entry per 16 bytes of the batch; a batch of denser entries is counted first and emitted again.
int RowsOut::gtf_attributes(SideScratch *scratch) {
    const uint64_t k = scan.n_records;
    const uint64_t n_chunks = (k + r->batch_rows - 1) / r->batch_rows;
    const uint64_t ws_bytes = exg_gtf_attributes_workspace_bytes(k);
    void *d_ws = scratch->take(ws_bytes), *d_entries = scratch->take(k * 16), *d_bases = scratch->take((n_chunks + 1) * 8);
    void *d_res = scratch->take(64);
    if (!d_ws || !d_entries || !d_bases || !d_res) return fail(r, EXG_E_HIP, "out of device memory");
    exg_gtf_attributes_args a;
    memset(&a, 0, sizeof a);
    a.d_strings = (const exg_string_t *)r->d_cols[8];
    a.d_payload = scan.d_input;
    a.payload_base = (uint64_t)(uintptr_t)scan.h;
    a.d_row_map = row_map;
    a.n_rows = k;
    a.chunk_rows = r->batch_rows;
    a.d_out_entries = (exg_list_entry_t *)d_entries;
    a.d_out_chunk_base = (uint64_t *)d_bases;
    a.d_workspace = d_ws, a.workspace_bytes = ws_bytes;
    a.d_result = (struct exg_gtf_attributes_result *)d_res;
    a.stream = r->stream;
    struct exg_gtf_attributes_result ar;
    uint64_t cap = n / 16 + k + 1024;
    for (int attempt = 0;; attempt++) {
        a.entries_capacity = cap;
        if (!(a.d_out_keys = (exg_string_t *)scratch->take(cap * 16)) || !(a.d_out_values = (exg_string_t *)scratch->take(cap * 16)))
            return fail(r, EXG_E_HIP, "out of device memory");
        int rc = exg_gtf_attributes(&a);
        if (rc) return fail(r, rc, exg_last_error_message());
        rc = exg_gtf_attributes_result(a.d_result, r->stream, &ar);
        if (rc == EXG_E_PARSE)
            return fail(r, EXG_E_PARSE, std::string(exg_parse_error_string(EXG_PE_GTF_ATTRIBUTES)) + " at byte " + std::to_string(ar.error_offset) +
                                            " of the attributes of feature line " + std::to_string(ar.error_row) + " of the batch that ends at byte " +
                                            std::to_string(batch_end) + " of " + r->files[r->file_idx - 1]);
        if (rc) return fail(r, rc, exg_last_error_message());
        if (!(ar.flags & EXG_RF_CAPACITY)) break;
        if (attempt) return fail(r, EXG_E_CAPACITY, "internal: the attributes' entries do not fit the count of the pass before");
        cap = ar.total_entries;
    }
    const uint64_t total = ar.total_entries;
    void *h_entries = b->host.alloc(k * 16), *h_bases = b->host.alloc((n_chunks + 1) * 8);
    void *h_keys = b->host.alloc(total * 16 + 16), *h_vals = b->host.alloc(total * 16 + 16);
    if (!h_entries || !h_bases || !h_keys || !h_vals) return fail(r, EXG_E_HIP, "out of pinned host memory");
    RD_HIP(r, hipMemcpyAsync(h_entries, d_entries, k * 16, hipMemcpyDeviceToHost, r->stream));
    RD_HIP(r, hipMemcpyAsync(h_bases, d_bases, (n_chunks + 1) * 8, hipMemcpyDeviceToHost, r->stream));
    if (total) {
        RD_HIP(r, hipMemcpyAsync(h_keys, a.d_out_keys, total * 16, hipMemcpyDeviceToHost, r->stream));
        RD_HIP(r, hipMemcpyAsync(h_vals, a.d_out_values, total * 16, hipMemcpyDeviceToHost, r->stream));
    }
    r->host_vector_bytes += k * 16 + (n_chunks + 1) * 8 + total * 32;
    b->nested.resize((size_t)b->n_cols);
    NVec &m = b->nested[8];
    m.type = EXG_TYPE_MAP, m.data = h_entries, m.elem = 16, m.length = k, m.child_base = (const uint64_t *)h_bases;
    m.children.resize(1);
    NVec &st = m.children[0];
    st.type = EXG_TYPE_STRUCT, st.length = total;
    st.children.resize(2);
    st.children[0].type = st.children[1].type = EXG_TYPE_VARCHAR;
    st.children[0].elem = st.children[1].elem = 16;
    st.children[0].length = st.children[1].length = total;
    st.children[0].data = h_keys, st.children[1].data = h_vals;
    return EXG_OK;
}
// FASTA: the joined sequences
int RowsOut::fasta_sequences(hipStream_t cs) {
    // by a kernel's stores, not by a copy engine: the next batch's upload (slices that each take whichever engine is free
    // when they are enqueued) ended up behind this copy on ITS engine every other batch and landed 5 ms late
    // (a decoded stream: no upload beside it, the engine is faster)
    if (switches().fasta_d2h_engine || r->src || (((uintptr_t)b->payload | (uintptr_t)r->d_payload) & 15)) {
        RD_HIP(r, hipMemcpyAsync(b->payload, r->d_payload, scan.res.payload_bytes, hipMemcpyDeviceToHost, cs));
    } else if (int prc = exg::stream_to_host(b->payload, r->d_payload, scan.res.payload_bytes, cs)) {
        return fail(r, prc, exg_last_error_message());
    }
    r->host_vector_bytes += scan.res.payload_bytes;  // (the joined sequences: the strings' payload is made on the device)
    return EXG_OK;
}

}  // namespace exg_rd
