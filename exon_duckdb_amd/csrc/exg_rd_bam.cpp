// exg_rd_bam.cpp — reader level of read_bam_file_records: a BAM file is BGZF members around a binary record stream.  The
// members are inflated (and their CRCs verified) by the gzip producer into a bounded stream of decoded segments in HBM
// (exg_rd_source.hpp); this file is everything behind the inflate:
//   bam_open_file   the header, read from the front of the decoded stream through acquire() — as much of it as it takes: a
//                   header may be larger than a segment — and parsed on the host (exg_bam_header.cpp); the reference names go
//                   into a pinned table that every batch keeps alive (reference / mate_reference strings longer than 12
//                   bytes point into it) and, with their offsets, into device memory
//   bam_next_batch  one device batch = the records that lie completely inside what acquire() returned; the tail is carried
//                   by asking for the next position; a batch without a complete record (one record larger than it) asks for
//                   more.  Nothing of a BAM segment is useful on the host as it is — the sequence is packed, the qualities
//                   lack their offset, the aux data is unwanted — so no host mirror is ever requested: the selected
//                   columns' out-of-line strings are produced into a side buffer (exg_bam.hip) and only that, and the
//                   vectors, cross PCIe.
#include <string.h>

#include <algorithm>

#include "exg_bam.hpp"
#include "exg_bam_header.hpp"
#include "exg_filter.hpp"
#include "exg_rd_bam.hpp"
#include "exg_rd_source.hpp"
#include "exg_rd_stages.hpp"

namespace exg_rd {

namespace {

struct BamState {
    int device = 0;
    BamHeader header;
    std::shared_ptr<PinnedBlock> names;  // the reference names on the host (pinned, pooled): kept alive by every batch
    void *d_names = nullptr, *d_offsets = nullptr;
    size_t d_names_bytes = 0, d_offsets_bytes = 0;
    // the scan's workspace and side buffer (the reader's dev_alloc: freed with the reader, or when a batch needs larger ones); the
    // columns, validity words, row map and gather scratch are the reader's own fields, provisioned here with BAM's sizing
    void *d_ws = nullptr, *d_side = nullptr;
    uint64_t in_cap = 0, side_cap = 0;  // (in_cap = 0: provision again)
    uint64_t rows_before = 0;  // records of the current file in front of the current batch (a record error names its ordinal)
    std::atomic<uint64_t> tiles{0}, tiles_rewalked{0};
    void drop_tables() {
        if (d_names) dev_pool()->give(device, d_names, d_names_bytes);
        if (d_offsets) dev_pool()->give(device, d_offsets, d_offsets_bytes);
        d_names = d_offsets = nullptr;
    }
    ~BamState() { drop_tables(); }
};

BamState *state_of(exg_reader *r) {
    if (!r->bam_state) {
        auto s = std::make_shared<BamState>();
        s->device = r->device;
        r->bam_state = s;
    }
    return (BamState *)r->bam_state.get();
}

int ensure_buffers(exg_reader *r, BamState *s, uint64_t n, uint64_t side_bytes) {
    if (s->d_ws && n <= s->in_cap && side_bytes <= s->side_cap) return EXG_OK;
    if (s->d_ws) {
        RD_HIP(r, hipStreamSynchronize(r->stream));
        r->free_device();
    }
    // segments come at about the target size + what the scan carries over: provision once
    s->in_cap = std::max<uint64_t>(n, r->device_batch_bytes + r->device_batch_bytes / 4 + (r->src ? r->src->reserve() : 0) + 4096);
    // rows: a 150 bp read is ~350 bytes, one per 64 bytes is dense; the smallest record there can be is 37 bytes — a batch
    // that holds more rows than provisioned is found out before a column is written and provisioned for the worst case
    r->cap_records = r->worst_case_rows ? s->in_cap / exg::bam::kMinRecordBytes + 2 : s->in_cap / 64 + 4096;
    // side buffer: name + CIGAR text + sequence + qualities of a 150 bp read are about its own bytes (the sequence doubles,
    // the aux fields are dropped); a batch that needs more says so before anything is written
    s->side_cap = std::max<uint64_t>(side_bytes, s->in_cap + s->in_cap / 4);
    int rc;
    if ((rc = r->dev_alloc(&s->d_ws, exg_scan_workspace_bytes(EXG_FMT_BAM, s->in_cap)))) return rc;
    if ((rc = r->dev_alloc(&s->d_side, s->side_cap + 64))) return rc;
    if ((rc = alloc_columns(r, r->want_cols | r->filter_cols))) return rc;  // (only what is selected or the predicate reads)
    if (r->has_filter && (rc = alloc_row_selection(r))) return rc;
    if (!r->d_res && !(r->d_res = dev_pool()->take(r->device, 4096))) return fail(r, EXG_E_HIP, "out of device memory");
    return EXG_OK;
}

}  // namespace

int bam_open_file(exg_reader *r) {
    BamState *s = state_of(r);
    const std::string &path = r->files[r->file_idx - 1];
    s->rows_before = 0;
    RD_HIP(r, hipStreamSynchronize(r->stream));  // (a batch of the file before may still read the tables)
    s->drop_tables();
    PinBuf host;
    auto front = [&](uint64_t want, uint64_t *avail, bool *eof) {
        const uint8_t *d_at = nullptr;
        std::string msg;
        int rc = r->src->acquire(0, want, &d_at, avail, eof, &msg);
        if (rc) return fail(r, rc, msg + (msg.find(path) == std::string::npos ? in_file(path) : ""));
        const uint64_t len = std::min<uint64_t>(want, *avail);
        if (!host.ensure((size_t)len + 64)) return fail(r, EXG_E_HIP, "out of pinned host memory for the BAM header");
        if (len) RD_HIP(r, hipMemcpyAsync(host.p, d_at, len, hipMemcpyDeviceToHost, r->stream));
        RD_HIP(r, hipStreamSynchronize(r->stream));
        return (int)EXG_OK;
    };
    auto inspect = [&](uint64_t len, bool ended, uint64_t *need) {
        std::string why;
        const int prc = bam_parse_header((const uint8_t *)host.p, len, ended, &s->header, need, &why);
        if (prc == kBamHeaderBad) return fail(r, EXG_E_PARSE, why + in_file(path));
        return prc == kBamHeaderOk ? (int)kPrefixDone : (int)kPrefixMore;
    };
    if (int rc = read_prefix(64u << 10, front, inspect, prefix_grow_need_or_double)) return rc;
    // the reference names: a pinned table of the reader's (the batches keep it alive), and a copy on the device
    const BamHeader &h = s->header;
    auto blk = std::make_shared<PinnedBlock>();
    size_t cap = h.names.size() + 64;
    blk->p = global_pool()->take(&cap);
    if (!blk->p) return fail(r, EXG_E_HIP, "out of pinned host memory for the BAM reference names");
    blk->cap = cap, blk->pooled = true, blk->n = h.names.size();
    memcpy(blk->p, h.names.data(), h.names.size());
    s->names = blk;
    s->d_names_bytes = h.names.size() + 64, s->d_offsets_bytes = h.offsets.size() * 8;
    if (!(s->d_names = dev_pool()->take(r->device, s->d_names_bytes)) || !(s->d_offsets = dev_pool()->take(r->device, s->d_offsets_bytes)))
        return fail(r, EXG_E_HIP, "out of device memory for the BAM reference names");
    if (!h.names.empty()) RD_HIP(r, hipMemcpyAsync(s->d_names, blk->p, h.names.size(), hipMemcpyHostToDevice, r->stream));
    RD_HIP(r, hipMemcpyAsync(s->d_offsets, h.offsets.data(), h.offsets.size() * 8, hipMemcpyHostToDevice, r->stream));
    RD_HIP(r, hipStreamSynchronize(r->stream));
    r->file_pos = r->data_base = h.end;
    return EXG_OK;
}

void bam_stats(exg_reader *r, uint64_t *tiles, uint64_t *rewalked) {
    *tiles = *rewalked = 0;
    if (!r->bam_state) return;
    BamState *s = (BamState *)r->bam_state.get();
    *tiles = s->tiles.load(), *rewalked = s->tiles_rewalked.load();
}

namespace {

// what discover() found, against what is provisioned (nothing has been written yet)
enum BamVerdict { kBamAccept, kBamWiden, kBamWorstCaseRows, kBamFailRows, kBamGrowSide };
BamVerdict bam_judge(const exg_bam_scan_result &res, const exg_reader *r, const BamState *s, bool eof, bool no_store) {
    if (res.n_records == 0 && !res.error_code && !eof) return kBamWiden;  // one record larger than the batch
    if (!no_store && res.n_records > r->cap_records) return r->worst_case_rows ? kBamFailRows : kBamWorstCaseRows;
    if (!no_store && res.side_bytes > s->side_cap) return kBamGrowSide;
    return kBamAccept;
}

// rows where the predicate is TRUE -> row map; the columns are gathered through it on their way out (the side
// buffer travels whole: the strings of the rows that stay behind are in it too)
int bam_select_rows(exg_reader *r, BamState *s, const exg_bam_scan_args &a, uint64_t *k, const uint32_t **row_map) {
    ea::FilterCols fc;
    memset(&fc, 0, sizeof fc);
    for (int c = 0; c < EXG_BAM_COLUMNS; c++) {  // reference and mate_reference point into the name table, the rest into the side buffer
        const bool ref = c == 2 || c == 7;
        fc.d_base[c] = ref ? (const uint8_t *)s->d_names : (const uint8_t *)s->d_side;
        fc.payload_base[c] = ref ? a.ref_names_base : a.side_base;
    }
    return select_rows(r, &fc, nullptr, k, row_map);
}

// the vectors on the scan's stream, and the side buffer whole behind them
int bam_columns_to_host(exg_reader *r, BamState *s, const std::shared_ptr<Batch> &b, const exg_bam_scan_result &res, uint8_t *h_side, uint64_t k,
                        const uint32_t *row_map) {
    TraceRange d2h_range("exg: columns -> host");
    if (int rc = flat_columns_to_host(r, b.get(), k, row_map, r->stream, nullptr)) return rc;
    const uint64_t side_cols = 1ull << 0 | 1ull << 6 | 1ull << 8 | 1ull << 9;  // name, cigar, sequence, quality_score
    if ((r->want_cols & side_cols) && res.side_bytes) {
        RD_HIP(r, hipMemcpyAsync(h_side, s->d_side, res.side_bytes, hipMemcpyDeviceToHost, r->stream));
        r->host_vector_bytes += res.side_bytes;  // (the strings' payload is made on the device: it is part of the vectors)
    }
    RD_HIP(r, hipStreamSynchronize(r->stream));
    publish_batch(r, b);
    return EXG_OK;
}

}  // namespace

int bam_next_batch(exg_reader *r, bool count_only, uint64_t *n_records_out) {
    BamState *s = state_of(r);
    const std::string &path = r->files[r->file_idx - 1];
    const bool no_store = count_only && !r->has_filter;  // a predicate needs its columns even for COUNT(*)
    uint64_t want = r->device_batch_bytes;
    for (;;) {
        // "the rest of the segment that holds file_pos"; a batch that held no complete record asks for more than a batch
        const uint64_t ask = want > r->device_batch_bytes ? want : std::min<uint64_t>(want, 1u << 20);
        const uint8_t *d_at = nullptr;
        uint64_t n = 0;
        bool eof = false;
        std::string msg;
        int rc = r->src->acquire(r->file_pos, ask, &d_at, &n, &eof, &msg);
        if (rc) return fail(r, rc, msg + (msg.find(path) == std::string::npos ? in_file(path) : ""));
        r->n_segments = r->src->segments_consumed() + 1;
        if (n == 0 && eof) {
            r->file_done = true;
            return EXG_OK;
        }
        if ((rc = ensure_buffers(r, s, n, 0))) return rc;
        TraceRange scan_range("exg: scan bam batch");
        exg_bam_scan_args a;
        memset(&a, 0, sizeof a);
        a.d_input = d_at;
        a.n_bytes = n;
        a.flags = (eof ? EXG_F_EOF : 0u) | (no_store ? EXG_F_NO_STORE : 0u);
        a.n_ref = s->header.n_ref;
        // every record is validated whatever is selected; only the selected columns (and the predicate's) are produced
        a.columns = (r->want_cols | r->filter_cols) & ((1ull << EXG_BAM_COLUMNS) - 1);
        if (!a.columns) a.columns = 1ull << 63;
        a.d_ref_names = (const uint8_t *)s->d_names;
        a.d_ref_offsets = (const uint64_t *)s->d_offsets;
        a.ref_names_base = (uint64_t)(uintptr_t)s->names->p;
        a.d_workspace = s->d_ws;
        a.workspace_bytes = exg_scan_workspace_bytes(EXG_FMT_BAM, s->in_cap);
        a.d_result = (exg_bam_scan_result *)r->d_res;
        a.stream = r->stream;
        exg_bam_scan_result res;
        if ((rc = exg::bam::discover(&a, &res))) return fail(r, rc, exg_last_error_message());
        r->n_batches++;
        s->tiles += res.tiles, s->tiles_rewalked += res.tiles_rewalked;
        switch (bam_judge(res, r, s, eof, no_store)) {  // (the only place that scans the batch again)
            case kBamAccept: break;
            case kBamWiden: want = std::max<uint64_t>(want, n) * 2; continue;
            case kBamFailRows: return fail(r, EXG_E_CAPACITY, "more BAM records than bytes allow: internal error");
            case kBamWorstCaseRows:  // denser rows than provisioned: worst-case vectors, same batch again
                r->worst_case_rows = true;
                s->in_cap = 0;
                continue;
            case kBamGrowSide:
                if ((rc = ensure_buffers(r, s, n, res.side_bytes))) return rc;
                continue;  // (the workspace moved: same batch again)
        }
        uint64_t k = res.n_records;
        if (res.error_code) {
            r->pending_error = res.error_code;
            r->pending_error_offset = r->file_pos + res.error_offset;
            r->pending_error_text = "invalid BAM record " + std::to_string(s->rows_before + res.error_record) + ": " +
                                    exg_parse_error_string(res.error_code) + " at byte " + std::to_string(r->file_pos + res.error_offset) +
                                    " of the decoded stream of " + path;
        }
        s->rows_before += res.n_records;
        if (k && !no_store) {
            auto b = std::make_shared<Batch>();
            b->host.reserve(r->host_hint);
            b->file = s->names;
            uint8_t *h_side = nullptr;
            if (res.side_bytes && !(h_side = (uint8_t *)b->host.alloc(res.side_bytes + 64))) return fail(r, EXG_E_HIP, "out of pinned host memory");
            for (int c = 0; c < EXG_BAM_COLUMNS; c++) a.d_columns[c] = r->d_cols[c], a.d_validity[c] = (uint64_t *)r->d_col_valid[c];
            a.d_side = (uint8_t *)s->d_side;
            a.side_capacity = s->side_cap;
            a.side_base = (uint64_t)(uintptr_t)h_side;
            a.capacity_records = r->cap_records;
            if ((rc = exg::bam::emit(&a, &res))) return fail(r, rc, exg_last_error_message());
            const uint32_t *row_map = nullptr;
            if (r->has_filter && (rc = bam_select_rows(r, s, a, &k, &row_map))) return rc;
            if (k && !count_only && (rc = bam_columns_to_host(r, s, b, res, h_side, k, row_map))) return rc;
        }
        *n_records_out = k;
        if (res.error_code) {
            r->file_done = true;
        } else {
            r->file_pos += res.consumed_bytes;
            if (eof) r->file_done = true;  // (a tail behind the last record at the end of the stream is an error above)
        }
        return EXG_OK;
    }
}

}  // namespace exg_rd
