// exg_rd_batch.cpp — reader level: an open file (exg_rd_open.cpp) is scanned one device batch at a time: bytes -> HBM
// (prefetched slot / decoded segment / synchronous upload) -> scan kernels -> what the result means for the attempt; the rows
// that leave take exg_rd_rows_out.cpp's way to the batch's host vectors, or the Arrow emitter's.
// Replaces exon's BatchReader::read_batch loop behind the stream `new_reader` returns (rust/src/arrow_reader.rs:116-153)
// and the per-batch pull in WTArrowTableFunction::Scan (exon/src/exon/arrow_table_function/module.cpp:257-294).
//
// Data layout: device batches are record aligned (each starts on the first byte after the last complete record of the
// previous one); the kernels emit string_t whose pointers address host memory (the file's mapping, or the pinned block that
// receives a decoded batch), i.e. the DataChunk payload is zero-copy and only 64 B/record of string_t + validity cross
// PCIe on the way back.  Chunks are 2048-row slices of the batch's host vectors, reference counted until
// exg_release_chunk.
#include <string.h>

#include <algorithm>
#include <memory>
#include <type_traits>

#include "exg_fastq_ws.hpp"
#include "exg_filter.hpp"
#include "exg_map_guard.hpp"
#include "exg_rd_bam.hpp"
#include "exg_rd_region.hpp"
#include "exg_rd_source.hpp"
#include "exg_rd_stages.hpp"

namespace exg_rd {

int advance_batch(exg_reader *r, bool *end) {
    *end = false;
    for (;;) {
        if (r->batch && r->batch_row < r->batch->n_rows) return EXG_OK;
        if (r->pending_error) {
            // rows before the failing record have been handed out; now surface the error
            std::string msg = std::string(exg_parse_error_string(r->pending_error)) + " at byte " + std::to_string(r->pending_error_offset) + " of " +
                              r->files[r->file_idx - 1];
            if (!r->pending_error_text.empty()) msg.swap(r->pending_error_text), r->pending_error_text.clear();
            r->pending_error = 0;
            r->batch.reset();
            return fail(r, EXG_E_PARSE, msg);
        }
        if (r->file_done) {
            if (int jrc = r->finish_source()) return jrc;
            if (r->file_idx >= r->files.size()) {
                r->batch.reset();
                *end = true;
                return EXG_OK;
            }
            int rc = open_next_file(r);
            if (rc) return rc;
        }
        uint64_t k;
        int rc = next_batch(r, false, &k);
        if (rc) return rc;
    }
}

int alloc_columns(exg_reader *r, uint64_t produce) {
    // per column: what the scan writes, the validity words of a nullable one, the vector of a number parsed beside its text
    const FormatDesc &f = format_desc(r->format);
    int rc;
    for (int c = 0; c < f.n_columns; c++) {
        const ColumnDesc &d = f.col[c];
        if (!((produce >> c) & 1ull)) continue;
        if ((rc = r->dev_alloc(&r->d_cols[c], r->cap_records * f.scan_elem(c)))) return rc;
        if (d.validity && (rc = r->dev_alloc(&r->d_col_valid[c], (r->cap_records + 63) / 64 * 8))) return rc;
        if (void **parsed = r->parsed_vector(d.parsed))
            if ((rc = r->dev_alloc(parsed, r->cap_records * d.elem))) return rc;
    }
    return EXG_OK;
}

int ensure_device(exg_reader *r, uint64_t need_bytes) {
    if (r->d_ws && need_bytes <= r->d_in_cap) return EXG_OK;
    if (r->d_ws) {
        RD_HIP(r, hipStreamSynchronize(r->stream));
        r->free_device();
    }
    if (r->src)  // segments come at about the target size + what the scan carries over: provision once
        need_bytes = std::max<uint64_t>(need_bytes, r->device_batch_bytes + r->device_batch_bytes / 4 + r->src->reserve() + 4096);
    else if (r->format != EXG_FMT_FASTA && r->file)  // room for a prefetched batch (its slack included), small files stay small
        need_bytes = std::max<uint64_t>(need_bytes, std::min<uint64_t>(r->device_batch_bytes, r->file->n) + kPrefetchSlack + 64);
    uint64_t cap = std::max<uint64_t>(need_bytes, 1 << 16);
    r->d_in_cap = cap;
    // Rows the output vectors can hold.  Realistic density first (FormatDesc::bytes_per_row: a FASTQ record under 32 bytes, a FASTA
    // record or a VCF line under 16 would be unusual) — the worst case (bytes_per_row_worst: FASTQ "@\n\n+\n" = 5 bytes, FASTA
    // ">a\n" minus LF, a blank VCF line) would pin 16 B x 9 columns per input BYTE of device memory; a batch that does
    // overflow is reported by the kernels (EXG_RF_CAPACITY) and rescanned with worst-case vectors.
    const FormatDesc &f = format_desc(r->format);
    r->cap_records = cap / (r->worst_case_rows ? f.bytes_per_row_worst : f.bytes_per_row) + 4096;
    r->ws_bytes = exg_scan_workspace_bytes(r->format, cap);
    if (r->mem_cap && !r->ws_full) {
        // The general path's line index is provisioned for min(n, 1 Mi) lines whatever the batch size (8 MiB; FASTA keeps
        // four such arrays): under a memory budget, one line per 8 bytes + 64 Ki — a denser batch is reported
        // (EXG_RF_INDEX_OVERFLOW) and scanned again with the full workspace
        const uint64_t arrays = f.line_index_arrays;
        const exg::FastqWsLayout l = exg::fastq_ws_layout(cap, 0, arrays);
        const uint64_t lines = cap / 8 + 65536 + 8;
        r->ws_bytes = std::min<uint64_t>(r->ws_bytes, l.off_nl_pos + (lines + 2) * 8 * arrays);
    }
    // two upload slots (a FASTA under a memory cap: one, its batches are then not prefetched); a decoded stream is scanned in its
    // segments: none (FASTA: one, for the 16-byte aligned copy its scan wants)
    int arc = 0;
    const int n_slots = r->format == EXG_FMT_FASTA ? (r->src || r->mem_cap || switches().no_fasta_prefetch ? 1 : 2) : r->src ? 0 : 2;
    for (int k = 0; k < n_slots; k++)
        if ((arc = r->dev_alloc(&r->d_in_slot[k], cap + 64))) return arc;
    r->d_in = r->d_in_slot[0];
    r->cur_slot = 0;
    if (!r->up_stream) {
        RD_HIP(r, exg_rd::stream_pool()->take(r->device, &r->up_stream));
        for (int k = 0; k < 2; k++) RD_HIP(r, hipEventCreateWithFlags(&r->up_done_of[k], hipEventDisableTiming));
    }
    if ((arc = r->dev_alloc(&r->d_ws, r->ws_bytes))) return arc;
    if ((arc = alloc_columns(r, ~0ull))) return arc;
    const uint64_t validity_bytes = (r->cap_records + 63) / 64 * 8;
    for (uint32_t k = 0; k < f.spare_validity; k++)
        if ((arc = r->dev_alloc(&r->d_valid_spare[k], validity_bytes))) return arc;
    if (r->format == EXG_FMT_FASTA && (arc = r->dev_alloc(&r->d_payload, cap + 64))) return arc;
    // GTF: which rows are feature lines, and — a batch with `#` lines is gathered like a filtered one — the row map's buffers
    // (a region reader: which rows overlap the region — exg_rd_region.hpp)
    if ((r->format == EXG_FMT_GTF || r->region) && (arc = r->dev_alloc(&r->d_keep, validity_bytes))) return arc;
    if ((r->has_filter || r->format == EXG_FMT_GTF || r->region) && (arc = alloc_row_selection(r))) return arc;
    if (!r->d_res && !(r->d_res = exg_rd::dev_pool()->take(r->device, 4096))) return fail(r, EXG_E_HIP, "out of device memory");
    return EXG_OK;
}

int truncated_while_read(exg_reader *r) {
    if (!r->file || r->file->guard < 0 || !MapGuard::hit(r->file->guard)) return EXG_OK;
    return fail(r, EXG_E_IO, "'" + r->files[r->file_idx - 1] + "' was truncated while it was being read");
}

namespace {

// What one attempt at a batch scans (BatchOut: what the rows' way out reads of it).  Re-made at the top of every attempt: a retry
// cannot read a field of the attempt before.
struct BatchIn : BatchOut {
    uint64_t lead = 0;        // bytes of d_input in front of file_pos (the halo, and what a 16-byte boundary brings along)
    uint64_t shard_halo = 0;  // first batch of a shard that begins inside the file: bytes in front of it that travel along
    bool range_end = false;   // the batch reaches the end of this reader's bytes ...
    bool eof = false;         // ... which is the end of the file unless a later shard follows
    const void *d_input = nullptr;
    const uint8_t *h = nullptr;  // host address of the byte at d_input[0] (the strings' payload_base)
    // a decoded stream: the bytes from file_pos on (and the halo in front) made contiguous in HBM — everything up to the end of
    // the segment that holds them is this batch
    const uint8_t *src_at = nullptr;  // device address of stream byte src_pos
    uint64_t src_pos = 0;
};

// The state of one next_batch call: its stages in the order the driver (next_batch, below) runs them.  A stage returns an error
// code; what it hands to the stages behind it is in `in` (this attempt), `res` (the scan's result), `k` / `row_map` (the rows that
// leave).
struct BatchRun {
    exg_reader *const r;
    const bool count_only;
    const bool no_store;  // a predicate needs the columns even for COUNT(*)
    uint64_t want;        // bytes an attempt asks for: a device batch, doubled while a batch holds no complete record
    BatchIn in;
    exg_scan_result res;
    uint64_t first_line_index = 0;
    uint64_t k = 0;  // rows that leave: the scan's records, or those the predicate keeps (through row_map)
    const uint32_t *row_map = nullptr;
    double t_scan = 0;

    // (GTF: COUNT(*) counts feature lines, so the scan stores — d_keep alone: every column is a NULL pointer to it; a region reader
    // counts the rows its predicate keeps, which reads chrom, pos, ref and info)
    BatchRun(exg_reader *reader, bool count)
        : r(reader), count_only(count), no_store(count && !reader->has_filter && reader->format != EXG_FMT_GTF && !reader->region),
          want(reader->device_batch_bytes) {}

    // ---- 1: the size of the attempt, from `want`, the ramp and the range (in.n == 0: nothing of this reader's is left)
    void size_attempt() {
        in = BatchIn();
        // (the head of a text file: a small batch first — exg_reader.hpp ramp_bytes; the uploads behind it are sized where they are issued)
        const bool ramp = r->ramp_bytes && !r->src && !r->pf.valid && want == r->device_batch_bytes && r->range_hi > r->file_pos;
        const AttemptSize a = exg_rd::size_attempt(want, r->file_pos, r->range_hi, r->range_eof, ramp ? r->next_ramp() : ~0ull, r->shard_first,
                                                   r->data_base, r->halo_want, r->src != nullptr);
        in.n = a.n, in.range_end = a.range_end, in.eof = a.eof, in.shard_halo = a.shard_halo;
    }

    // ---- 2: a decoded stream — the segment that holds file_pos (in.n == 0: the stream has ended)
    int acquire_segment() {
        in.src_pos = r->file_pos - in.shard_halo;
        uint64_t avail = 0;
        bool src_eof = false;
        std::string msg;
        // What is asked of the stream is "the rest of the segment that holds file_pos", not a batch's worth of bytes: a
        // segment shorter than a device batch (the first windows of a file are small on purpose: latency) used to be MERGED
        // with the one behind it — a device copy of both, a pinned block of an odd size for the merged batch's payload
        // (hipHostMalloc: ~1 ms per 10 MiB) and no host mirror.  Only a batch that held no complete record asks for more.
        const uint64_t ask = (want > r->device_batch_bytes || r->format == EXG_FMT_FASTA) ? want : std::min<uint64_t>(want, 1u << 20);
        const double t_acq = now_s();
        int arc = r->src->acquire(in.src_pos, ask + in.shard_halo, &in.src_at, &avail, &src_eof, &msg);
        TRACE("acquire(decoded segment)", t_acq);
        trace_at("C acquired", r->n_batches);
        if (arc) return fail(r, arc, msg + (msg.find(r->files[r->file_idx - 1]) == std::string::npos ? " in '" + r->files[r->file_idx - 1] + "'" : ""));
        r->n_segments = r->src->segments_consumed() + 1;
        if (avail <= in.shard_halo && src_eof) {  // nothing behind file_pos: the stream has ended
            in.n = 0;
            return EXG_OK;
        }
        in.n = avail - in.shard_halo;
        in.range_end = src_eof;
        in.eof = in.range_end && r->range_eof;
        return r->fa_shard ? fasta_shard_end(avail) : EXG_OK;
    }
    // a shard of a compressed FASTA: where does the first record begin that is NOT this shard's?  (mark 1: the decoded offset behind
    // its own members / frames — while it is not set, nothing handed out so far lies behind it)
    int fasta_shard_end(uint64_t avail) {
        uint64_t own_end = 0;
        if (r->fa_end == ~0ull && r->src->peek_mark(1, &own_end)) {
            if (own_end <= r->file_pos) {
                r->fa_end = r->file_pos;
            } else if (own_end < in.src_pos + avail) {
                uint64_t pos = ~0ull;
                if (int arc = fetch_word(r, &pos, [&](void *d_word) {
                        return exg_fasta_find_record(in.src_at, own_end - in.src_pos, avail, 0, (uint64_t *)d_word, r->stream);
                    }))
                    return arc;
                if (pos != ~0ull) r->fa_end = in.src_pos + pos;
            }
        }
        if (r->fa_end != ~0ull) {
            in.n = r->fa_end <= r->file_pos ? 0 : r->fa_end - r->file_pos;
            in.range_end = in.eof = true;
        }
        return EXG_OK;
    }

    // ---- 3: the input of the scan: the inflated bytes already in HBM (gzip), the prefetched slot, or a synchronous
    // H2D copy.  In the first two cases the batch start is only byte aligned: the buffer starts at the
    // 16-byte boundary below it and `lead` skips the tail of the previous record (whose last '\n' is
    // then inside the buffer).
    bool prefetch_covers_file_pos() const {
        return r->pf.valid && want == r->device_batch_bytes && r->file_pos >= r->pf.file_start && r->file_pos < r->pf.file_start + r->pf.len;
    }
    // The batch about to be scanned is on its way (or there); if its upload is the one this call will use, the batch
    // AFTER it starts travelling now, into the slot of the batch that was scanned last (free: its columns have left) —
    // issued after this call's scan, an upload began only when the link had already been idle for a scan + a D2H.
    void upload_second_ahead() {
        if (switches().no_prefetch || r->pf2.valid || r->src || r->format == EXG_FMT_FASTA || !prefetch_covers_file_pos() ||
            !r->d_in_slot[r->pf.slot ^ 1] || r->up_thread_of[r->pf.slot ^ 1].joinable())
            return;
        const uint64_t end1 = r->pf.file_start + r->pf.len;  // where the coming batch's bytes end
        if (end1 >= r->range_hi) return;
        const PrefetchWindow w = prefetch_window(r->file_pos, end1, kPrefetchSlack);
        if (const uint64_t len = w.len(r->range_hi, r->next_ramp(), r->d_in_cap)) start_upload(r, &r->pf2, w.start, len, r->pf.slot ^ 1);
    }
    int bind_input() {
        upload_second_ahead();
        trace_at("N batch begins", r->n_batches);
        if (int rc = r->join_prefetch()) return rc;  // the upload thread of the previous call (its error is this call's)
        trace_at("N upload thread joined", r->n_batches);
        in.h = (const uint8_t *)r->file->p + r->file_pos;
        in.batch_end = r->file_pos + in.n;
        if (r->src) return bind_decoded();
        return prefetch_covers_file_pos() ? bind_prefetched() : bind_uploaded();
    }
    int bind_decoded() {
        in.lead = in.shard_halo + (in.src_pos & 15);
        in.d_input = in.src_at - (in.src_pos & 15);
        in.n += in.lead;
        if (r->format == EXG_FMT_FASTA) {
            // the FASTA scan wants its batch on a 16-byte boundary with nothing in front: a device copy (the decoders
            // in front of it run at a few percent of what a copy does)
            if (in.shard_halo) return fail(r, EXG_E_INVALID_ARG, "internal: a FASTA batch has no halo");
            in.n -= in.lead;
            RD_HIP(r, hipMemcpyAsync(r->d_in_slot[0], in.src_at, in.n, hipMemcpyDeviceToDevice, r->stream));
            RD_HIP(r, hipMemsetAsync((char *)r->d_in_slot[0] + in.n, 0, 16, r->stream));
            r->d_in = r->d_in_slot[0];
            in.d_input = r->d_in;
            in.lead = 0;
        }
        return route_payload();
    }
    // where a decoded batch's strings will point: `in.h` and the payload route
    int route_payload() {
        // A projection that leaves payload-bearing columns out (SELECT name FROM read_fastq('x.fastq.gz'); chrom, pos, ref of a
        // bgzip VCF): the decoded bytes stay in HBM, the out-of-line strings of the selected columns are closed up into a side
        // buffer behind the scan and only that crosses PCIe (payload_*_from_col, repoint_strings).  Not when a nested VCF
        // column is selected: its element views are cut out of the line's text by the emitter.
        const bool to_host = !count_only && !r->arrow_emit;
        const PayloadRoute route = to_host ? payload_route(r) : kPayloadNone;
        in.compact = route == kPayloadCompact;
        if (in.compact || !to_host) {
            // (compact: a base the side buffer's pointers replace.)  COUNT(*) / the Arrow stream: no host copy; h is only the base the
            // device subtracts again
            in.h = (const uint8_t *)(uintptr_t)0x100000000000ull + (r->file_pos - in.lead);
            return EXG_OK;
        }
        // The strings of this batch point into host memory that holds the decoded bytes.  From the first such batch on
        // the producer sends every segment to the host as it hands it over (HostMirror: the copy runs while the segment
        // waits in the queue and while this thread is busy with the batch in front): the batch then points into that
        // block, and only the bytes in front of the segment's own — the tail carried over from the segment before —
        // are copied here.  A segment without a mirror (pushed before the first call, a block of the consumer's own
        // making, FASTA) is copied behind the scan as before.
        const uint8_t *h_at = nullptr;
        uint64_t m_from = 0;
        if (route == kPayloadMirror) r->src->want_host_mirror();
        if (route == kPayloadMirror && r->src->host_view((const uint8_t *)in.d_input, &h_at, &m_from, &in.gz_mirror)) {
            const uint64_t first = in.src_pos - (in.src_pos & 15);  // the stream offset of d_input[0]
            in.gz_payload = in.gz_mirror->blk;
            in.h = h_at;
            in.gz_front = m_from > first ? std::min<uint64_t>(in.n, m_from - first) : 0;
            return EXG_OK;
        }
        in.gz_mirror.reset();
        in.gz_payload = std::make_shared<PinnedBlock>();
        size_t cap = in.n + 64;
        in.gz_payload->p = global_pool()->take(&cap);
        if (!in.gz_payload->p) return fail(r, EXG_E_HIP, "out of pinned host memory for the inflated bytes");
        in.gz_payload->cap = cap;
        in.gz_payload->pooled = true;
        in.gz_payload->n = in.n;
        in.h = (const uint8_t *)in.gz_payload->p;
        return EXG_OK;
    }
    int bind_prefetched() {
        const uint64_t off = r->file_pos - r->pf.file_start;
        in.lead = off & 15;
        r->cur_slot = r->pf.slot;
        r->d_in = r->d_in_slot[r->cur_slot];
        in.d_input = (const uint8_t *)r->d_in + (off - in.lead);
        in.batch_end = r->pf.file_start + r->pf.len;
        in.n = in.batch_end - r->file_pos + in.lead;
        in.range_end = in.batch_end == r->range_hi;
        in.eof = in.range_end && r->range_eof;
        in.h -= in.lead;
        r->pf.valid = false;
        RD_HIP(r, hipStreamWaitEvent(r->stream, r->up_done_of[r->cur_slot], 0));
        return EXG_OK;
    }
    int bind_uploaded() {
        if (r->pf.valid) RD_HIP(r, hipStreamSynchronize(r->up_stream));  // a prefetch that missed: let it land first
        r->pf.valid = false;
        r->d_in = r->d_in_slot[r->cur_slot];
        in.lead = in.shard_halo;
        int rc;
        if (r->format == EXG_FMT_FASTA && in.n > (512ull << 20)) {
            // a whole genome in one batch: through two 256 MiB pinned windows, not one pinned block of its size
            rc = upload_file(r, r->d_in, in.n, r->file_pos);
            if (!rc && hipMemsetAsync((char *)r->d_in + in.n, 0, 16, r->stream) != hipSuccess) rc = fail(r, EXG_E_HIP, "hipMemsetAsync failed");
        } else {
            rc = upload_range(r, r->file_pos - in.lead, in.n + in.lead, r->cur_slot, r->stream);
        }
        if (rc) return rc;
        in.d_input = r->d_in;
        in.n += in.lead;
        in.h -= in.lead;
        return EXG_OK;
    }
    // While the columns travel back (and the consumer works through the chunks): the bytes the next batch will need
    // move into the other slot — unless they left at the top of this call already (pf2), which is the steady state
    void prefetch_next() {
        // FASTA (round 6: its batches were uploaded, scanned and sent back one after the other — 22.7 GB/s end to end against
        // FASTQ's 50): the scan wants its batch at a 16-byte boundary with nothing in front, and where the next batch begins —
        // behind this one's last whole record — is known with the scan's result: its upload starts HERE, at exactly that file
        // offset into the other slot's first byte (no slack, no lead), beside this batch's sequences on their way back
        const bool fasta = r->format == EXG_FMT_FASTA;
        const bool can = !in.range_end && !res.error_code && !r->src && want == r->device_batch_bytes && !switches().no_prefetch && (!fasta || res.n_records);
        const PrefetchWindow w = prefetch_window(r->file_pos, in.batch_end, kPrefetchSlack, fasta ? r->file_pos + (res.consumed_bytes - in.lead) : ~0ull);
        const int other = r->cur_slot ^ 1;
        if (r->pf2.valid) {
            // (its length was chosen where it was issued: a step of the ramp, or a full batch)
            if (can && r->pf2.file_start == w.start && r->pf2.len > 0 && r->pf2.slot == other) {
                r->pf = r->pf2;
                r->pf2.valid = false;
            } else {
                r->drop_prefetch2();  // (the batch turned out otherwise: an error, a retry, the end of the range)
            }
        }
        if (can && !r->pf.valid && r->d_in_slot[other] && !r->up_thread_of[other].joinable()) {
            const uint64_t ramp_before = r->ramp_bytes;
            if (const uint64_t len = w.len(r->range_hi, r->next_ramp(), r->d_in_cap)) start_upload(r, &r->pf, w.start, len, other);
            else r->ramp_bytes = ramp_before;
        }
    }

    // ---- 4: the first batch of a FASTQ shard — the 4-line phase of the line that holds the shard's first byte, from the bytes around
    // the cut ('@' opens a record but also quality lines, so several records are looked at: exg_fastq_guess_phase)
    int fastq_first_line_phase() {
        first_line_index = 0;
        if (!in.lead || !r->shard_first || r->format != EXG_FMT_FASTQ) return EXG_OK;
        uint32_t guess = 0xFFFFFFFFu;
        int rc = fetch_word(r, &guess, [&](void *d_word) { return exg_fastq_guess_phase(in.d_input, in.n, in.lead, (uint32_t *)d_word, r->stream); });
        if (rc) return rc;
        if (guess <= 3) {
            uint8_t prev = 0;
            if (r->src) {
                RD_HIP(r, hipMemcpyAsync(&prev, (const uint8_t *)in.d_input + in.lead - 1, 1, hipMemcpyDeviceToHost, r->stream));
                RD_HIP(r, hipStreamSynchronize(r->stream));
            } else {
                prev = ((const uint8_t *)r->file->p)[r->file_pos - 1];
            }
            first_line_index = prev == '\n' ? guess : (guess + 3) % 4;
        } else if (r->src) {
            // a shard of a compressed input: exact when the halo begins with the file (the newlines in front are then all
            // in HBM); else (few lines in view — records far longer than the halo — or several phases fit) the newlines in
            // front of the shard's own bytes are counted by a decoder of their own, segment by segment
            uint64_t nl = 0;
            if (r->data0_is_line_start && in.lead == r->file_pos) {
                if ((rc = fetch_word(r, &nl, [&](void *d_word) { return exg_count_newlines(in.d_input, 0, in.lead, (uint64_t *)d_word, r->stream); }))) return rc;
            } else {
                if (!r->exact_nl_known) {
                    if ((rc = count_newlines_in_front(r, &r->exact_nl))) return rc;
                    r->exact_nl_known = true;
                }
                nl = r->exact_nl;
            }
            first_line_index = nl;
        } else {
            // too few lines around the cut to tell (a tiny file, a tiny shard) or several phases fit: count the
            // newlines in front of it — exact, and only as slow as a memchr over the page cache
            const char *d = (const char *)r->file->p;
            uint64_t nl = 0;
            for (const char *q = d, *end = d + r->file_pos; q < end;) {
                const void *hit = memchr(q, '\n', (size_t)(end - q));
                if (!hit) break;
                nl++;
                q = (const char *)hit + 1;
            }
            first_line_index = nl;
        }
        return EXG_OK;
    }

    // ---- 5: the scan.  One launch function per format fills its args from `in`; `algo` is the reader's sticky choice, or
    // EXG_ALGO_MULTIPASS for the rescan of a launch the fused kernels gave up
    uint32_t scan_flags() const {
        // a line starts at d_input[0] when the batch is record aligned, or when a shard's halo reaches back to the
        // first byte behind the header
        const bool at_line_start = in.lead == 0 || (r->shard_first && in.shard_halo && in.lead == in.shard_halo && r->data0_is_line_start &&
                                                    r->file_pos - in.lead == r->data_base);
        return (at_line_start ? EXG_F_BOF : 0u) | (in.eof ? EXG_F_EOF : 0u) | (no_store ? EXG_F_NO_STORE : 0u);
    }
    template <class Args>
    void fill_common(Args *a) const {  // what every format's scan is told
        memset(a, 0, sizeof *a);
        a->d_input = in.d_input;
        a->n_bytes = in.n;
        a->payload_base = (uint64_t)(uintptr_t)in.h;
        a->flags = scan_flags();
        a->capacity_records = r->cap_records;
        a->d_workspace = r->d_ws;
        a->workspace_bytes = r->ws_bytes;
        a->d_result = (exg_scan_result *)r->d_res;
        a->stream = r->stream;
    }
    int launch_fastq(uint32_t algo) {
        exg_fastq_scan_args a;
        fill_common(&a);
        a.lead = in.lead;
        a.first_line_index = first_line_index;
        a.algo = algo;
        a.d_name = (exg_string_t *)r->d_cols[0];
        a.d_description = (exg_string_t *)r->d_cols[1];
        a.d_sequence = (exg_string_t *)r->d_cols[2];
        a.d_quality = (exg_string_t *)r->d_cols[3];
        a.d_description_validity = (uint64_t *)r->d_col_valid[1];
        return scan_rc(exg_fastq_scan(&a));
    }
    int launch_vcf(uint32_t algo) {
        exg_vcf_scan_args a;
        fill_common(&a);
        a.lead = in.lead;
        a.algo = algo;
        for (int c = 0; c < 9; c++) a.d_fields[c] = (exg_string_t *)r->d_cols[c];
        if (!r->arrow_emit) {
            // The projection reaches the kernel (a NULL column is skipped: 16 B per row less to write): POS / QUAL leave as
            // numbers, their text is nobody's; CHROM / REF are written when they are selected or the predicate reads them.
            // The other five feed the nested columns, which are built — and validated: a malformed value is the same error
            // whether or not its column is selected — from their text
            a.d_fields[1] = a.d_fields[5] = nullptr;
            for (int c : {0, 3})
                if (!r->want(c) && !((r->filter_cols >> c) & 1ull) && !r->region) a.d_fields[c] = nullptr;  // (the region predicate reads both)
        }
        a.d_pos = (int64_t *)r->d_pos;
        a.d_qual = (float *)r->d_qual;
        a.d_qual_validity = (uint64_t *)r->d_col_valid[5];
        a.d_formats_validity = (uint64_t *)r->d_col_valid[8];
        if (r->flat_pending) {  // (the batch before: its flat columns' copies read what this scan writes)
            RD_HIP(r, hipStreamWaitEvent(r->stream, r->flat_ev, 0));
            r->flat_pending = false;
        }
        return scan_rc(exg_vcf_scan(&a));
    }
    // BED, SAM, GTF: a line is a row of n_columns fields.  The projection reaches the kernel (a NULL column is validated, not
    // written): `produce` has a bit for every column that is selected or that the predicate reads
    template <class Args>
    int launch_line_rows(uint32_t algo, int n_columns, uint64_t produce, int (*entry)(const Args *)) {
        Args a;
        fill_common(&a);
        a.lead = in.lead;
        a.algo = algo;
        for (int c = 0; c < n_columns; c++) {
            if (!((produce >> c) & 1ull)) continue;
            a.d_columns[c] = r->d_cols[c];
            a.d_validity[c] = (uint64_t *)r->d_col_valid[c];
        }
        if constexpr (std::is_same<Args, exg_gtf_scan_args>::value) a.d_keep = (uint64_t *)r->d_keep;
        return scan_rc(entry(&a));
    }
    int launch_fasta() {
        in.b = std::make_shared<Batch>();
        if (!count_only) {
            in.b->payload = in.b->host.alloc(in.n + 64);
            if (!in.b->payload) return fail(r, EXG_E_HIP, "out of pinned host memory");
        }
        exg_fasta_scan_args a;
        fill_common(&a);
        a.seq_payload_base = (uint64_t)(uintptr_t)in.b->payload;
        a.d_id = (exg_string_t *)r->d_cols[0];
        a.d_description = (exg_string_t *)r->d_cols[1];
        a.d_sequence = (exg_string_t *)r->d_cols[2];
        a.d_description_validity = (uint64_t *)r->d_col_valid[1];
        a.d_seq_payload = (uint8_t *)r->d_payload;
        return scan_rc(exg_fasta_scan(&a));
    }
    int scan_rc(int rc) { return rc ? fail(r, rc, exg_last_error_message()) : EXG_OK; }
    int launch_scan(uint32_t algo) {
        const uint64_t produce = r->want_cols | r->filter_cols;
        switch (r->format) {
            case EXG_FMT_FASTQ: return launch_fastq(algo);
            case EXG_FMT_VCF: return launch_vcf(algo);
            case EXG_FMT_BED: return launch_line_rows<exg_bed_scan_args>(algo, EXG_BED_COLUMNS, produce, exg_bed_scan);
            case EXG_FMT_SAM: return launch_line_rows<exg_sam_scan_args>(algo, EXG_SAM_COLUMNS, produce, exg_sam_scan);
            // (COUNT(*) without a predicate: no column at all.  Column 8 is the raw ninth field, what `attributes` is built from)
            case EXG_FMT_GTF: return launch_line_rows<exg_gtf_scan_args>(algo, EXG_GTF_COLUMNS, count_only ? r->filter_cols : produce, exg_gtf_scan);
            default: return launch_fasta();
        }
    }
    int scan() {
        int rc = launch_scan(r->fused_algo);
        if (rc) return rc;
        r->n_batches++;
        t_scan = now_s();
        rc = exg_fetch_result((const exg_scan_result *)r->d_res, r->stream, &res);
        if (rc) return fail(r, rc, exg_last_error_message());
        if (r->format != EXG_FMT_FASTA && (res.flags & EXG_RF_FALLBACK)) {
            // (no fused launch gives a batch up any more — long records, dense halves and bytes >= 0x80 are the any-shape
            // scan's —; should one ever say so, the general path takes the batch)
            if ((rc = launch_scan(EXG_ALGO_MULTIPASS))) return rc;
            rc = exg_fetch_result((const exg_scan_result *)r->d_res, r->stream, &res);
            if (rc) return fail(r, rc, exg_last_error_message());
            res.flags |= EXG_RF_FALLBACK;
        }
        return EXG_OK;
    }

    // ---- 6: what the result means for the attempt (the driver's switch acts on it), and for the scan the next batch starts with
    BatchVerdict judge() {
        const uint64_t tile_bytes = format_desc(r->format).tile_bytes;
        const bool vcf = r->format == EXG_FMT_VCF;
        const bool no_index = vcf && getenv("EXG_NO_VCF_INDEX") != nullptr;  // (per batch: the tests switch it inside one process)
        r->fused_algo = sticky_algo(r->fused_algo, res, in.n, in.lead, tile_bytes, vcf, no_index);
        TRACE("wait(h2d) + scan", t_scan);
        trace_at("N scan result", r->n_batches);
        const JudgeState s = {r->mem_cap != 0, r->ws_full, r->worst_case_rows, no_store, r->shard_first, in.eof, in.range_end,
                              r->file_pos - in.shard_halo <= r->data_base};
        return judge_batch(res.flags, res.n_records, res.error_code, s);
    }
    // The record that ends behind the cut begins in front of the halo (a long read, a very wide VCF line): it belongs
    // to this shard, so this shard looks further back — eight times as far, up to the first byte of the data — and
    // scans the batch again.  (The shard in front leaves the record alone: it ends behind ITS range.)
    int look_further_back() {
        RD_HIP(r, hipStreamSynchronize(r->stream));
        r->halo_want = grow_halo(r->halo_want);
        if (!r->src) return EXG_OK;
        // a decoded stream begins with its halo: its members / frames are chosen again
        r->src.reset();
        r->file_idx--;
        return open_next_file(r);
    }
    // the same batch again with larger device buffers (ensure_device provisions them: `flag` says which)
    int provision_again(bool *flag) {
        RD_HIP(r, hipStreamSynchronize(r->stream));
        r->free_device();
        *flag = true;
        return EXG_OK;
    }

    // ---- 7: rows where the predicate is TRUE -> row map; the columns are gathered through it on their way out.  GTF: the rows
    // that are feature lines (d_keep), ANDed with the predicate when there is one.  A region reader: the rows that overlap the region
    // (d_keep, written here by exg_vcf_region_keep), ANDed likewise
    bool rows_skipped() const { return r->format == EXG_FMT_GTF && (res.flags & EXG_RF_ROWS_SKIPPED); }
    bool keep_words() const { return rows_skipped() || r->region; }
    int select_rows() {
        if (r->region)
            if (int rc = region_keep(r, in.d_input, (uint64_t)(uintptr_t)in.h, k, (uint64_t *)r->d_keep)) return rc;
        exg::arrow::FilterCols fc;
        memset(&fc, 0, sizeof fc);
        for (int c = 0; c < format_desc(r->format).n_columns; c++) {  // a text format's strings point into the input
            fc.d_base[c] = (const uint8_t *)in.d_input;
            fc.payload_base[c] = (uint64_t)(uintptr_t)in.h;
        }
        if (r->format == EXG_FMT_FASTA) {  // its sequences are the joined payload, not the input
            fc.d_base[2] = (const uint8_t *)r->d_payload;
            fc.payload_base[2] = (uint64_t)(uintptr_t)(in.b ? in.b->payload : nullptr);
        }
        return exg_rd::select_rows(r, &fc, keep_words() ? (const uint64_t *)r->d_keep : nullptr, &k, &row_map);
    }

    // ---- 8: the rows leave.  new_reader: the columns stay in HBM and become Arrow buffers there (exg_arrow_stream.cpp)
    ScanCtx scan_ctx() const { return ScanCtx{in.d_input, in.h, k, res, in.b ? (const uint8_t *)in.b->payload : nullptr}; }
    int arrow_emit() {
        const double t_emit = now_s();
        if (k)
            if (int rc = r->arrow_emit(r, scan_ctx())) return rc;
        TRACE("arrow emit", t_emit);
        return EXG_OK;
    }
    // ... or the batch's host vectors (exg_rd_rows_out.cpp)
    int columns_to_host() { return RowsOut{in, r, scan_ctx(), row_map}.columns_to_host(); }

    // ---- 9: the position behind the batch
    void commit_position() {
        r->shard_first = false;
        if (res.error_code || in.eof) {
            r->file_done = true;
        } else {
            r->file_pos += res.consumed_bytes - in.lead;
            if (in.range_end) r->file_done = true;  // what is left belongs to the next shard, whose halo reaches back to where that record begins
        }
    }
};

}  // namespace

// Scan the next device batch of the current file.  On return r->batch holds its host vectors
// (n_rows may be 0 when the file is exhausted).  count_only: no column leaves the device.
int next_batch(exg_reader *r, bool count_only, uint64_t *n_records_out) {
    *n_records_out = 0;
    r->batch.reset();
    r->batch_row = 0;
    if (int trc = truncated_while_read(r)) return trc;
    if (r->file_done) return EXG_OK;  // (opening the file found nothing of this shard's in it)
    if (r->format == EXG_FMT_BAM) return bam_next_batch(r, count_only, n_records_out);
    BatchRun run(r, count_only);
    const BatchIn &in = run.in;
    const double t_batch = now_s();
    for (;;) {
        int rc;
        run.size_attempt();
        if (in.n && r->src && (rc = run.acquire_segment())) return rc;
        if (!in.n) {
            r->file_done = true;
            return EXG_OK;
        }
        if ((rc = ensure_device(r, in.n + in.shard_halo + 16))) return rc;
        if ((rc = run.bind_input())) return rc;
        if ((rc = run.fastq_first_line_phase())) return rc;
        TraceRange scan_range(format_desc(r->format).scan_label);
        if ((rc = run.scan())) return rc;
        switch (run.judge()) {  // (the only place that scans the batch again)
            case kAccept: break;
            case kRetryHalo:
                if ((rc = run.look_further_back())) return rc;
                continue;
            case kRetryFullWorkspace:
                if ((rc = run.provision_again(&r->ws_full))) return rc;
                continue;
            case kRetryWorstCaseRows:
                if ((rc = run.provision_again(&r->worst_case_rows))) return rc;
                continue;
            case kWiden: run.want *= 2; continue;
            case kFailIndexOverflow: return fail(r, EXG_E_CAPACITY, "line index overflow in the general path (pathological line density)");
            case kFailCapacity: return fail(r, EXG_E_CAPACITY, "more rows than bytes allow: internal error");
        }
        if (run.res.error_code) {
            r->pending_error = run.res.error_code;
            r->pending_error_offset = r->file_pos - in.lead + run.res.error_offset;
        }
        const double t_pf = now_s();
        run.prefetch_next();
        TRACE("prefetch issue", t_pf);
        run.k = run.res.n_records;
        if ((r->has_filter || run.keep_words()) && run.k && !r->arrow_emit && (rc = run.select_rows())) return rc;
        *n_records_out = run.k;
        if (r->arrow_emit && !count_only) rc = run.arrow_emit();
        else rc = run.k && !count_only ? run.columns_to_host() : EXG_OK;
        if (rc) return rc;
        run.commit_position();
        TRACE("batch (h2d+scan+d2h)", t_batch);
        if (trace_on())
            fprintf(stderr, "[exg] device bytes held: %.2f MiB now, %.2f MiB at the peak (batch of %llu bytes, %llu rows)\n", r->meter.cur.load() / 1048576.0,
                    r->meter.peak.load() / 1048576.0, (unsigned long long)in.n, (unsigned long long)run.k);
        return EXG_OK;
    }
}

}  // namespace exg_rd
