// exg_rd_stages.hpp — the decisions of next_batch (exg_rd_batch.cpp) that make no HIP call: how large an attempt is and how
// far its halo reaches back, which file bytes the next upload carries, what a scan's result means for the attempt; and the loop
// that reads a header from the front of a decoded stream (exg_rd_open.cpp, exg_rd_bam.cpp, exg_rd_bcf.cpp).  Host
// only and free of any HIP include: under ASan + UBSan in tests/host_asan_driver.cpp.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "../../include/exon_gpu.h"

namespace exg_rd {

// ---- stage 1: the size of an attempt ------------------------------------------------------------------------------------
struct AttemptSize {
    uint64_t n;           // bytes behind file_pos (0: nothing of this reader's is left)
    bool range_end, eof;  // the batch reaches the end of this reader's bytes ... which is the end of the file unless a later shard follows
    uint64_t shard_halo;  // bytes in front of file_pos that travel along
};
// first batch of a shard that begins inside the file: up to `halo_want` bytes in front of it travel along, so that
// the record / line that ends behind the cut — it belongs to this shard — has its beginning in the buffer
// (a buffer that already lives in HBM — a decoded stream — must be entered at a 16-byte boundary: a few bytes of the header's
// last line may then come along in front — they end inside the halo and are nobody's rows)
inline uint64_t shard_halo_bytes(uint64_t file_pos, uint64_t data_base, uint64_t halo_want, bool decoded) {
    const uint64_t from = file_pos - std::min<uint64_t>(halo_want, file_pos - data_base);
    return file_pos - (decoded ? (std::max<uint64_t>(data_base, from) & ~15ull) : std::max<uint64_t>(data_base, from & ~15ull));
}
// eight times as far, up to everything (saturates: a halo above ~0 >> 4 does not wrap)
inline uint64_t grow_halo(uint64_t halo_want) { return halo_want > (~0ull >> 4) ? ~0ull : halo_want * 8; }
// ramp_step: the head of a text file takes a small batch first (~0: no ramp applies to this attempt)
inline AttemptSize size_attempt(uint64_t want, uint64_t file_pos, uint64_t range_hi, bool range_eof, uint64_t ramp_step, bool shard_first,
                                uint64_t data_base, uint64_t halo_want, bool decoded) {
    AttemptSize a = {0, false, false, 0};
    const uint64_t remaining = range_hi > file_pos ? range_hi - file_pos : 0;
    if (remaining == 0) return a;
    a.n = std::min<uint64_t>(std::min<uint64_t>(want, remaining), ramp_step);
    a.range_end = a.n == remaining;
    a.eof = a.range_end && range_eof;
    if (shard_first) a.shard_halo = shard_halo_bytes(file_pos, data_base, halo_want, decoded);
    return a;
}

// ---- the file bytes an upload ahead carries ---------------------------------------------------------------------------------
// The next batch starts where this one's last complete record ends — known only after the scan — so its upload starts `slack`
// bytes in front of the end of this batch's bytes [begin, end), at a 16-byte boundary.  FASTA: the scan wants its batch at a
// 16-byte boundary with nothing in front, and the upload is issued when the scan has said where the next record begins
// (fasta_next; ~0: not FASTA): exactly there, no slack.
struct PrefetchWindow {
    uint64_t start, slack;
    // step: what the ramp gives the next upload.  0: no upload (it would not fit an input slot)
    uint64_t len(uint64_t range_hi, uint64_t step, uint64_t d_in_cap) const {
        const uint64_t l = std::min<uint64_t>(range_hi - start, step + slack);
        return l + 16 <= d_in_cap ? l : 0;
    }
};
inline PrefetchWindow prefetch_window(uint64_t begin, uint64_t end, uint64_t max_slack, uint64_t fasta_next = ~0ull) {
    if (fasta_next != ~0ull) return {fasta_next, 0};
    const uint64_t slack = std::min<uint64_t>(max_slack, (end - begin) / 2);
    return {(end - slack) & ~15ull, slack};
}

// ---- a header at the front of a decoded stream ----------------------------------------------------------------------------------
// A growing prefix of the stream comes to the host until a parser is satisfied (the VCF / SAM header lines, the BAM and the BCF
// header).  `front(want, &avail, &eof)` brings min(want, avail) bytes of the stream's front to the host (avail: what the stream
// holds from its first byte on, eof: it ends there) and returns an error code or 0.  `inspect(len, ended, &need)` looks at those
// len bytes — ended: the stream ends with them, there will be no more — and answers kPrefixDone, kPrefixMore (need: how many
// bytes it knows it wants, 0 when it cannot tell) or an error code (negative, EXG_E_*: the reason is the caller's to keep).
// `grow(want, need)` is the next size to ask for.  What the first error says, and to whom, is the callables' business.
enum { kPrefixDone = 0, kPrefixMore = 1 };
template <class Front, class Inspect, class Grow>
int read_prefix(uint64_t first, Front front, Inspect inspect, Grow grow) {
    for (uint64_t want = first;;) {
        uint64_t avail = 0, need = 0;
        bool eof = false;
        if (int rc = front(want, &avail, &eof)) return rc;
        const uint64_t len = std::min<uint64_t>(want, avail);
        const int answer = inspect(len, eof && len == avail, &need);
        if (answer != kPrefixMore) return answer;
        want = grow(want, need);
    }
}
// the growth rules: text headers (lines: the parser cannot say how much it needs) and the binary ones (it can)
inline uint64_t prefix_grow_times8(uint64_t want, uint64_t) { return want * 8; }
inline uint64_t prefix_grow_need_or_double(uint64_t want, uint64_t need) { return std::max<uint64_t>(need, want * 2); }

// ---- stage 6: what a scan's result means for the attempt --------------------------------------------------------------------
enum BatchVerdict {
    kAccept,
    kRetryHalo,           // the record that ends behind the cut begins in front of the halo: look further back, same batch again
    kRetryFullWorkspace,  // denser lines than the budgeted workspace indexes: the full one, same batch again
    kRetryWorstCaseRows,  // denser rows than provisioned: worst-case vectors, same batch again
    kWiden,               // not even one complete record in the batch: widen it
    kFailIndexOverflow,
    kFailCapacity,
};
struct JudgeState {
    bool mem_cap, ws_full, worst_case_rows, no_store, shard_first, eof, range_end;
    bool halo_at_base;  // the halo already begins with the first byte of the data
};
// precedence: head unresolved, index overflow, capacity, widen
inline BatchVerdict judge_batch(uint32_t flags, uint64_t n_records, uint32_t error_code, const JudgeState &s) {
    if (s.shard_first && (flags & EXG_RF_HEAD_UNRESOLVED) && !s.halo_at_base) return kRetryHalo;
    if (flags & EXG_RF_INDEX_OVERFLOW) return s.mem_cap && !s.ws_full ? kRetryFullWorkspace : kFailIndexOverflow;
    if ((flags & EXG_RF_CAPACITY) && !s.no_store) return s.worst_case_rows ? kFailCapacity : kRetryWorstCaseRows;
    if (n_records == 0 && !error_code && !s.eof && !s.range_end) return kWiden;
    return kAccept;
}

// Which scan the next batch starts with, from this one's result (sticky: exg_reader.hpp fused_algo).  n: the scanned bytes, `lead`
// of them in front of the batch's own; tile_bytes: a super-tile of the lean scan
inline uint32_t sticky_algo(uint32_t algo, const exg_scan_result &res, uint64_t n, uint64_t lead, uint64_t tile_bytes, bool vcf, bool no_vcf_index) {
    // sticky (exg_reader.hpp) — when the marks are the input's shape: more than an eighth of the batch's super-tiles.  The
    // odd long read in a short-read file is cheaper redone (its tiles only) than paid for by the any-shape scan's ~20 % on
    // every batch behind it
    if ((res.flags & EXG_RF_REDO) && res.redo_tiles * 8 > n / tile_bytes) algo = EXG_ALGO_FUSED_FULL;
    if (vcf && res.n_lines) {
        // the any-shape scan on WIDE lines (cohort VCFs) leaves the rows to a kernel of their own (EXG_ALGO_FUSED_INDEX: exg_vcf.hip):
        // measured over line widths (tools/vcf_index_crossover.py, TB/s indexed against rows inside): level at 483 B a line, 2.72
        // against 2.21 at 882 B, 3.13 against 2.15 at 1.7 kB, 3.82 against 2.28 at 10 kB — the switch at an average of 640 B;
        // sticky both ways with a gap between the thresholds (EXG_NO_VCF_INDEX: never — A/B)
        const uint64_t per_line = (n - lead) / res.n_lines;
        if (algo == EXG_ALGO_FUSED_FULL && per_line >= 640 && !no_vcf_index) algo = EXG_ALGO_FUSED_INDEX;
        else if (algo == EXG_ALGO_FUSED_INDEX && per_line < 448) algo = EXG_ALGO_FUSED_FULL;
    }
    return algo;
}

}  // namespace exg_rd
