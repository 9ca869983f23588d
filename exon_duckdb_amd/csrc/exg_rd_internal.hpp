// exg_rd_internal.hpp — what the translation units of the reader level share (not part of any ABI):
//   exg_rd_io.cpp      pinned blocks, NUMA pinning, page cache -> pinned -> HBM uploads, the reader's device buffers
//   exg_rd_bgzf.cpp    host only: the BGZF / gzip member walk (no HIP call; under ASan in tests/host_asan_driver.cpp)
//   exg_rd_plan.cpp    host only: compression inference, shard planning, replacement_scan
//   exg_rd_source.cpp  compressed inputs as a bounded stream of decoded segments in HBM (DecodedSource), and what the
//                      producers of such a stream share (exg_rd_source.hpp)
//   exg_rd_gzip.cpp    the gzip / BGZF producer;  exg_rd_zstd.cpp  the zstd producer;  exg_rd_bzip2.cpp  the bzip2 producer
//   exg_zstd_index.cpp host only: the zstd frame / block walk and a round's block list (no HIP call; under ASan as above)
//   exg_rd_fanout.cpp  host only: stripes of one input read by worker threads on N devices (exg_rd_fanout.hpp)
//   exg_rd_open.cpp    open_next_file: the mapping or the decoded stream, its header prefix, the shard's place in the file
//   exg_rd_batch.cpp   next_batch: one device batch from the input to the scan's verdict, as a driver over named stages
//   exg_rd_rows_out.cpp  the rows' way out: row selection, the side buffer, the columns -> the batch's host vectors (RowsOut);
//                      what exg_rd_bam.cpp shares of it
//   exg_rd_bam.cpp     read_bam_file_records: the header, and a batch loop of its own in front of the shared way out
//   exg_rd_stages.hpp  host only: the stages' decisions that make no HIP call — attempt size and halo, the upload window, what a
//                      scan's result means, the loop that reads a header's prefix (under ASan as above)
//   exg_reader.cpp     the C entry points (exg_open ... exg_close) and the chunk slicing
#pragma once
#include <stdio.h>
#include <time.h>

#include <condition_variable>
#include <mutex>
#include <string>
#include <vector>

#include "exg_reader.hpp"

namespace exg::arrow {
struct FilterCols;  // exg_arrow.hpp
}
namespace exg_rd {

struct HostMirror;  // exg_rd_source.hpp

#define RD_HIP(r, expr)                                                                            \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return ::exg_rd::fail(r, EXG_E_HIP, std::string(#expr " failed: ") + hipGetErrorString(_e)); \
    } while (0)

inline double now_s() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + ts.tv_nsec * 1e-9;
}
inline bool trace_on() {
    static int on = getenv("EXG_TRACE") ? 1 : 0;
    return on;
}
#define TRACE(label, t0)                                                            \
    do {                                                                            \
        if (::exg_rd::trace_on()) fprintf(stderr, "[exg] %-22s %.1f ms\n", label, (::exg_rd::now_s() - (t0)) * 1e3); \
    } while (0)

// EXG_TRACE=2: absolute timestamps (ms since the process's first such line) of the producer's and the consumer's steps, one
// line each — what a pipeline's bubbles are read from
inline void trace_at(const char *what, uint64_t idx) {
    static const int lvl = getenv("EXG_TRACE") ? atoi(getenv("EXG_TRACE")) : 0;
    if (lvl < 2) return;
    static const double t0 = now_s();
    fprintf(stderr, "[exg@] %9.2f %s %llu\n", (now_s() - t0) * 1e3, what, (unsigned long long)idx);
}

// roctx ranges around the reader's stages (upload, inflate / decode, scan, columns back) so that a rocprofiler timeline
// (rocprofv3 --marker-trace) of a query is readable (the reference has no tracing of its own).  The marker
// library is looked up at run time (librocprofiler-sdk-roctx.so, ROCm's): the product does not link against a profiler; without
// it — or without EXG_ROCTX=1 — a range costs one predictable branch.
struct RoctxApi {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
};
const RoctxApi &roctx_api();  // exg_rd_io.cpp
struct TraceRange {
    bool on;
    explicit TraceRange(const char *name) : on(roctx_api().push != nullptr) {
        if (on) (void)roctx_api().push(name);
    }
    ~TraceRange() {
        if (on) (void)roctx_api().pop();
    }
    TraceRange(const TraceRange &) = delete;
    TraceRange &operator=(const TraceRange &) = delete;
};

// a device buffer from the pool for the length of a scope. The stream that used it is waited for before the block goes
// back (idle already on the normal path; an error return may leave work in flight, and the pool is process-wide)
struct PoolBuf {
    int dev;
    hipStream_t stream;
    void *p = nullptr;
    size_t sz = 0;
    PoolBuf(int d, hipStream_t s) : dev(d), stream(s) {}
    PoolBuf(const PoolBuf &) = delete;
    PoolBuf &operator=(const PoolBuf &) = delete;
    void *take(size_t bytes) {
        release();
        sz = bytes ? bytes : 16;
        return p = dev_pool()->take(dev, sz);
    }
    void *detach() {  // the caller owns the block from here on (it goes back with dev_pool()->give(dev, p, sz))
        void *q = p;
        p = nullptr;
        return q;
    }
    void release() {
        if (!p) return;
        (void)hipStreamSynchronize(stream);
        dev_pool()->give(dev, p, sz);
        p = nullptr;
    }
    ~PoolBuf() { release(); }
};
struct SideScratch {  // pooled device scratch of one batch's side buffer (next_batch: the compact payload route)
    int dev;
    hipStream_t st;
    std::vector<std::pair<void *, size_t>> blocks;
    void *take(size_t n) {
        void *p = dev_pool()->take(dev, n);
        if (p) blocks.emplace_back(p, n);
        return p;
    }
    ~SideScratch() {
        if (!blocks.empty()) (void)hipStreamSynchronize(st);  // (an early return: kernels may still read them)
        for (auto &bl : blocks) dev_pool()->give(dev, bl.first, bl.second);
    }
};
// (whatever way next_batch's columns -> host is left once copies are on the columns' stream: they have landed — or the batch
// carries the event that says when — before its pinned blocks can go back to the pool)
struct ColDrain {
    hipStream_t cs = nullptr;
    ~ColDrain() {
        if (cs) (void)hipStreamSynchronize(cs);
    }
};

// bytes in front of a shard that travel with its first batch (the beginning of the record that ends behind the cut);
// grown by the reader when the record turns out to begin further back
static constexpr uint64_t kShardHalo = 1u << 20;
// The next batch starts where this one's last complete record ends - known only after the scan - so the
// prefetch starts this many bytes before the end of the current batch; a batch whose unconsumed tail is
// longer (one giant record) falls back to the synchronous upload.
static constexpr uint64_t kPrefetchSlack = 1u << 20;
static constexpr uint64_t kRampFirstBytes = 32u << 20;  // the first device batch of a text file (exg_reader.hpp: ramp_bytes)
static constexpr size_t kUploadWindow = 256u << 20;

// ---- exg_rd_io.cpp
void pin_to_device_node(int device);
int list_files(exg_reader *r, const std::string &path);
// a consumer that follows an upload window by window (events recorded on the upload's stream)
struct UploadProgress {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<hipEvent_t> done;  // one per window, created by the consumer
    size_t recorded = 0;
    bool finished = false;
    int rc = 0;
    // window w has been enqueued (true) / the upload ended without it (false)
    bool wait_for(size_t w) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return recorded > w || finished; });
        return recorded > w;
    }
};
// file bytes [file_off, file_off + n) -> d_dst on `st` (NULL: r->stream): windows of 256 MiB through two pooled pinned
// blocks, each window read by parallel pread and sent slice by slice
int upload_file(exg_reader *r, void *d_dst, uint64_t n, uint64_t file_off = 0, hipStream_t st = nullptr, UploadProgress *prog = nullptr);
// the same without a reader (a decoder thread: errors go to *err, not to the reader's message)
int upload_fd(int device, int fd, void *d_dst, uint64_t n, uint64_t file_off, hipStream_t st, UploadProgress *prog, std::string *err);
// file bytes [off, off + n) -> the slot's pinned bounce buffer (parallel pread) -> d_in_slot[slot], on `st`
int upload_range(exg_reader *r, uint64_t off, uint64_t n, int slot, hipStream_t st);
// the same on a host thread of its own (pread + the H2D enqueue block their caller for as long as the bytes take to leave)
void start_upload(exg_reader *r, exg_reader::Prefetch *which, uint64_t start, uint64_t len, int slot);
// fd bytes [off, off + n) -> host memory `dst` by up to 8 threads pinned to the device's NUMA node; when d_dst != NULL every
// slice is sent on to d_dst + (its offset) on `st` as soon as it has been read.  false: short read (*hip_failed: a copy failed)
bool pread_parallel(int device, int fd, uint64_t off, size_t n, char *dst, char *d_dst, hipStream_t st, bool *hip_failed);
// Column c of a batch's k rows -> pinned vectors of `b` on `st`: its values (d_col, `es` = 4, 8 or 16 bytes each; NULL: none)
// and its validity bits (d_valid; NULL: none), each gathered through row_map into d_gather first when there is one
int column_to_host(exg_reader *r, Batch *b, int c, const void *d_col, uint32_t es, const void *d_valid, uint64_t k, const uint32_t *row_map,
                   void *d_gather, hipStream_t st);

// ---- exg_rd_bgzf.cpp (host only)
// The few bytes the BGZF walk looks at — a member's header, the trailer right in front of the next header — read with pread
// into a small window, NOT through the file's mapping: a fault on the mapping maps sixteen pages (fault-around), two faults
// per 18 KB member map the whole file, and unmapping a 5 GB file that had been mapped that way cost 80-120 ms (page-table
// teardown, TLB shootdowns on a 256-thread host) behind a 300 ms decode; the walk itself was page-fault bound (35-55 ms
// per 5 GB on eight threads).  fd < 0: the bytes are in memory at `map`.
struct Peek {
    const uint8_t *map;
    int fd;
    uint64_t n;
    uint8_t buf[512];
    uint64_t b0 = ~0ull, b1 = 0;  // buf holds file bytes [b0, b1)
    Peek(const uint8_t *m, int f, uint64_t size) : map(m), fd(f), n(size) {}
    const uint8_t *at(uint64_t off, size_t len);  // file bytes [off, off + len), len <= 256; nullptr past the end of the file
};
uint64_t bgzf_member_at(Peek &f, uint64_t pos, exg_inflate_member *m, uint32_t *crc = nullptr);
uint64_t bgzf_find(const uint8_t *d, int fd, uint64_t n, uint64_t from);
bool bgzf_parallel_index(const uint8_t *d, int fd, uint64_t n, exg_inflate_member *members, uint64_t cap, uint64_t *k_out, uint64_t *total_out,
                         std::vector<uint32_t> *crc_out, uint64_t upto = ~0ull);

// ---- exg_rd_plan.cpp (host only)
bool parse_compression(const std::string &s, Compression *out);
Compression compression_of(const exg_open_args *args);


struct Stripe;
int list_path(const std::string &path, std::vector<std::string> *files, std::string *err);
int plan_stripes(const std::vector<std::string> &files, Compression compression, const exg_open_args *args, std::vector<Stripe> *out, unsigned *n_workers);

// The A/B switches of the reader level, read once per process.  (EXG_NO_VCF_INDEX and EXG_VCF_ONE_STREAM are not here: they are read
// per batch, where they are used — the tests switch them inside one process.)
struct Switches {
    const bool fasta_whole_text = getenv("EXG_FASTA_WHOLE_TEXT") != nullptr;      // a decoded FASTA: the decoded text behind the scan, no side buffer
    const bool no_payload_compact = getenv("EXG_NO_PAYLOAD_COMPACT") != nullptr;  // a projection of a decoded input: no side buffer
    const bool no_host_mirror = getenv("EXG_NO_HOST_MIRROR") != nullptr;          // (and tests) a decoded input: the copy behind the scan
    const bool no_ramp = getenv("EXG_NO_RAMP") != nullptr;                        // a text file's first batch is a full one
    const bool no_fasta_prefetch = getenv("EXG_NO_FASTA_PREFETCH") != nullptr;    // FASTA: one input slot, no upload beside the way back
    const bool no_prefetch = getenv("EXG_NO_PREFETCH") != nullptr;                // no upload ahead of the scan
    const bool fastq_one_stream = getenv("EXG_FASTQ_ONE_STREAM") != nullptr;      // a text FASTQ's vectors on the scan's stream
    const bool vcf_eager_landing = getenv("EXG_VCF_EAGER_LANDING") != nullptr;    // read_vcf waits for its vectors inside next_batch
    const bool fasta_d2h_engine = getenv("EXG_FASTA_D2H_ENGINE") != nullptr;      // FASTA: the joined sequences by a copy engine
};
inline const Switches &switches() {
    static const Switches s;
    return s;
}

// One word from a kernel: `launch(d_word)` enqueues on r->stream what writes a u32 / u64 to d_word (the reader's d_phase, taken
// when first needed) and returns an EXG code; the word comes back into *out and the stream is idle on return.
template <class Word, class Launch>
int fetch_word(exg_reader *r, Word *out, Launch launch) {
    static_assert(sizeof(Word) == 4 || sizeof(Word) == 8, "a device word is 4 or 8 bytes");
    if (!r->d_phase && !(r->d_phase = dev_pool()->take(r->device, 4096))) return fail(r, EXG_E_HIP, "out of device memory");
    if (int rc = launch(r->d_phase)) return fail(r, rc, exg_last_error_message());
    RD_HIP(r, hipMemcpyAsync(out, r->d_phase, sizeof(Word), hipMemcpyDeviceToHost, r->stream));
    RD_HIP(r, hipStreamSynchronize(r->stream));
    return EXG_OK;
}

// ---- exg_rd_open.cpp (open_next_file: exg_reader.hpp)
// How the bytes a decoded input's strings point into reach the host when chunks are handed out (never for COUNT(*) or the Arrow
// stream): kPayloadCompact — a projection that leaves payload-bearing columns out: the selected columns' out-of-line strings are
// closed up into a side buffer behind the scan; kPayloadMirror — the decoded segments themselves, sent ahead by the producer
// (HostMirror; a segment without one is copied behind its scan); kPayloadNone — no string column is selected.  FASTA (round 6):
// always the side buffer for id / description — its sequences are joined on the device and travel as that, so the decoded text is
// needed for the definition lines' strings alone, 2 % of it (the whole text went along until then: a bgzip FASTA into DataChunks
// sent every byte back twice, 92 ms for 1.96 GB).
enum PayloadRoute { kPayloadNone, kPayloadCompact, kPayloadMirror };
PayloadRoute payload_route(const exg_reader *r);
// Newlines in the decoded bytes of the members / frames in front of a shard's own (file bytes [0, own_c_begin)), by a decoder
// of their own: a segment is counted on the device and dropped, nothing but it is resident (the phase of a shard of a
// compressed FASTQ when the bytes around the cut do not tell it: a memchr over the page cache in the text case).
int count_newlines_in_front(exg_reader *r, uint64_t *out);

// ---- exg_rd_batch.cpp
// the reader's vectors of the columns in `produce` (bit c: schema column c), for r->cap_records rows (the reader's dev_alloc)
int alloc_columns(exg_reader *r, uint64_t produce);
// the next device batch with rows -> r->batch (false + *end: every file is exhausted); what exg_next_chunk and a fan-out
// worker both do between two batches: pending parse errors, the end of a file, the next file
int advance_batch(exg_reader *r, bool *end);
// the mapping of the current file lost pages to a truncation (exg_map_guard.hpp): EXG_E_IO
int truncated_while_read(exg_reader *r);

// ---- exg_rd_rows_out.cpp: the rows' way out of a scanned batch (chunk boundary)
// Rows where the predicate is TRUE — and whose bit in d_keep is set, when there are keep words — -> the reader's row map; the
// columns are gathered through it on their way out.  The caller says where each column's strings live (fc->d_base, fc->payload_base);
// kinds, data and validity come from the format table and the reader's column vectors.  *k: the scan's rows in, the rows that leave out.
int select_rows(exg_reader *r, exg::arrow::FilterCols *fc, const uint64_t *d_keep, uint64_t *k, const uint32_t **row_map);
// ... and its buffers, for r->cap_records rows (the reader's dev_alloc): the row map, one column of gather scratch, the scan's scratch
int alloc_row_selection(exg_reader *r);
struct SideBuf;
// The flat columns the projection wants -> b, each with its validity words, gathered through the row map and copied back on `cs`
// (side: the compact route's side buffer, whose string columns are repointed first; NULL: none)
int flat_columns_to_host(exg_reader *r, Batch *b, uint64_t k, const uint32_t *row_map, hipStream_t cs, const SideBuf *side);
// the batch is whole (or carries the event that says when): it becomes r->batch
void publish_batch(exg_reader *r, const std::shared_ptr<Batch> &b);
// What the way out reads of one attempt at a batch (the rest of it — BatchIn, exg_rd_batch.cpp — is the input half's alone)
struct BatchOut {
    uint64_t n = 0;          // bytes of the attempt: behind file_pos until the input is bound, then all the scan is given (`lead` included)
    uint64_t batch_end = 0;  // file offset one past the bytes of this batch
    std::shared_ptr<PinnedBlock> gz_payload;  // gzip: this batch's inflated bytes on the host (string_t payload)
    std::shared_ptr<HostMirror> gz_mirror;    // ... when the producer sent them ahead (exg_rd_source.hpp); then only
    uint64_t gz_front = 0;                    // ... the first gz_front bytes of the batch (the carried tail) are copied here
    bool compact = false;                     // ... or: only the selected columns' out-of-line strings travel (a side buffer)
    std::shared_ptr<Batch> b;  // FASTA: made in front of the scan (its pinned block takes the joined sequences); else by columns_to_host
};
// The way out of a text format's batch, and everything it depends on: that of the attempt, the reader, what the scan left in HBM
// and the rows that leave.  BAM has no use for it: its side buffer is the scan's own and travels whole (exg_rd_bam.cpp).
struct RowsOut : BatchOut {
    exg_reader *r;
    ScanCtx scan;             // d_input, h, the rows that leave (n_records), the scan's result, FASTA's payload base
    const uint32_t *row_map;  // NULL: every row of the scan leaves
    int columns_to_host();                    // -> r->batch

private:
    int side_buffer(SideBuf *side, SideScratch *scratch);
    int columns_stream(hipStream_t *cs, ColDrain *col_drain);
    int vcf_nested_columns(hipStream_t cs, ColDrain *col_drain);
    int gtf_attributes(SideScratch *scratch);
    int fasta_sequences(hipStream_t cs);
};

}  // namespace exg_rd
