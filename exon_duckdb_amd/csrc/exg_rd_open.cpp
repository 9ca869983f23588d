// exg_rd_open.cpp — reader level: a file is opened.  A text file is mapped (the DataChunk strings point into the mapping); a
// compressed one is handed to a decoder and becomes a bounded stream of decoded segments in HBM (exg_rd_source.hpp), of which
// the header's prefix comes back to the host.  Then the reader's place in the file: the header's end, and for a shard the bytes
// (or the members / frames) that are its own and the halo in front of them.  Replaces the opening half of exon's
// BatchReader behind the stream `new_reader` returns (rust/src/arrow_reader.rs:116-153); the batches are exg_rd_batch.cpp's.
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <memory>

#include "exg_map_guard.hpp"
#include "exg_rd_bam.hpp"
#include "exg_rd_region.hpp"
#include "exg_rd_source.hpp"
#include "exg_rd_stages.hpp"
#include "exg_sam_header.hpp"

namespace exg_rd {

// ---- compressed inputs: the file becomes a stream of decoded segments (exg_rd_source.hpp) --------------------------------

// room every segment leaves in front of its bytes for the tail the scan carries over (a longer tail moves into a block of its own)
static uint64_t source_reserve(const exg_reader *r) { return std::min<uint64_t>(std::max<uint64_t>(r->device_batch_bytes / 8, 64u << 10), 8u << 20); }

// the formats whose text begins with a header, and the byte its lines begin with (VCF: parsed; SAM: only skipped)
static bool has_text_header(const exg_reader *r) { return r->format == EXG_FMT_VCF || r->format == EXG_FMT_SAM; }
static char header_marker(const exg_reader *r) { return r->format == EXG_FMT_SAM ? '@' : '#'; }

// The leading '#' lines of a decoded VCF ('@' lines of a SAM) come back to the host for the header parse (blk->p holds a prefix
// of the decoded stream; the DataChunk payload travels per batch): `src` is read from its first byte until a line that does
// not start with the marker begins inside the prefix, or the stream ends.
static int source_header_prefix(exg_reader *r, DecodedSource *src, PinnedBlock &b) {
    auto front = [&](uint64_t want, uint64_t *avail, bool *eof) {
        const uint8_t *d_at = nullptr;
        std::string msg;
        int rc = src->acquire(0, want, &d_at, avail, eof, &msg);
        if (rc) return fail(r, rc, msg);
        const size_t len = (size_t)std::min<uint64_t>(want, *avail);
        if (b.p) global_pool()->give((char *)b.p, b.cap), b.p = nullptr;
        size_t cap = len + 64;
        b.p = global_pool()->take(&cap);
        if (!b.p) return fail(r, EXG_E_HIP, "out of pinned host memory for the VCF header");
        b.cap = cap;
        b.pooled = true;
        if (len) RD_HIP(r, hipMemcpyAsync(b.p, d_at, len, hipMemcpyDeviceToHost, r->stream));
        RD_HIP(r, hipStreamSynchronize(r->stream));
        return (int)EXG_OK;
    };
    auto inspect = [&](uint64_t len, bool ended, uint64_t *) {
        if (leading_lines_end((const char *)b.p, (size_t)len, header_marker(r)) >= len && !ended) return (int)kPrefixMore;
        r->gz_header_prefix = len;
        return (int)kPrefixDone;
    };
    // (not more than a device batch at first: what is acquired here is the first batch's size, which sizes the scan's buffers)
    return read_prefix(std::min<uint64_t>(4u << 20, r->device_batch_bytes), front, inspect, prefix_grow_times8);
}

// The first FASTA record start ('>' at the beginning of a line) of a decoded stream at or behind `from` (~0: none before the
// stream ends).  Everything from `from` on stays resident: the record that begins there is the next batch.
static int source_find_record(exg_reader *r, uint64_t from, uint64_t *found) {
    *found = ~0ull;
    const uint64_t base = from ? from - 1 : 0;  // (the byte in front says whether `from` begins a line)
    for (uint64_t want = r->device_batch_bytes;; want *= 2) {
        const uint8_t *d_at = nullptr;
        uint64_t avail = 0;
        bool eof = false;
        std::string msg;
        int rc = r->src->acquire(base, want, &d_at, &avail, &eof, &msg);
        if (rc) return fail(r, rc, msg);
        if (base + avail > from) {
            uint64_t pos = ~0ull;
            rc = fetch_word(r, &pos, [&](void *d_word) {
                return exg_fasta_find_record(d_at, from - base, avail, base == 0 && r->data0_is_line_start, (uint64_t *)d_word, r->stream);
            });
            if (rc) return rc;
            if (pos != ~0ull) {
                *found = base + pos;
                return EXG_OK;
            }
        }
        if (eof || avail < want) return EXG_OK;
    }
}

// Shard `shard_index` of `shard_count` of a BGZF file: a member belongs to the shard in whose 1/shard_count of the FILE's
// bytes its header begins.  The reader finds its members without indexing the file (a search for a header whose chain holds
// near each cut: the pointer chase over a whole file costs 110 ms per 10 GB and every rank would pay it) and streams
// [c_begin, c_end): ~1 MiB (inflated) of members in front of its own — the halo that holds the beginning of the record that
// ends behind the cut — then its own.  Positions of the reader are offsets in THAT stream.
static int plan_bgzf_shard(exg_reader *r, const std::string &path, uint64_t n, uint64_t *c_begin, uint64_t *c_end, uint64_t header_bytes) {
    const int fd = r->fd_keep->fd;
    Peek peek(nullptr, fd, n);
    exg_inflate_member probe;
    if (!bgzf_member_at(peek, 0, &probe))
        return fail(r, EXG_E_UNSUPPORTED, "shards of a gzip input need BGZF framing (every member carries its size): '" + path + "'");
    const uint64_t lo = (uint64_t)((unsigned __int128)n * r->shard_index / r->shard_count);
    const uint64_t hi = r->shard_index + 1 == r->shard_count ? n : (uint64_t)((unsigned __int128)n * (r->shard_index + 1) / r->shard_count);
    const uint64_t first_own = lo == 0 ? 0 : bgzf_find(nullptr, fd, n, lo);
    *c_end = hi >= n ? n : std::max<uint64_t>(first_own, bgzf_find(nullptr, fd, n, hi));
    // candidates for the halo: members that begin in the ~1.5 MiB of file in front of the cut (BGZF does not expand)
    std::vector<uint64_t> hdr, out;
    const uint64_t halo_want = r->halo_want;
    const uint64_t back = halo_want > n ? n : halo_want + (halo_want >> 1) + (128u << 10);
    for (uint64_t pos = first_own == 0 ? 0 : bgzf_find(nullptr, fd, n, lo > back ? lo - back : 0); pos < first_own;) {
        exg_inflate_member m;
        const uint64_t nx = bgzf_member_at(peek, pos, &m);
        if (!nx) return fail(r, EXG_E_PARSE, "not a BGZF member at byte " + std::to_string(pos) + " of '" + path + "'");
        hdr.push_back(pos);
        out.push_back(m.out_cap);
        pos = nx;
    }
    size_t h0 = hdr.size();
    uint64_t halo_bytes = 0;
    while (h0 > 0 && halo_bytes < halo_want) halo_bytes += out[--h0];
    *c_begin = h0 < hdr.size() ? hdr[h0] : first_own;
    // VCF: where do the members that hold the header end?  A halo that would begin among them is taken from the start of
    // the file instead, so that the end of the header is a known offset of this reader's stream
    if (header_bytes && *c_begin != 0) {
        uint64_t q = 0, sum = 0;
        while (q < n && sum < header_bytes) {
            exg_inflate_member m;
            const uint64_t nx = bgzf_member_at(peek, q, &m);
            if (!nx) return fail(r, EXG_E_PARSE, "not a BGZF member at byte " + std::to_string(q) + " of '" + path + "'");
            sum += m.out_cap;
            q = nx;
        }
        if (*c_begin < q) {  // q: compressed offset behind the header's members
            for (uint64_t pos = 0; pos < *c_begin;) {
                exg_inflate_member m;
                const uint64_t nx = bgzf_member_at(peek, pos, &m);
                if (!nx) return fail(r, EXG_E_PARSE, "not a BGZF member at byte " + std::to_string(pos) + " of '" + path + "'");
                halo_bytes += m.out_cap;
                pos = nx;
            }
            *c_begin = 0;
        }
    }
    if (*c_begin > *c_end) *c_begin = *c_end;
    // does any inflated byte follow this reader's members?  (the empty BGZF end marker — or a later shard that owns nothing
    // else — must not keep the shard with the file's last record from seeing the end of the file)
    bool bytes_follow = false;
    for (uint64_t q = *c_end; q < n && !bytes_follow;) {
        exg_inflate_member m;
        const uint64_t nx = bgzf_member_at(peek, q, &m);
        if (!nx) return fail(r, EXG_E_PARSE, "not a BGZF member at byte " + std::to_string(q) + " of '" + path + "'");
        bytes_follow = m.out_cap != 0;
        q = nx;
    }
    r->own_c_begin = first_own;
    r->range_preset = true;
    r->preset_pos = halo_bytes;  // inflated bytes of the members in front of its own
    r->range_eof = !bytes_follow;
    r->data0_is_line_start = *c_begin == 0;  // byte 0 of the stream begins a line only when the stream begins with the file
    return EXG_OK;
}

PayloadRoute payload_route(const exg_reader *r) {
    if (r->format == EXG_FMT_BAM) return kPayloadNone;  // (a BAM segment is never mirrored: its strings are produced into a side buffer)
    const FormatDesc &f = format_desc(r->format);
    const uint64_t strs = f.payload_mask(), sel = r->want_cols & strs;  // the columns whose strings point into the input
    if (r->format == EXG_FMT_FASTA) return sel && !switches().fasta_whole_text ? kPayloadCompact : kPayloadNone;
    if (!sel) return kPayloadNone;
    if (!switches().no_payload_compact && sel != strs && !(sel & f.nested_mask())) return kPayloadCompact;
    return switches().no_host_mirror ? kPayloadNone : kPayloadMirror;
}

static int open_source(exg_reader *r, std::shared_ptr<PinnedBlock> &blk, const std::string &path, uint64_t n) {
    const int fd = r->fd_keep->fd;
    const uint64_t reserve = source_reserve(r), target = r->device_batch_bytes;
    auto out_blk = std::make_shared<PinnedBlock>();  // (n = 0: the decoded size is not known; p: the VCF header prefix)
    r->gz_header_prefix = 0;
    const size_t queued = getenv("EXG_SOURCE_QUEUE") ? (size_t)std::max(1, atoi(getenv("EXG_SOURCE_QUEUE"))) : r->mem_cap ? 1 : 2;
    auto make = [&](uint64_t c_begin, uint64_t c_end, bool bgzf_only, const uint64_t *marks) {
        std::unique_ptr<SegmentProducer> prod = r->region ? make_region_producer(r, fd, n, target, path, reserve)  // (the header + the index's member ranges)
                                                : r->bcf  ? make_bcf_producer(r, make_gzip_producer(r, fd, c_begin, c_end, bcf_input_target(target), path, true, bcf_input_reserve(target), nullptr),
                                                                           bcf_input_reserve(target), target, path, reserve)  // (BGZF -> BCF records -> VCF text)
                                                : r->compression == kGzip  ? make_gzip_producer(r, fd, c_begin, c_end, target, path, bgzf_only, reserve, marks)
                                                : r->compression == kBzip2 ? make_bzip2_producer(r, fd, n, target, path, reserve)
                                                                           : make_zstd_producer(r, fd, n, c_begin, c_end, target, path, reserve, marks);
        // (EXG_OPEN_CHUNKS: the caller said it will pull chunks — the segments travel to the host from the first one on)
        const bool mirror0 = r->expect_chunks && !r->arrow_emit && payload_route(r) == kPayloadMirror;
        return std::unique_ptr<DecodedSource>(new DecodedSource(r->device, r->stream, std::move(prod), reserve, queued, &r->meter, mirror0));
    };
    if (r->compression == kGzip && n == 0) return fail(r, EXG_E_PARSE, "empty gzip file '" + path + "'");
    r->fa_shard = false;
    r->fa_end = ~0ull;
    if (r->shard_count > 1 && r->compression == kBzip2)
        return fail(r, EXG_E_UNSUPPORTED, "shards of a bzip2 input are not supported (one file is one shard): '" + path + "'");
    if (r->shard_count > 1) {
        // VCF: every rank needs the header (schema, and where the data begins): read from the start of the file by a
        // source of its own, kept on the host like in the unsharded case
        uint64_t header_bytes = 0;
        if (has_text_header(r)) {
            std::unique_ptr<DecodedSource> head = make(0, n, r->compression == kGzip, nullptr);
            int rc = source_header_prefix(r, head.get(), *out_blk);
            if (rc) return rc;
            header_bytes = leading_lines_end((const char *)out_blk->p, (size_t)r->gz_header_prefix, header_marker(r));
        }
        const bool fasta = r->format == EXG_FMT_FASTA;
        uint64_t c_begin = 0, c_end = n, marks[2] = {~0ull, ~0ull};
        bool wait_own = false;  // where the shard's own bytes begin is told by the decoder (mark 0)
        if (r->compression == kGzip && !fasta) {
            int rc = plan_bgzf_shard(r, path, n, &c_begin, &c_end, header_bytes);
            if (rc) return rc;
        } else if (r->compression == kGzip) {
            // bgzip FASTA: a record belongs to the shard in whose members' bytes its '>' line begins.  The stream starts one
            // member in front of the shard's own (is their first byte a line start?) and runs on behind them until the next
            // record start is found
            Peek peek(nullptr, fd, n);
            exg_inflate_member probe;
            if (!bgzf_member_at(peek, 0, &probe))
                return fail(r, EXG_E_UNSUPPORTED, "shards of a gzip input need BGZF framing (every member carries its size): '" + path + "'");
            const uint64_t lo = (uint64_t)((unsigned __int128)n * r->shard_index / r->shard_count);
            const uint64_t hi = r->shard_index + 1 == r->shard_count ? n : (uint64_t)((unsigned __int128)n * (r->shard_index + 1) / r->shard_count);
            const uint64_t own_lo = lo == 0 ? 0 : bgzf_find(nullptr, fd, n, lo);
            const uint64_t own_hi = hi >= n ? n : std::max<uint64_t>(own_lo, bgzf_find(nullptr, fd, n, hi));
            c_begin = own_lo;
            for (uint64_t pos = own_lo == 0 ? 0 : bgzf_find(nullptr, fd, n, own_lo > (192u << 10) ? own_lo - (192u << 10) : 0); pos < own_lo;) {
                exg_inflate_member m;
                const uint64_t nx = bgzf_member_at(peek, pos, &m);
                if (!nx) return fail(r, EXG_E_PARSE, "not a BGZF member at byte " + std::to_string(pos) + " of '" + path + "'");
                c_begin = pos;  // (the last member in front of the shard's own)
                pos = nx;
            }
            marks[0] = own_lo;
            marks[1] = own_hi >= n ? ~0ull : own_hi;
            wait_own = true;
        } else {
            uint64_t own_lo = 0, own_hi = n;
            bool bytes_follow = false;
            int rc = plan_zstd_shard(r, fd, n, path, fasta ? 1 : r->halo_want, header_bytes, &c_begin, &c_end, &own_lo, &own_hi, &bytes_follow);
            if (rc) return rc;
            marks[0] = own_lo;
            r->own_c_begin = own_lo;
            if (fasta) {
                c_end = n;
                marks[1] = own_hi >= n ? ~0ull : own_hi;
            }
            r->range_eof = !bytes_follow;
            wait_own = true;
        }
        r->src = make(c_begin, c_end, true, marks);
        if (wait_own) {
            // The decoder tells where the shard's own bytes begin (mark 0) when it gets there; until then the halo's segments
            // are taken one by one — never a blocking wait for the mark: the decoder cannot run further ahead than its queue —
            // and only the newest `keep` bytes of them stay: a halo is made of whole frames / members, and with few large
            // frames in front of the shard everything from the stream's first byte would otherwise be resident (and copied
            // again for every segment more) before the shard's first row
            uint64_t own = 0;
            const uint64_t keep = std::max<uint64_t>(fasta ? 0 : r->halo_want, 256u << 10) + (64u << 10);
            for (uint64_t pos = 0, end = 0; !r->src->peek_mark(0, &own);) {
                if (end - pos > keep) pos = (end - keep) & ~15ull;  // (what lies in front of it is dropped by the acquire)
                const uint8_t *d_at = nullptr;
                uint64_t avail = 0;
                bool eof = false;
                std::string msg;
                int rc = r->src->acquire(pos, end - pos + 1, &d_at, &avail, &eof, &msg);  // one segment more
                if (rc) return fail(r, rc, msg);
                if (r->src->peek_mark(0, &own)) break;
                if (eof) {
                    own = ~0ull >> 1;  // (behind everything: the stream holds nothing of this shard's)
                    break;
                }
                end = pos + avail;
            }
            r->range_preset = true;
            r->preset_pos = own;
            r->data0_is_line_start = c_begin == 0;
        }
        if (fasta) {
            r->fa_shard = true;
            r->range_eof = true;  // (a shard of a FASTA is a FASTA file of its own)
        }
    } else {
        r->src = make(0, n, r->format == EXG_FMT_BAM, nullptr);  // (a BAM file is BGZF, SAM spec 4.1: any other gzip member in it is refused, like in a BCF)
        if (has_text_header(r)) {
            int rc = source_header_prefix(r, r->src.get(), *out_blk);
            if (rc) return rc;
        }
    }
    blk = out_blk;
    return EXG_OK;
}

int count_newlines_in_front(exg_reader *r, uint64_t *out) {
    *out = 0;
    if (!r->own_c_begin) return EXG_OK;
    const std::string &path = r->files[r->file_idx - 1];
    const int fd = r->fd_keep->fd;
    struct stat st;
    if (fstat(fd, &st)) return fail(r, EXG_E_IO, "cannot stat '" + path + "'");
    const uint64_t reserve = source_reserve(r), target = r->device_batch_bytes;
    if (r->compression == kBzip2) return fail(r, EXG_E_UNSUPPORTED, "shards of a bzip2 input are not supported: '" + path + "'");
    std::unique_ptr<SegmentProducer> prod = r->compression == kGzip
                                                ? make_gzip_producer(r, fd, 0, r->own_c_begin, target, path, true, reserve, nullptr)
                                                : make_zstd_producer(r, fd, (uint64_t)st.st_size, 0, r->own_c_begin, target, path, reserve, nullptr);
    DecodedSource head(r->device, r->stream, std::move(prod), reserve, 1, &r->meter);
    for (uint64_t pos = 0;;) {
        const uint8_t *d_at = nullptr;
        uint64_t avail = 0;
        bool eof = false;
        std::string msg;
        int rc = head.acquire(pos, 1, &d_at, &avail, &eof, &msg);
        if (rc) return fail(r, rc, msg);
        if (avail) {
            uint64_t nl = 0;
            const uint64_t skew = pos & 15;  // (an address is congruent to its stream offset mod 16)
            if ((rc = fetch_word(r, &nl, [&](void *d_word) { return exg_count_newlines(d_at - skew, skew, skew + avail, (uint64_t *)d_word, r->stream); })))
                return rc;
            *out += nl;
            pos += avail;
        }
        if (eof) break;
        if (!avail) return fail(r, EXG_E_HIP, "internal: a decoded source returned nothing before its end");
    }
    std::string e;
    const int frc = head.finish(&e);
    return frc ? fail(r, frc, e) : EXG_OK;
}

// Where this reader's bytes of the file just opened begin and end (file_pos, range_hi), and whether its first batch takes a halo
static int place_shard(exg_reader *r, const PinnedBlock &blk) {
    if (r->fa_shard) {
        // a shard of a compressed FASTA: the run of whole records from the first '>' line that begins in its own bytes to the
        // first that begins behind them (found while scanning: next_batch), like a text shard's run
        r->shard_first = false;
        if (r->preset_pos == 0 && r->data0_is_line_start) {
            r->file_pos = 0;
        } else {
            uint64_t at = ~0ull;
            int rc = source_find_record(r, r->preset_pos, &at);
            if (rc) return rc;
            if (at == ~0ull) r->file_done = true;  // no record begins in this shard's bytes (or behind them)
            else r->file_pos = at;
        }
    } else if (r->range_preset) {  // BGZF / zstd shard: the members / frames were chosen in open_source
        // its stream begins with the file (header and all) or somewhere behind the header
        r->data_base = r->data0_is_line_start ? r->data_base : 0;
        r->file_pos = std::max<uint64_t>(r->preset_pos, r->data_base);
        r->shard_first = r->file_pos > r->data_base;
    } else if (r->shard_count > 1 && r->format == EXG_FMT_FASTA) {
        // FASTA: a record belongs to the shard in whose bytes its '>' line BEGINS, and a shard is the run of whole
        // records from its first such line to the next shard's — scanned like a file of its own (a record is never
        // cut, however long its sequence: the run simply reaches as far as it has to)
        const char *d = (const char *)blk.p;
        const uint64_t N = blk.n;
        auto first_record_at_or_after = [&](uint64_t pos) -> uint64_t {
            if (pos == 0) return 0;
            for (uint64_t q = pos - 1; q + 1 < N;) {  // a line start is the byte behind a newline
                const void *hit = memchr(d + q, '\n', (size_t)(N - q));
                if (!hit) return N;
                q = (uint64_t)((const char *)hit - d) + 1;
                if (q < N && d[q] == '>') return q;
            }
            return N;
        };
        const uint64_t lo = (uint64_t)((unsigned __int128)N * r->shard_index / r->shard_count);
        const uint64_t hi = r->shard_index + 1 == r->shard_count ? N : (uint64_t)((unsigned __int128)N * (r->shard_index + 1) / r->shard_count);
        r->file_pos = first_record_at_or_after(lo);
        r->range_hi = hi == N ? N : first_record_at_or_after(hi);
        if (r->range_hi < r->file_pos) r->range_hi = r->file_pos;
        r->range_eof = true;  // the run is a FASTA file of its own
    } else if (r->shard_count > 1) {
        const uint64_t base = r->file_pos, span = blk.n - base;
        const uint64_t lo = base + (uint64_t)((unsigned __int128)span * r->shard_index / r->shard_count);
        const uint64_t hi = r->shard_index + 1 == r->shard_count
                                ? blk.n
                                : base + (uint64_t)((unsigned __int128)span * (r->shard_index + 1) / r->shard_count);
        r->file_pos = lo;
        r->range_hi = hi;
        r->shard_first = lo > base;
        r->range_eof = hi == blk.n;
    }
    return EXG_OK;
}

int open_next_file(exg_reader *r) {
    if (int jrc = r->finish_source()) return jrc;
    r->src.reset();  // (its thread reads the previous file's descriptor)
    const std::string &p = r->files[r->file_idx++];
    int fd = open(p.c_str(), O_RDONLY);
    if (fd < 0) return fail(r, EXG_E_IO, "cannot open '" + p + "': " + strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0) {
        const std::string why = strerror(errno);
        close(fd);
        return fail(r, EXG_E_IO, "cannot stat '" + p + "': " + why);
    }
    if (!S_ISREG(st.st_mode)) {
        close(fd);
        return fail(r, EXG_E_IO, "'" + p + "' is not a regular file");
    }
    auto blk = std::make_shared<PinnedBlock>();
    blk->n = (size_t)st.st_size;
    double t0 = now_s();
    if (r->compression != kNone) {
        // decoded by a producer thread that reads the file with pread: nothing is mapped
    } else if (blk->n) {
        // The file is mapped, not copied: DataChunk strings point straight into the page cache mapping
        // (kept alive by the chunks); bytes travel to the device through a pinned bounce buffer.
        void *m = mmap(nullptr, blk->n, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) {
            close(fd);
            return fail(r, EXG_E_IO, "cannot map '" + p + "': " + strerror(errno));
        }
        blk->p = m;
        blk->mapped = blk->n;
        // (another process may truncate the file while its rows are out: zeros + EXG_E_IO at the next call, not a SIGBUS that
        // ends the DuckDB process — exg_map_guard.hpp)
        blk->guard = MapGuard::add(m, blk->n);
        if (blk->guard < 0) {  // (the table holds 4096 mappings: chunks of thousands of files are still out)
            blk.reset();       // (unmaps)
            close(fd);
            return fail(r, EXG_E_NOMEM, "too many text files mapped at once (4096): release chunks or close readers before opening '" + p + "'");
        }
    } else {
        hipError_t he = hipHostMalloc(&blk->p, 64, hipHostMallocDefault);
        if (he != hipSuccess) {
            close(fd);
            return fail(r, EXG_E_HIP, std::string("hipHostMalloc failed: ") + hipGetErrorString(he));
        }
        memset(blk->p, 0, 64);
    }
    r->fd_keep.reset(new exg_reader::FdCloser{fd});
    TRACE("mmap(file)", t0);
    r->range_preset = false;
    r->range_eof = true;
    r->data0_is_line_start = true;
    r->own_c_begin = 0;
    r->exact_nl_known = false;
    (void)r->join_prefetch();
    r->drop_prefetch2();
    if (r->pf.valid && r->up_stream) (void)hipStreamSynchronize(r->up_stream);  // a prefetch of the previous file
    r->pf.valid = false;
    if (r->compression != kNone) {
        int rc = open_source(r, blk, p, (uint64_t)st.st_size);  // replaces blk (decoded size unknown; VCF: the header prefix on the host)
        if (rc) return rc;
    }
    r->file = blk;
    r->file_pos = 0;
    r->file_done = false;
    if (r->format == EXG_FMT_VCF) {
        // header = the leading '#' lines (noodles-vcf read_header); it must hold the #CHROM line
        const char *d = (const char *)blk->p;
        const size_t hn = r->compression != kNone ? (size_t)r->gz_header_prefix : blk->n;  // gzip / zstd: only the header prefix is on the host
        size_t pos = 0;
        bool chrom = false;
        while (pos < hn && d[pos] == '#') {
            if (hn - pos >= 6 && memcmp(d + pos, "#CHROM", 6) == 0) chrom = true;
            const void *nl = memchr(d + pos, '\n', hn - pos);
            pos = nl ? (size_t)((const char *)nl - d) + 1 : hn;
        }
        if (!chrom) return fail(r, EXG_E_PARSE, std::string(exg_parse_error_string(EXG_PE_VCF_NO_HEADER)) + " in '" + p + "'");
        r->vcf_header_bytes = pos;
        r->file_pos = pos;
    } else if (r->format == EXG_FMT_SAM) {
        // header = the leading '@' lines, skipped unread (a header-only or empty file has no rows); a decoded stream has the
        // prefix that holds them on the host, however long they are (source_header_prefix)
        r->file_pos = sam_header_end((const char *)blk->p, r->compression != kNone ? (size_t)r->gz_header_prefix : blk->n);
    }
    // byte-range shard of this file: [lo, hi) of the bytes behind the header; records / lines belong to the shard they END in
    r->range_hi = r->src ? ~0ull : blk->n;  // (a decoded stream ends where its source says so)
    r->shard_first = false;
    r->data_base = r->file_pos;  // 0, or the end of the VCF header
    if (r->format == EXG_FMT_BAM) return bam_open_file(r);  // (the header, from the front of the decoded stream; one shard)
    // Which scan first: from the first MiB behind the header, which is mapped anyway (a decoded stream has no bytes on the host: its
    // first batches' results decide, as before).  The batches' result flags correct the choice either way.
    if (!r->src && blk->p && blk->n > r->file_pos && !getenv("EXG_NO_ALGO_HINT"))
        r->fused_algo = (uint32_t)exg_scan_algo_hint(r->format, (const uint8_t *)blk->p + r->file_pos, blk->n - r->file_pos);
    r->ramp_bytes = (!r->src && r->format != EXG_FMT_FASTA && !switches().no_ramp && r->device_batch_bytes > kRampFirstBytes) ? kRampFirstBytes : 0;
    return r->fa_shard || r->range_preset || r->shard_count > 1 ? place_shard(r, *blk) : EXG_OK;
}

}  // namespace exg_rd
