// exg_rd_bcf.cpp — reader level of read_bcf_file_records: a BCF file is BGZF members around a header and binary records that
// stand for VCF lines.  This producer sits between the BGZF producer and the VCF reader: it consumes the decoded BCF bytes
// (a DecodedSource of its own, on its own thread and stream), reads the header (exg_bcf_header.cpp), puts the two
// dictionaries into device memory, and pushes segments of VCF TEXT — the header's text first, verbatim, then the lines the
// device transcoder (exg_bcf.hip) renders from the records.  Everything behind it is the VCF reader as it is: the header
// hand-over, the scan, the nested columns, filters, projection, host mirrors, the memory cap.
//
// A segment is sized by its OUTPUT: the transcoder is given `target` bytes of room and says how many records fit; the input
// goes on from there (the tail record, or the records that did not fit, are the next call's).  Text grows over binary (an int8
// `-100,` is five bytes for one), so the decoded BCF is asked for in smaller pieces than the text is handed on in.  A single
// record whose line does not fit a segment is an error, not a loop.
#include <string.h>

#include <algorithm>

#include "exg_bcf.hpp"
#include "exg_bcf_header.hpp"
#include "exg_rd_source.hpp"
#include "exg_rd_stages.hpp"

namespace exg_rd {

uint64_t bcf_input_target(uint64_t target) { return std::max<uint64_t>(64u << 10, (target / 4) & ~15ull); }
uint64_t bcf_input_reserve(uint64_t target) { return std::min<uint64_t>(std::max<uint64_t>(bcf_input_target(target) / 8, 64u << 10), 8u << 20); }

namespace {

class BcfProducer : public SegmentProducer {
public:
    BcfProducer(exg_reader *r, std::unique_ptr<SegmentProducer> decoded, uint64_t in_reserve, uint64_t target, const std::string &path, uint64_t reserve)
        : r_(r), decoded_(std::move(decoded)), in_reserve_(in_reserve), target_(std::max<uint64_t>(target, 4096)), path_(path), reserve_((reserve + 15) & ~15ull) {}
    int run(SegmentSink &sink, std::string *err) override;

private:
    struct Tables {  // the dictionaries on the device, and the transcoder's scratch
        SegmentSink *sink = nullptr;
        hipStream_t st = nullptr;
        void *contig_bytes = nullptr, *contig_table = nullptr, *string_bytes = nullptr, *string_table = nullptr, *res = nullptr, *ws = nullptr;
        size_t contig_bytes_n = 0, contig_table_n = 0, string_bytes_n = 0, string_table_n = 0, ws_n = 0;
        ~Tables() {
            if (!sink) return;
            (void)hipStreamSynchronize(st);  // (an error return may leave work in flight, and the pool is process-wide)
            sink->give(contig_bytes, contig_bytes_n), sink->give(contig_table, contig_table_n);
            sink->give(string_bytes, string_bytes_n), sink->give(string_table, string_table_n);
            sink->give(res, 4096), sink->give(ws, ws_n);
        }
    };
    int read_header(DecodedSource &src, hipStream_t st, BcfHeader *h, std::string *err);
    int upload(SegmentSink &sink, hipStream_t st, const BcfHeader &h, Tables *t, std::string *err);

    exg_reader *r_;
    std::unique_ptr<SegmentProducer> decoded_;
    uint64_t in_reserve_, target_;
    std::string path_;
    uint64_t reserve_;
};

int BcfProducer::read_header(DecodedSource &src, hipStream_t st, BcfHeader *h, std::string *err) {
    PinBuf host;
    auto front = [&](uint64_t want, uint64_t *avail, bool *eof) {
        const uint8_t *d_at = nullptr;
        int rc = src.acquire(0, want, &d_at, avail, eof, err);
        if (rc) {
            if (err->find(path_) == std::string::npos) *err += in_file(path_);
            return rc;
        }
        const uint64_t len = std::min<uint64_t>(want, *avail);
        if (!host.ensure((size_t)len + 64)) {
            *err = "out of pinned host memory for the BCF header";
            return (int)EXG_E_HIP;
        }
        if (len) PRODUCER_HIP(hipMemcpyAsync(host.p, d_at, len, hipMemcpyDeviceToHost, st));
        PRODUCER_HIP(hipStreamSynchronize(st));
        return (int)EXG_OK;
    };
    auto inspect = [&](uint64_t len, bool ended, uint64_t *need) {
        std::string why;
        const int prc = bcf_parse_header((const uint8_t *)host.p, len, ended, h, need, &why);
        if (prc == kBcfHeaderBad) {
            *err = why + in_file(path_);
            return (int)EXG_E_PARSE;
        }
        return prc == kBcfHeaderOk ? (int)kPrefixDone : (int)kPrefixMore;
    };
    return read_prefix(64u << 10, front, inspect, prefix_grow_need_or_double);
}

int BcfProducer::upload(SegmentSink &sink, hipStream_t st, const BcfHeader &h, Tables *t, std::string *err) {
    t->sink = &sink, t->st = st;
    t->contig_bytes_n = h.contigs.bytes.size() + 64, t->contig_table_n = h.contigs.table.size() * 4 + 64;
    t->string_bytes_n = h.strings.bytes.size() + 64, t->string_table_n = h.strings.table.size() * 4 + 64;
    if (!(t->contig_bytes = sink.take(t->contig_bytes_n)) || !(t->contig_table = sink.take(t->contig_table_n)) ||
        !(t->string_bytes = sink.take(t->string_bytes_n)) || !(t->string_table = sink.take(t->string_table_n)) || !(t->res = sink.take(4096))) {
        *err = "out of device memory for the BCF dictionaries of '" + path_ + "'";
        return EXG_E_HIP;
    }
    if (!h.contigs.bytes.empty()) PRODUCER_HIP(hipMemcpyAsync(t->contig_bytes, h.contigs.bytes.data(), h.contigs.bytes.size(), hipMemcpyHostToDevice, st));
    if (!h.contigs.table.empty()) PRODUCER_HIP(hipMemcpyAsync(t->contig_table, h.contigs.table.data(), h.contigs.table.size() * 4, hipMemcpyHostToDevice, st));
    if (!h.strings.bytes.empty()) PRODUCER_HIP(hipMemcpyAsync(t->string_bytes, h.strings.bytes.data(), h.strings.bytes.size(), hipMemcpyHostToDevice, st));
    if (!h.strings.table.empty()) PRODUCER_HIP(hipMemcpyAsync(t->string_table, h.strings.table.data(), h.strings.table.size() * 4, hipMemcpyHostToDevice, st));
    PRODUCER_HIP(hipStreamSynchronize(st));
    return EXG_OK;
}

int BcfProducer::run(SegmentSink &sink, std::string *err) {
    StreamLease st(r_->device, true);
    if (!st.s) {
        *err = "cannot make a HIP stream for the BCF transcoder";
        return EXG_E_HIP;
    }
    // the decoded BCF bytes: a bounded stream of their own, one segment queued
    DecodedSource src(r_->device, st, std::move(decoded_), in_reserve_, 1, &r_->meter);
    BcfHeader h;
    int rc = read_header(src, st, &h, err);
    if (rc) return rc;
    Tables t;
    if ((rc = upload(sink, st, h, &t, err))) return rc;

    uint64_t in_pos = h.end, t_pos = 0, records = 0;
    uint64_t head = h.text.size();  // the header's text goes in front of the first segment's lines
    uint64_t want = bcf_input_target(target_);
    for (;;) {
        if (sink.cancelled()) return EXG_OK;
        const uint8_t *d_at = nullptr;
        uint64_t n = 0;
        bool eof = false;
        if ((rc = src.acquire(in_pos, want, &d_at, &n, &eof, err))) {
            if (err->find(path_) == std::string::npos) *err += in_file(path_);
            return rc;
        }
        const uint64_t ws_need = exg::bcf::workspace_bytes(n);
        if (ws_need > t.ws_n) {
            sink.give(t.ws, t.ws_n);
            t.ws_n = (size_t)(ws_need + ws_need / 4);
            if (!(t.ws = sink.take(t.ws_n))) {
                t.ws_n = 0;
                *err = "out of device memory (" + std::to_string(ws_need >> 20) + " MiB) for the BCF transcoder of '" + path_ + "'";
                return EXG_E_HIP;
            }
        }
        Segment seg;
        seg.cap = (size_t)(reserve_ + 16 + head + target_ + 64);
        if (!(seg.buf = sink.take(seg.cap))) {
            *err = "out of device memory (" + std::to_string(seg.cap >> 20) + " MiB) for a segment of VCF text of '" + path_ + "'";
            return EXG_E_HIP;
        }
        seg.org = (int64_t)(t_pos & ~15ull) - (int64_t)reserve_;
        seg.lo = seg.start = t_pos;
        uint8_t *out = (uint8_t *)seg.buf + reserve_ + (t_pos & 15);
        struct GiveBack {  // (until the segment is pushed)
            SegmentSink &sink;
            Segment &seg;
            hipStream_t st;
            ~GiveBack() {
                if (!seg.buf) return;
                (void)hipStreamSynchronize(st);
                sink.give(seg.buf, seg.cap);
            }
        } give_back{sink, seg, st};
        if (head) PRODUCER_HIP(hipMemcpyAsync(out, h.text.data(), head, hipMemcpyHostToDevice, st));
        exg_bcf_to_vcf_args a;
        memset(&a, 0, sizeof a);
        a.d_input = d_at, a.n_bytes = n;
        a.flags = eof ? EXG_F_EOF : 0u;
        a.n_samples = h.n_samples;
        a.d_contig_bytes = (const uint8_t *)t.contig_bytes, a.d_contig_table = (const uint32_t *)t.contig_table, a.n_contigs = h.contigs.size();
        a.d_string_bytes = (const uint8_t *)t.string_bytes, a.d_string_table = (const uint32_t *)t.string_table, a.n_strings = h.strings.size();
        a.gt_index = h.gt_index;
        a.d_output = out + head, a.output_capacity = target_;
        a.d_workspace = t.ws, a.workspace_bytes = t.ws_n;
        a.d_result = (exg_bcf_to_vcf_result *)t.res;
        a.stream = st.s;
        exg_bcf_to_vcf_result res;
        if ((rc = exg::bcf::to_vcf(&a, &res))) {
            *err = std::string(exg_last_error_message()) + in_file(path_);
            return rc;
        }
        if (!res.n_records && !res.error_code && n) {
            if (res.flags & EXG_RF_CAPACITY) {
                *err = "BCF record " + std::to_string(records) + " is a VCF line longer than a segment of the stream (" + std::to_string(target_) +
                       " bytes; raise EXG_DEVICE_BATCH_BYTES / EXG_DEVICE_MEM_CAP_MB)" + in_file(path_);
                return EXG_E_CAPACITY;
            }
            if (!eof) {  // one record larger than what was asked for: more of the stream (its segments are appended to the tail)
                want = std::max<uint64_t>(want, n) * 2;
                continue;
            }
        }
        const uint64_t text = head + res.text_bytes;
        PRODUCER_HIP(hipMemsetAsync(out + text, 0, 64, st));
        PRODUCER_HIP(hipStreamSynchronize(st));
        seg.hi = t_pos + text;
        seg.last = !res.error_code && eof && res.consumed_bytes == n;
        const bool last = seg.last;
        t_pos = seg.hi, in_pos += res.consumed_bytes, records += res.n_records, head = 0;
        want = bcf_input_target(target_);
        if (!sink.push(std::move(seg))) return EXG_OK;  // (the consumer is gone; push gave the block back)
        seg.buf = nullptr;
        if (res.error_code) {  // the lines in front of the record are on their way; the consumer meets the error behind them
            *err = "invalid BCF record " + std::to_string(records) + ": " + exg_parse_error_string(res.error_code) + " at byte " +
                   std::to_string(in_pos) + " of the decoded stream of " + path_;
            return EXG_E_PARSE;
        }
        if (last) break;
    }
    std::string ferr;
    if ((rc = src.finish(&ferr))) {  // (a checksum that is verified behind the last member)
        *err = ferr;
        return rc;
    }
    return EXG_OK;
}

}  // namespace

std::unique_ptr<SegmentProducer> make_bcf_producer(exg_reader *r, std::unique_ptr<SegmentProducer> decoded, uint64_t in_reserve, uint64_t target,
                                                   const std::string &path, uint64_t reserve) {
    return std::unique_ptr<SegmentProducer>(new BcfProducer(r, std::move(decoded), in_reserve, target, path, reserve));
}

}  // namespace exg_rd
