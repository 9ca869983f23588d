// exg_rd_region.cpp — reader level of vcf_query: see exg_rd_region.hpp.  The index (<path>.tbi, itself BGZF) and the planned
// members of the data file go through the same few steps — a window of whole members is read, inflated by exg_inflate_members,
// and every member's size and CRC-32 are checked (Inflater) —; no zlib is linked.
#include "exg_rd_region.hpp"

#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>

#include "exg_sam_header.hpp"

namespace exg_rd {

RegionPlan::~RegionPlan() {
    if (d_name) dev_pool()->give(device, d_name, d_name_bytes);
}

int region_member_ranges(int fd, uint64_t n, const std::vector<exg_virtual_chunk> &chunks, std::vector<MemberRange> *out, std::string *err) {
    out->clear();
    Peek peek(nullptr, fd, n);
    auto stale = [&](uint64_t voff, const char *why) {
        *err = "the index does not belong to this file (stale, or another file's): virtual offset " + std::to_string(voff >> 16) + ":" +
               std::to_string(voff & 0xFFFF) + " " + why;
        return EXG_E_IO;
    };
    // a member header at c, and `u` inside its inflated bytes; *next: the member behind it
    auto member = [&](uint64_t voff, uint64_t *next) {
        exg_inflate_member m;
        const uint64_t c = voff >> 16;
        if (c >= n) return stale(voff, "lies outside the file");
        if (!(*next = bgzf_member_at(peek, c, &m))) return stale(voff, "is not on a BGZF member header");
        if ((voff & 0xFFFF) > m.out_cap) return stale(voff, "lies behind the inflated bytes of its member");
        return (int)EXG_OK;
    };
    for (const exg_virtual_chunk &ch : chunks) {
        uint64_t next = 0;
        if (ch.end < ch.begin) return stale(ch.end, "ends a chunk in front of its begin");
        if (int rc = member(ch.begin, &next)) return rc;
        MemberRange mr{ch.begin >> 16, ch.end >> 16, (uint32_t)(ch.begin & 0xFFFF)};
        if (ch.end & 0xFFFF) {  // the last member counts
            if (int rc = member(ch.end, &next)) return rc;
            mr.c_end = next;
        } else if (mr.c_end != n) {  // (the end of the file is a member boundary by itself)
            if (int rc = member(ch.end, &next)) return rc;
        }
        if (!out->empty() && mr.c_begin <= out->back().c_end) out->back().c_end = std::max(out->back().c_end, mr.c_end);  // overlapping or adjacent
        else if (mr.c_end > mr.c_begin) out->push_back(mr);
    }
    return EXG_OK;
}

namespace {

// Whole BGZF members of a file: a window of them is read and listed (window), then inflated into a device block and checked
// (inflate).  One stream; inflate() returns with the stream idle.
struct Inflater {
    int dev;
    hipStream_t st;
    PinBuf pin, tab;
    PoolBuf d_comp, d_tab;
    std::vector<exg_inflate_member> mem;
    std::vector<uint32_t> crc;
    uint64_t out = 0;  // inflated bytes of the window's members
    Inflater(int device, hipStream_t stream) : dev(device), st(stream), d_comp(device, stream), d_tab(device, stream) {}

    // the members from file offset c on that end at or in front of c_lim: as many as inflate to `room` bytes (one at least, at
    // most max_members).  *c_next: the first member not taken.  No member at c: EXG_E_IO
    int window(int fd, uint64_t c, uint64_t c_lim, uint64_t room, uint64_t max_members, const std::string &path, uint64_t *c_next, std::string *err) {
        mem.clear(), crc.clear(), out = 0;
        const uint64_t a0 = c & ~15ull;
        const uint64_t len = std::min<uint64_t>(c_lim - a0, room + (128u << 10) + (c - a0));  // (a member is at most 64 KiB, either way)
        if (!pin.ensure((size_t)len + 64) || !d_comp.take((size_t)len + 64)) {
            *err = "out of memory for a window of compressed bytes of '" + path + "'";
            return EXG_E_HIP;
        }
        if (int rc = read_to_device(dev, fd, a0, (size_t)len, pin.p, (char *)d_comp.p, st, path, err)) return rc;
        Peek pk((const uint8_t *)pin.p, -1, len);
        uint64_t rel = c - a0;
        while (rel < len && mem.size() < max_members) {
            exg_inflate_member m;
            uint32_t sum = 0;
            const uint64_t nx = bgzf_member_at(pk, rel, &m, &sum);
            if (!nx || (!mem.empty() && out + m.out_cap > room)) break;
            m.out_off = out;
            out += m.out_cap;
            mem.push_back(m), crc.push_back(sum);
            rel = nx;
        }
        if (mem.empty()) {
            *err = "no whole BGZF member at byte " + std::to_string(c) + " of '" + path + "' (a truncated file, or an index that does not belong to it)";
            return EXG_E_IO;
        }
        *c_next = a0 + rel;
        return EXG_OK;
    }
    // member i -> d_block + out_off + (the inflated sizes in front of it); 64 zero bytes behind the last
    int inflate(void *d_block, uint64_t out_off, const std::string &path, std::string *err) {
        const uint64_t k = mem.size();
        const size_t m_bytes = k * sizeof(exg_inflate_member), tab_bytes = m_bytes + k * (sizeof(exg_inflate_status) + 4) + 64;
        if (!tab.ensure(tab_bytes) || !d_tab.take(tab_bytes)) {
            *err = "out of memory for the member table";
            return EXG_E_HIP;
        }
        exg_inflate_member *h_m = (exg_inflate_member *)tab.p;
        for (uint64_t i = 0; i < k; i++) h_m[i] = mem[i], h_m[i].out_off += out_off;
        exg_inflate_member *d_m = (exg_inflate_member *)d_tab.p;
        exg_inflate_status *d_s = (exg_inflate_status *)((char *)d_tab.p + m_bytes);
        uint32_t *d_c = (uint32_t *)((char *)d_s + k * sizeof(exg_inflate_status));
        PRODUCER_HIP(hipMemcpyAsync(d_m, h_m, m_bytes, hipMemcpyHostToDevice, st));
        int rc = exg_inflate_members(d_comp.p, d_block, d_m, d_s, (uint32_t)k, st);
        if (!rc) rc = exg_crc32_members(d_block, d_m, d_s, (uint32_t)k, d_c, st);
        if (rc) {
            *err = exg_last_error_message();
            (void)hipStreamSynchronize(st);
            return rc;
        }
        PRODUCER_HIP(hipMemsetAsync((char *)d_block + out_off + out, 0, 64, st));
        PRODUCER_HIP(hipMemcpyAsync(tab.p + m_bytes, d_s, k * (sizeof(exg_inflate_status) + 4), hipMemcpyDeviceToHost, st));
        PRODUCER_HIP(hipStreamSynchronize(st));
        const exg_inflate_status *s = (const exg_inflate_status *)(tab.p + m_bytes);
        const uint32_t *c = (const uint32_t *)((const char *)s + k * sizeof(exg_inflate_status));
        for (uint64_t i = 0; i < k; i++) {
            if (s[i].code || s[i].produced != mem[i].out_cap || s[i].consumed + 8 != mem[i].comp_size) {
                *err = "corrupt deflate stream (a BGZF member, code " + std::to_string(s[i].code) + ")" + in_file(path);
                return EXG_E_PARSE;
            }
            if (c[i] != crc[i]) {
                *err = "corrupt gzip stream does not have a matching checksum" + in_file(path);
                return EXG_E_PARSE;
            }
        }
        return EXG_OK;
    }
};

struct Fd {
    int fd;
    ~Fd() {
        if (fd >= 0) close(fd);
    }
};

// the inflated bytes of a BGZF file (the index: a few MB at the most), window by window
int inflate_file(exg_reader *r, const std::string &path, std::vector<uint8_t> *bytes) {
    Fd f{open(path.c_str(), O_RDONLY)};
    struct stat st;
    if (f.fd < 0 || fstat(f.fd, &st) != 0) return fail(r, EXG_E_IO, "cannot open the index '" + path + "': " + strerror(errno));
    const uint64_t n = (uint64_t)st.st_size;
    Inflater inf(r->device, r->stream);
    PoolBuf d_out(r->device, r->stream);
    PinBuf h_out;
    std::string err;
    bytes->clear();
    for (uint64_t c = 0; c < n;) {
        uint64_t next = 0;
        int rc = inf.window(f.fd, c, n, 16u << 20, ~0ull, path, &next, &err);
        if (rc == EXG_E_IO) return fail(r, EXG_E_IO, "'" + path + "' is not a BGZF-compressed tabix index: " + err);
        if (rc) return fail(r, rc, err);
        if (!d_out.take((size_t)inf.out + 64) || !h_out.ensure((size_t)inf.out + 64)) return fail(r, EXG_E_HIP, "out of memory for the index '" + path + "'");
        if ((rc = inf.inflate(d_out.p, 0, path, &err))) return fail(r, rc, err);
        if (inf.out) {
            RD_HIP(r, hipMemcpyAsync(h_out.p, d_out.p, inf.out, hipMemcpyDeviceToHost, r->stream));
            RD_HIP(r, hipStreamSynchronize(r->stream));
            bytes->insert(bytes->end(), (const uint8_t *)h_out.p, (const uint8_t *)h_out.p + inf.out);
        }
        c = next;
    }
    return EXG_OK;
}

class RegionProducer : public SegmentProducer {
public:
    RegionProducer(exg_reader *r, int fd, uint64_t n, uint64_t target, const std::string &path, uint64_t reserve)
        : r_(r), fd_(fd), n_(n), target_(std::max<uint64_t>(target, 64u << 10)), path_(path), front_(((reserve + 15) & ~15ull) + (64u << 10)) {}
    int run(SegmentSink &sink, std::string *err) override;

private:
    // a segment with room for `bytes` of the stream at t_pos_ (and front_ bytes in front: the consumer's carry, and what a range's
    // first member holds in front of the range's first line)
    bool segment(SegmentSink &sink, uint64_t bytes, Segment *seg, std::string *err) {
        seg->cap = (size_t)(front_ + 16 + bytes + 64);
        if (!(seg->buf = sink.take(seg->cap))) {
            *err = "out of device memory (" + std::to_string(seg->cap >> 20) + " MiB) for a segment of '" + path_ + "'";
            return false;
        }
        seg->org = (int64_t)(t_pos_ & ~15ull) - (int64_t)front_;
        seg->lo = seg->start = seg->hi = t_pos_;
        return true;
    }
    uint64_t base() const { return front_ + (t_pos_ & 15); }  // offset of stream byte t_pos_ in a segment's block
    int header(SegmentSink &sink, Inflater &inf, std::string *err);
    int range(SegmentSink &sink, Inflater &inf, const MemberRange &mr, std::string *err);
    int complete_line(SegmentSink &sink, Inflater &inf, uint64_t c, std::string *err);

    exg_reader *r_;
    int fd_;
    uint64_t n_, target_;
    std::string path_;
    uint64_t front_;
    uint64_t t_pos_ = 0;  // the stream's bytes so far
    PinBuf host_;
};

struct GiveBack {  // (a segment's block until it is pushed)
    SegmentSink &sink;
    Segment &seg;
    ~GiveBack() {
        if (seg.buf) sink.give(seg.buf, seg.cap);
    }
};

// the leading members, one at a time, until a line that is not a header line begins (or the file ends): the header's text is the
// stream's first segment
int RegionProducer::header(SegmentSink &sink, Inflater &inf, std::string *err) {
    std::string text;
    PoolBuf d_out(r_->device, inf.st);
    size_t end = 0;
    for (uint64_t c = 0; c < n_;) {
        uint64_t next = 0;
        int rc = inf.window(fd_, c, n_, 64u << 10, 1, path_, &next, err);
        if (rc) return rc;
        if (!d_out.take((size_t)inf.out + 64) || !host_.ensure((size_t)inf.out + 64)) {
            *err = "out of memory for the header of '" + path_ + "'";
            return EXG_E_HIP;
        }
        if ((rc = inf.inflate(d_out.p, 0, path_, err))) return rc;
        if (inf.out) PRODUCER_HIP(hipMemcpyAsync(host_.p, d_out.p, inf.out, hipMemcpyDeviceToHost, inf.st));
        PRODUCER_HIP(hipStreamSynchronize(inf.st));
        text.append(host_.p, (size_t)inf.out);
        r_->region->members++;
        c = next;
        end = leading_lines_end(text.data(), text.size(), '#');
        if (end < text.size()) break;
    }
    Segment seg;
    if (!segment(sink, end, &seg, err)) return EXG_E_HIP;
    GiveBack give_back{sink, seg};
    if (end) PRODUCER_HIP(hipMemcpyAsync((char *)seg.buf + base(), text.data(), end, hipMemcpyHostToDevice, inf.st));
    PRODUCER_HIP(hipMemsetAsync((char *)seg.buf + base() + end, 0, 64, inf.st));
    PRODUCER_HIP(hipStreamSynchronize(inf.st));
    seg.hi = t_pos_ += end;
    (void)sink.push(std::move(seg));
    return EXG_OK;
}

// the lines that start in the range's members, about target_ bytes a segment
int RegionProducer::range(SegmentSink &sink, Inflater &inf, const MemberRange &mr, std::string *err) {
    uint64_t skip = mr.skip;
    bool at_line_start = true;
    for (uint64_t c = mr.c_begin; c < mr.c_end && !sink.cancelled();) {
        uint64_t next = 0;
        int rc = inf.window(fd_, c, mr.c_end, target_, ~0ull, path_, &next, err);
        if (rc) return rc;
        if (skip > inf.out) {
            *err = "the index does not belong to '" + path_ + "' (stale, or another file's): a chunk begins behind the inflated bytes of its member";
            return EXG_E_IO;
        }
        Segment seg;
        if (!segment(sink, inf.out, &seg, err)) return EXG_E_HIP;
        GiveBack give_back{sink, seg};
        // (the bytes in front of the range's first line land in the room in front of the segment's own)
        if ((rc = inf.inflate(seg.buf, base() - skip, path_, err))) return rc;
        const uint64_t bytes = inf.out - skip;
        if (bytes) {
            char last = 0;
            PRODUCER_HIP(hipMemcpyAsync(&last, (const char *)seg.buf + base() + bytes - 1, 1, hipMemcpyDeviceToHost, inf.st));
            PRODUCER_HIP(hipStreamSynchronize(inf.st));
            at_line_start = last == '\n';
        }
        r_->region->members += inf.mem.size();
        seg.hi = t_pos_ += bytes;
        skip = 0;
        c = next;
        if (!bytes) continue;  // (nothing of the range in these members: no segment)
        if (!sink.push(std::move(seg))) return EXG_OK;
    }
    return at_line_start || sink.cancelled() ? EXG_OK : complete_line(sink, inf, mr.c_end, err);
}

// the line that crosses out of a range's last member: the bytes up to its newline, from the member(s) at c on
int RegionProducer::complete_line(SegmentSink &sink, Inflater &inf, uint64_t c, std::string *err) {
    while (c < n_ && !sink.cancelled()) {
        uint64_t next = 0;
        int rc = inf.window(fd_, c, n_, 64u << 10, 1, path_, &next, err);
        if (rc) return rc;
        Segment seg;
        if (!segment(sink, inf.out, &seg, err) || !host_.ensure((size_t)inf.out + 64)) return EXG_E_HIP;
        GiveBack give_back{sink, seg};
        if ((rc = inf.inflate(seg.buf, base(), path_, err))) return rc;
        if (inf.out) PRODUCER_HIP(hipMemcpyAsync(host_.p, (const char *)seg.buf + base(), inf.out, hipMemcpyDeviceToHost, inf.st));
        PRODUCER_HIP(hipStreamSynchronize(inf.st));
        const void *nl = inf.out ? memchr(host_.p, '\n', (size_t)inf.out) : nullptr;
        const uint64_t bytes = nl ? (uint64_t)((const char *)nl - host_.p) + 1 : inf.out;
        if (nl) {  // (what the member holds behind the line is not this range's)
            PRODUCER_HIP(hipMemsetAsync((char *)seg.buf + base() + bytes, 0, 64, inf.st));
            PRODUCER_HIP(hipStreamSynchronize(inf.st));
        }
        seg.hi = t_pos_ += bytes;
        c = next;
        if (!sink.push(std::move(seg)) || nl) return EXG_OK;
    }
    return EXG_OK;
}

int RegionProducer::run(SegmentSink &sink, std::string *err) {
    StreamLease st(r_->device, true);
    if (!st.s) {
        *err = "cannot make a HIP stream for the region reader";
        return EXG_E_HIP;
    }
    Inflater inf(r_->device, st);
    int rc = header(sink, inf, err);
    for (size_t i = 0; !rc && i < r_->region->ranges.size() && !sink.cancelled(); i++) rc = range(sink, inf, r_->region->ranges[i], err);
    if (rc || sink.cancelled()) return rc;
    return push_empty_last(sink, t_pos_, front_, st, err);
}

}  // namespace

std::unique_ptr<SegmentProducer> make_region_producer(exg_reader *r, int fd, uint64_t n, uint64_t target, const std::string &path, uint64_t reserve) {
    r->region->members = 0;
    return std::unique_ptr<SegmentProducer>(new RegionProducer(r, fd, n, target, path, reserve));
}

int region_open(exg_reader *r, const char *region) {
    const std::string &path = r->files[0];
    std::vector<uint8_t> index;
    if (int rc = inflate_file(r, path + ".tbi", &index)) return rc;
    std::unique_ptr<RegionPlan> plan(new RegionPlan());
    plan->device = r->device;
    exg::tabix::Index idx;
    std::string err;
    if (!exg::tabix::parse_index(index.data(), index.size(), &idx, &err)) return fail(r, EXG_E_IO, "'" + path + ".tbi': " + err);
    if (!exg::tabix::parse_region(idx, region, &plan->region, &err)) return fail(r, EXG_E_INVALID_ARG, err + " ('" + path + ".tbi')");
    exg::tabix::plan(idx, plan->region, &plan->chunks);
    Fd f{open(path.c_str(), O_RDONLY)};
    struct stat st;
    if (f.fd < 0 || fstat(f.fd, &st) != 0) return fail(r, EXG_E_IO, "cannot open '" + path + "': " + strerror(errno));
    if (int rc = region_member_ranges(f.fd, (uint64_t)st.st_size, plan->chunks, &plan->ranges, &err)) return fail(r, rc, "'" + path + ".tbi': " + err);
    plan->d_name_bytes = plan->region.name.size() + 16;
    if (!(plan->d_name = dev_pool()->take(r->device, plan->d_name_bytes))) return fail(r, EXG_E_HIP, "out of device memory");
    RD_HIP(r, hipMemcpyAsync(plan->d_name, plan->region.name.data(), plan->region.name.size(), hipMemcpyHostToDevice, r->stream));
    RD_HIP(r, hipStreamSynchronize(r->stream));
    r->region = std::move(plan);
    return EXG_OK;
}

int region_keep(exg_reader *r, const void *d_input, uint64_t payload_base, uint64_t n_rows, uint64_t *d_keep) {
    exg_vcf_region_args a;
    memset(&a, 0, sizeof a);
    a.d_chrom = (const exg_string_t *)r->d_cols[0];
    a.d_ref = (const exg_string_t *)r->d_cols[3];
    a.d_pos = (const int64_t *)r->d_pos;
    a.d_info = (const exg_string_t *)r->d_cols[7];
    a.d_payload = d_input;
    a.payload_base = payload_base;
    a.n_rows = n_rows;
    a.d_name = (const uint8_t *)r->region->d_name;
    a.name_len = (uint32_t)r->region->region.name.size();
    a.start = r->region->region.start, a.end = r->region->region.end;
    a.d_keep = d_keep;
    a.stream = r->stream;
    const int rc = exg_vcf_region_keep(&a);
    return rc ? fail(r, rc, exg_last_error_message()) : EXG_OK;
}

}  // namespace exg_rd
