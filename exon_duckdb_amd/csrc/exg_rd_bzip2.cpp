// exg_rd_bzip2.cpp — reader level, bzip2 inputs (compression='bzip2') as a bounded stream of decoded segments
// (exg_rd_source.hpp).  Replaces DataFusion 28 `FileCompressionType::BZIP2.convert_stream` behind rust/src/arrow_reader.rs:87-88.
//
// The producer decodes in ROUNDS: a window of compressed bytes is read into pinned memory and sent to the device, the blocks
// that begin at the carried bit offset and end inside the window are decoded (exg::bz2::decode_round), and their bytes go out
// as one segment.  What a round leaves unfinished — a block that runs past the window, or blocks beyond the round's memory —
// is read again by the next round from its block's first bit.  A round holds, per block, its BWT column and LF vector
// (5 bytes per byte of BWT input) beside its output: under EXG_DEVICE_MEM_CAP_MB the rounds shrink to one block.
#include <errno.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>

#include "exg_bzip2.hpp"
#include "exg_rd_source.hpp"

namespace exg_rd {

namespace bz = exg::bz2;

namespace {

class Bzip2Producer : public SegmentProducer {
public:
    Bzip2Producer(exg_reader *r, int fd, uint64_t n, uint64_t target, const std::string &path, uint64_t reserve)
        : device_(r->device), fd_(fd), n_(n), cap_(r->mem_cap), target_(round_out_bytes(target, 128u << 10, r->mem_cap != 0)), path_(path), reserve_((reserve + 15) & ~15ull) {
        if (const char *e = getenv("EXG_BZIP2_WINDOW_BYTES")) window_bytes_ = std::max<uint64_t>(16, strtoull(e, nullptr, 10));
    }
    int run(SegmentSink &sink, std::string *err) override;

private:
    int device_, fd_;
    uint64_t n_, cap_, target_;
    std::string path_;
    uint64_t reserve_;
    uint64_t window_bytes_ = 0;  // 0: sized from the blocks seen so far
};

int Bzip2Producer::run(SegmentSink &sink, std::string *err) {
    StreamLease st(device_);
    if (!st.acquire()) {
        *err = "cannot create a stream for the bzip2 decoder";
        return EXG_E_HIP;
    }
    int level = 9;
    if (n_ >= 4) {
        uint8_t head[4];
        if (pread(fd_, head, 4, 0) != 4) {
            *err = "short read of '" + path_ + "'";
            return EXG_E_IO;
        }
        if (head[3] >= '1' && head[3] <= '9') level = head[3] - '0';
    }
    PoolBuf d_win(device_, st);
    PinBuf pin;
    uint64_t bit = 0, d_pos = 0, blocks = 0;  // where the next round begins (file bit), decoded bytes so far, blocks so far
    bool at_header = true, first = true, pushed_last = false;
    uint32_t scrc = 0;
    uint64_t est_block = 0;  // compressed bytes per block seen so far
    uint64_t grow = 1;       // a block larger than the window: the window doubles until it holds one
    while (n_ && !sink.cancelled()) {  // (an empty file is an empty stream, as bz2 reads it)
        const uint64_t lo = (bit >> 3) & ~15ull;
        // blocks per round: the output target, and under a cap what the round's workspace may hold (~5.3 bytes per byte of
        // BWT input beside the output)
        const uint64_t slot = (uint64_t)level * 100000;
        uint64_t max_blocks = std::max<uint64_t>(1, target_ / slot);
        if (cap_) max_blocks = std::max<uint64_t>(1, std::min<uint64_t>(max_blocks, (cap_ / 3) / (slot * 53 / 10)));
        uint64_t want = est_block ? max_blocks * est_block + est_block / 2 + (64u << 10) : (cap_ ? (1u << 20) : std::max<uint64_t>(4u << 20, target_ / 3));
        if (window_bytes_) want = window_bytes_ * grow;  // (EXG_BZIP2_WINDOW_BYTES, tests: windows smaller than a block)
        else want = std::max<uint64_t>(want, 256u << 10) * grow;
        const uint64_t len = std::min<uint64_t>(want, n_ - std::min(n_, lo));
        const size_t wcap = (size_t)len + 128;
        if (!d_win.p || d_win.sz < wcap) {
            if (!d_win.take(wcap + wcap / 4)) {
                *err = "out of device memory for the compressed bytes of '" + path_ + "'";
                return EXG_E_HIP;
            }
        }
        if (pin.cap < wcap && !pin.ensure(wcap + wcap / 4)) {
            *err = "out of pinned host memory for the compressed bytes of '" + path_ + "'";
            return EXG_E_HIP;
        }
        if (len)
            if (int rc = read_to_device(device_, fd_, lo, (size_t)len, pin.p, (char *)d_win.p, st, path_, err)) return rc;
        if (hipMemsetAsync((char *)d_win.p + len, 0, 128, st) != hipSuccess) {
            *err = "hipMemsetAsync failed";
            return EXG_E_HIP;
        }
        bz::Round R;
        R.d_comp = d_win.p;
        R.n = len;
        R.bit0 = bit - lo * 8;
        R.at_header = at_header;
        R.first_stream = first;
        R.level = level;
        R.final_window = lo + len >= n_;
        R.max_blocks = max_blocks;
        const uint64_t pad = d_pos & 15;
        R.front_reserve = reserve_ + pad;
        R.blocks_before = blocks;
        uint64_t good = 0;
        const int rc = bz::decode_round(R, st, &good);
        auto push = [&](uint64_t bytes, bool last) -> bool {
            Segment seg;
            seg.buf = R.d_out;
            seg.cap = R.alloc;
            seg.org = (int64_t)(d_pos - pad) - (int64_t)reserve_;
            seg.lo = seg.start = d_pos;
            seg.hi = d_pos + bytes;
            seg.last = last;
            R.d_out = nullptr;
            d_pos += bytes;
            pushed_last = last;
            return sink.push(std::move(seg));
        };
        if (rc) {
            const std::string msg = std::string(exg_last_error_message()) + in_file(path_);
            if (R.d_out && good) (void)push(good, false);  // the rows in front of the damage first
            else if (R.d_out) sink.give(R.d_out, R.alloc);
            *err = msg;
            return rc;
        }
        // the stream CRCs: the blocks' CRCs folded in order, checked at every end of stream
        std::string crc_error;
        for (const bz::Round::Event &e : R.events) {
            if (e.kind == 0) {
                scrc = bz::fold_crc(scrc, e.value);
            } else {
                if (e.value != scrc && crc_error.empty())
                    crc_error = "bzip2: data error: stream CRC mismatch (combined CRC " + std::to_string(scrc) + ", stored " + std::to_string(e.value) + ")" + in_file(path_);
                scrc = 0;
            }
        }
        const bool progress = R.n_blocks || R.bit_end != R.bit0 || R.at_header_out != at_header;
        if (R.n_blocks) est_block = std::max<uint64_t>(1, (R.bit_end - R.bit0) / 8 / R.n_blocks), grow = 1;
        else if (!progress) grow *= 2;
        blocks += R.n_blocks;
        bit = lo * 8 + R.bit_end;
        at_header = R.at_header_out;
        level = R.level_out;
        if (progress) first = false;
        if (!crc_error.empty()) {
            if (R.produced) (void)push(R.produced, false);
            else sink.give(R.d_out, R.alloc);
            *err = crc_error;
            return EXG_E_PARSE;
        }
        if (R.produced || R.done) {
            if (!push(R.produced, R.done)) return EXG_OK;  // the consumer closed the stream
        } else {
            sink.give(R.d_out, R.alloc);
        }
        if (R.done) break;
        if (!progress && lo + len >= n_) {
            *err = "bzip2: unexpected end of stream" + in_file(path_);
            return EXG_E_PARSE;
        }
    }
    // (the consumer expects a last segment, even an empty one)
    if (!pushed_last && !sink.cancelled()) return push_empty_last(sink, d_pos, reserve_, st, err);
    return EXG_OK;
}

}  // namespace

std::unique_ptr<SegmentProducer> make_bzip2_producer(exg_reader *r, int fd, uint64_t n, uint64_t target, const std::string &path, uint64_t reserve) {
    return std::unique_ptr<SegmentProducer>(new Bzip2Producer(r, fd, n, target, path, reserve));
}

}  // namespace exg_rd
