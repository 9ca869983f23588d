// exg_bzip2.hpp — bzip2 streams on the device (exg_bzip2.hip): what the reader's producer (exg_rd_bzip2.cpp) and the
// whole-stream entry point exg_bzip2_decode share.
//
// Replaces the decompression the reference gets from DataFusion 28 `FileCompressionType::BZIP2` (async-compression ->
// bzip2 -> libbz2), selected by compression='bzip2' at rust/src/arrow_reader.rs:87-88.
//
// A bzip2 stream is a run of blocks of at most level x 100 000 bytes of BWT input, each independent of the others and
// each beginning with a 48-bit magic, so the work is split by blocks:
//   (1) discovery: every bit offset of the window is tested for the block / end-of-stream magics (a hit inside Huffman
//       data is possible, so a candidate counts only when the block in front of it ends exactly there);
//   (2) one wavefront per candidate parses the header, builds the Huffman tables in LDS and decodes the symbols (RLE2,
//       inverse MTF) into the block's BWT column; one thread then chains the candidates from the round's first bit;
//   (3) inverse BWT: a stable counting sort builds the LF vector, and the cycle is cut at sampled splitters that are
//       walked in parallel twice (lengths, then bytes at prefix-sum offsets);
//   (4) RLE1 undo: the run state at a piece boundary is one of five, so every piece is sized for all five, the states
//       are composed per block, and the pieces then write their bytes and CRC terms.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace exg {
namespace bz2 {

static constexpr uint32_t kMaxBlock = 900000;  // level 9

// One round: the blocks that begin at `bit0` of the window and end inside it.
struct Round {
    // in
    const void *d_comp = nullptr;  // the window on the device: 16-byte aligned, zero bytes from n to n + 64
    uint64_t n = 0;                // bytes of the window
    uint64_t bit0 = 0;             // where the round begins (a stream header when at_header, else a block / end magic)
    bool at_header = true;
    bool first_stream = true;      // the file's first stream header is expected at bit0 (anything else: not a bzip2 stream)
    int level = 9;                 // the current stream's level (at_header: the level the host read from the header)
    bool final_window = true;      // the window reaches the end of the input
    uint64_t max_blocks = ~0ull;   // decode at most this many blocks
    uint64_t front_reserve = 0;    // bytes of room in front of the output (multiple of 16)
    uint64_t blocks_before = 0;    // blocks of the input decoded by earlier rounds (error messages)
    // out
    void *d_out = nullptr;  // a dev_pool block of `alloc` bytes: [front_reserve | produced | 64 zero bytes]
    size_t alloc = 0;
    uint64_t produced = 0;
    uint64_t bit_end = 0;   // where the next round begins
    bool at_header_out = false;
    int level_out = 9;
    bool done = false;      // the input ends here (after the last stream; trailing bytes that are no stream are ignored)
    uint32_t n_blocks = 0;  // blocks decoded
    // what the host folds into the stream CRCs, in order: a block's CRC (kind 0) or a stream's stored CRC (kind 1)
    struct Event {
        uint32_t kind, value;
    };
    std::vector<Event> events;
    std::vector<uint64_t> block_end;  // decoded bytes of the round after block i (a bad block: the rows in front of it first)
};

// EXG_OK, or EXG_E_PARSE (a data error; *good_bytes = decoded bytes in front of the damaged block, R.d_out holds them
// when R.d_out is set) / EXG_E_HIP; the message is set (exg_last_error_message).  Synchronises the stream.
int decode_round(Round &R, void *stream, uint64_t *good_bytes);

// the per-block CRCs folded into a stream's combined CRC (bzip2: c = rotl1(c) ^ block_crc)
inline uint32_t fold_crc(uint32_t c, uint32_t block_crc) { return ((c << 1) | (c >> 31)) ^ block_crc; }

}  // namespace bz2
}  // namespace exg
