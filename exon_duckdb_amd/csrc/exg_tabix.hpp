// exg_tabix.hpp — host only (no HIP include): a tabix index (.tbi, the INFLATED bytes), the region grammar of the *_query table
// functions and the planner that turns a region into the BGZF virtual-offset chunks a reader has to look at.  Replaces what
// noodles-tabix / noodles-csi do behind the reference's vcf_query (rust/src/vcf_query_reader.rs; exon_extension.cpp:75-77).
// Everything read here is a user's file: the TU is built with ASan / UBSan in tests/region_host_driver.cpp.
//
// Region grammar [RECALLED: noodles-core Region::from_str]
//   G1  the whole string is a name of the index: that reference, unbounded
//   G2  else the string is split at its LAST ':'; `start` or `start-end` behind it — decimal digits only (at most 18), start >= 1,
//       end >= start — is the interval, what stands in front is the name; `name:start` runs to the end of the sequence
//   G3  what stands behind the colon is no such interval (or there is no colon): the whole string is the name
//   G4  coordinates are 1-based and closed
//   G5  the empty string, or a name the index does not hold: an error that names the region
//
// Planner (the UCSC binning scheme of the tabix paper: min_shift 14, depth 5)
//   P1  the region becomes zero-based half-open [s - 1, e), e clamped to 2^29
//   P2  the chunks of every bin of reg2bins(s - 1, e) are collected; pseudo-bin 37450 holds metadata and is skipped
//   P3  min_off = ioff[min((s - 1) >> 14, n_intv - 1)], 0 when the reference has no linear index
//   P4  chunks whose end is <= min_off are dropped
//   P5  the rest is sorted by begin (then end)
//   P6  a chunk is merged into its predecessor when next.begin <= cur.end — the only merge rule
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "exon_gpu.h"

namespace exg {
namespace tabix {

static constexpr uint32_t kPseudoBin = 37450;
static constexpr int64_t kMaxPos = (int64_t)1 << 29;  // what five levels over 16 KiB windows address
static constexpr int64_t kUnbounded = INT64_MAX;

struct Bin {
    uint32_t id;
    uint64_t first_chunk, n_chunks;  // in Reference::chunks
};
struct Reference {
    std::string name;
    std::vector<Bin> bins;
    std::vector<exg_virtual_chunk> chunks;
    std::vector<uint64_t> ioff;  // the linear index: a virtual offset per 16 KiB window
};
struct Index {
    int32_t format = 0, col_seq = 0, col_beg = 0, col_end = 0, meta = 0, skip = 0;
    std::vector<Reference> refs;
    bool has_no_coor = false;
    uint64_t n_no_coor = 0;
};

// the inflated bytes of a .tbi; false + *err: not an index this reader takes (truncated, a count that the bytes do not hold,
// format != 2).  Never reads outside [d, d + n).
bool parse_index(const uint8_t *d, uint64_t n, Index *out, std::string *err);

struct Region {
    uint32_t ref_id = 0;
    std::string name;
    int64_t start = 1, end = kUnbounded;  // 1-based, closed
};
// G1 .. G5 against the names of `idx`
bool parse_region(const Index &idx, const std::string &text, Region *out, std::string *err);

// the bins that may hold a feature overlapping zero-based half-open [beg, end), 0 <= beg < end <= 2^29
void reg2bins(int64_t beg, int64_t end, std::vector<uint32_t> *out);

// P1 .. P6
void plan(const Index &idx, const Region &region, std::vector<exg_virtual_chunk> *out);

}  // namespace tabix
}  // namespace exg
