// exg_rd_region.hpp — reader level of vcf_query (exg_open_region): the plan a region reader keeps — the resolved region, the
// chunks of the tabix planner (exg_tabix.hpp) and the member ranges they come to —, the producer that turns those ranges into a
// decoded stream of VCF text in front of the VCF reader, and the launch of the region predicate (exg_vcf_region.hip) behind
// every scan.
//
// From chunks to member ranges.  A chunk (begin, end) covers the members from begin >> 16 through end >> 16, the last one only
// when end & 0xFFFF > 0.  Ranges that overlap or are adjacent are merged; a range starts at the in-member offset begin & 0xFFFF
// of its earliest chunk, which the index guarantees to be a line start.
// Ownership of lines.  A range owns the lines that START in its members; the line that crosses out of its last member is
// completed from the member(s) behind it.  Ranges are disjoint, so no row appears twice; what a range holds beyond the region is
// harmless: the predicate decides which rows leave.
#pragma once
#include <atomic>
#include <memory>
#include <string>
#include <vector>

#include "exg_rd_source.hpp"
#include "exg_tabix.hpp"

namespace exg_rd {

struct MemberRange {
    uint64_t c_begin, c_end;  // file bytes [c_begin, c_end): whole BGZF members
    uint32_t skip;            // the range's first line begins this many bytes into its first member
};

struct RegionPlan {
    int device = 0;
    exg::tabix::Region region;
    std::vector<exg_virtual_chunk> chunks;
    std::vector<MemberRange> ranges;
    void *d_name = nullptr;  // the region's reference name in device memory (pooled)
    size_t d_name_bytes = 0;
    std::atomic<uint64_t> members{0};  // exg_reader_stats.reserved[0]
    ~RegionPlan();
};

// the chunks of a plan as member ranges of a file of n bytes (fd), every virtual offset checked against it: EXG_OK, or EXG_E_IO +
// *err for an offset outside the file, not on a member header, or inside a member beyond its inflated size
int region_member_ranges(int fd, uint64_t n, const std::vector<exg_virtual_chunk> &chunks, std::vector<MemberRange> *out, std::string *err);

// behind exg_open: <path>.tbi is read, inflated on the device and planned for `region`; r->region is set
int region_open(exg_reader *r, const char *region);

// the stream of a region reader: the header's text (the leading members, one at a time until a line that is not a header line
// begins), then every range's lines
std::unique_ptr<SegmentProducer> make_region_producer(exg_reader *r, int fd, uint64_t n, uint64_t target, const std::string &path, uint64_t reserve);

// exg_vcf_region_keep over the columns the scan of this batch left in HBM -> d_keep, on r->stream
int region_keep(exg_reader *r, const void *d_input, uint64_t payload_base, uint64_t n_rows, uint64_t *d_keep);

}  // namespace exg_rd
