// exg_rd_bam.hpp — read_bam_file_records at the reader level (exg_rd_bam.cpp)
#pragma once
#include "exg_rd_internal.hpp"

namespace exg_rd {
// the current file's decoded stream has been opened (r->src): reads the BAM header from its front; file_pos = the first record
int bam_open_file(exg_reader *r);
// next_batch for a BAM file: the records that lie completely inside the next decoded bytes -> r->batch
int bam_next_batch(exg_reader *r, bool count_only, uint64_t *n_records_out);
// exg_reader_stats: tiles of all batches so far and how many of them were walked a second time
void bam_stats(exg_reader *r, uint64_t *tiles, uint64_t *rewalked);
}  // namespace exg_rd
