// exg_rd_format.hpp — what a format's columns are, declared once: names, types and nullability (exg_schema_of, the Arrow
// stream's fields, the `filters` parser), how wide a column is at the chunk boundary, which columns are strings that point into
// the input, which are nested, which carry validity words a scan writes — and the format's sizing constants.  The reader's
// stages loop over this table; a comparison of `format` that is left in them chooses a code path (the BAM hand-off, FASTA's own
// pipeline, the VCF header and nested hand-over, the FASTQ phase guess, the scan's launch function), never a column fact.
// Host only, constexpr and free of any HIP include: under ASan + UBSan in tests/host_asan_driver.cpp.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/exon_gpu.h"

namespace exg_rd {

static constexpr int kMaxColumns = 12;  // (read_bed_file has twelve)

enum ParsedVector : uint8_t { kNotParsed = 0, kParsedPos, kParsedQual };

struct ColumnDesc {
    const char *name;
    int type;       // EXG_TYPE_*
    bool nullable;  // as the schema declares it
    // bytes a row of the column takes at the chunk boundary: 16 (a string_t), 8, 4; 0: the column is built by the nested emitter
    uint8_t elem;
    bool payload;   // its strings point into the input's bytes (they travel with the decoded text, or close up into a side buffer)
    bool nested;    // LIST / STRUCT: built from the field's text by the nested emitter (exg_vcf_nested.hpp)
    bool validity;  // the scan writes validity words for it: the reader holds a buffer, d_col_valid[c] (a nested column's own
                    // validity is the emitter's; VCF formats: the words say which lines have a FORMAT field at all)
    // the scan writes the field's text into d_cols[c] (the Arrow emitter and the nested one read it) and the parsed number into
    // a vector of the reader's own, named here: VCF pos -> d_pos, qual -> d_qual (exg_reader::parsed_vector)
    ParsedVector parsed;
};

struct FormatDesc {
    int format;              // EXG_FMT_*
    const char *name;        // exg_open_args.file_format, lower case
    const char *scan_label;  // the trace range of a batch's scan
    int n_columns;
    ColumnDesc col[kMaxColumns];
    // EXG_DEVICE_MEM_CAP_MB / mem_cap_div = the device batch: a batch in flight costs about ten times its bytes (segments queued
    // and being decoded, compressed windows, the scan's workspace and column vectors)
    uint32_t mem_cap_div;
    uint32_t bytes_per_row, bytes_per_row_worst;  // input bytes per provisioned row: realistic density first, the densest input after an overflow
    uint32_t tile_bytes;                          // a super-tile of the lean scan (sticky_algo)
    uint32_t line_index_arrays;                   // arrays of the general path's line index (exg_scan_workspace_bytes)
    // validity-sized buffers the reader holds beside those of its nullable columns and nothing reads (every format held two,
    // VCF's pair, from before validity was indexed by column): kept, so that a reader's footprint under a memory cap — what
    // mem_cap_div was measured with — is what it was
    uint32_t spare_validity;

    constexpr uint64_t mask(bool ColumnDesc::*flag) const {
        uint64_t m = 0;
        for (int c = 0; c < n_columns; c++)
            if (col[c].*flag) m |= 1ull << c;
        return m;
    }
    constexpr uint64_t mask_of_type(int type) const {
        uint64_t m = 0;
        for (int c = 0; c < n_columns; c++)
            if (col[c].type == type) m |= 1ull << c;
        return m;
    }
    constexpr uint64_t payload_mask() const { return mask(&ColumnDesc::payload); }
    constexpr uint64_t nested_mask() const { return mask(&ColumnDesc::nested); }
    constexpr uint64_t nullable_mask() const { return mask(&ColumnDesc::nullable); }
    constexpr uint64_t validity_mask() const { return mask(&ColumnDesc::validity); }
    // flat VARCHAR columns (a string_t per row at the chunk boundary)
    constexpr uint64_t string_mask() const {
        uint64_t m = 0;
        for (int c = 0; c < n_columns; c++)
            if (col[c].elem == 16) m |= 1ull << c;
        return m;
    }
    // bytes a row of column c takes in d_cols[c], as the scan writes it
    constexpr uint32_t scan_elem(int c) const { return col[c].nested || col[c].parsed != kNotParsed ? 16u : col[c].elem; }
};

// the kind of a column for the `filters` parser (exg_filter.hpp FilterColumn): 'x' is refused by it, like in new_reader
constexpr char filter_kind(const ColumnDesc &d) {
    return d.type == EXG_TYPE_BIGINT ? 'l' : d.type == EXG_TYPE_INTEGER ? 'i' : d.type == EXG_TYPE_FLOAT ? 'f' : d.type == EXG_TYPE_VARCHAR ? 'u' : 'x';
}

namespace format_detail {
// one column of each sort: {name, type, nullable, elem, payload, nested, validity, parsed}
constexpr ColumnDesc str(const char *name, bool nullable, bool payload = true) { return {name, EXG_TYPE_VARCHAR, nullable, 16, payload, false, nullable, kNotParsed}; }
constexpr ColumnDesc i64(const char *name, bool nullable) { return {name, EXG_TYPE_BIGINT, nullable, 8, false, false, nullable, kNotParsed}; }
constexpr ColumnDesc i32(const char *name, bool nullable) { return {name, EXG_TYPE_INTEGER, nullable, 4, false, false, nullable, kNotParsed}; }
// a flat FLOAT the scan writes as a number, with validity words (VCF's qual is not one: its number lands in a parsed vector)
constexpr ColumnDesc f32(const char *name, bool nullable) { return {name, EXG_TYPE_FLOAT, nullable, 4, false, false, nullable, kNotParsed}; }
constexpr ColumnDesc vcf_nested(const char *name, int type, bool validity = false) { return {name, type, true, 0, true, true, validity, kNotParsed}; }

// (inline: one table for the whole library, so that the addresses format_desc hands out are the same in every unit)
inline constexpr FormatDesc kFormats[] = {
    // `id` pinned by test_fasta_scan.test:34-37, order + NULL description by test_fasta_copy.test:75-80.  The sequences are joined
    // on the device and travel as that: their strings do not point into the input
    // (rows: a record under 16 bytes would be unusual; the densest is ">a\n" minus LF.  Four line-index arrays)
    {EXG_FMT_FASTA, "fasta", "exg: scan fasta batch", 3, {str("id", false), str("description", true), str("sequence", false, /*payload=*/false)},
     32, 16, 2, 2u * 16384u, 4, 1},
    // order pinned by test_fastq_scan.test:35-41; names as exon 0.2.6 registers them
    // (24: with 20 a single-member gzip under a 16 MiB cap peaked between 15.4 and 17.3 MB depending on how far the decoder thread
    // happened to run ahead of the scan — the first round's symbol buffer is sized for the worst ratio.  Per input byte a scan
    // provisions 16 B x columns / 32 of column vectors; a compressed input adds up to four segments and two compressed windows)
    // (rows: a record under 32 bytes would be unusual; the densest is "@\n\n+\n" = 5 bytes)
    {EXG_FMT_FASTQ, "fastq", "exg: scan fastq batch", 4,
     {str("name", false), str("description", true), str("sequence", false), str("quality_scores", false)}, 24, 32, 5, 3u * 16384u, 1, 1},
    // test_vcf_record_scan.test:10-19: alt is a LIST, info a STRUCT (module.cpp:126-147 maps exon's Arrow schema); the trees of the
    // nested columns come from the header (nested_schema).  pos / qual leave as numbers
    // (64: 16 B x (9 columns + POS + QUAL) / 16 of column vectors per input byte.  Rows: a line under 16 bytes would be unusual; the
    // densest input is blank lines)
    {EXG_FMT_VCF, "vcf", "exg: scan vcf batch", 9,
     {str("chrom", false), {"pos", EXG_TYPE_BIGINT, false, 8, false, false, false, kParsedPos}, vcf_nested("id", EXG_TYPE_LIST), str("ref", false),
      vcf_nested("alt", EXG_TYPE_LIST), {"qual", EXG_TYPE_FLOAT, true, 4, false, false, true, kParsedQual}, vcf_nested("filter", EXG_TYPE_LIST),
      vcf_nested("info", EXG_TYPE_STRUCT), vcf_nested("formats", EXG_TYPE_LIST, /*validity=*/true)},
     64, 16, 1, 2u * 16384u, 1, 0},
    // order pinned by test_bam_record_scan.test:5-17, names by test_sam_record_scan.test:6; the types are what exon 0.2.x is recalled
    // to declare ([RECALLED]).  The strings are produced into a side buffer (or point into the reference names):
    // none into the input
    // (32: segments as for the text formats, a workspace of ~0.8 B, a side buffer of ~1.25 B and ~2 B of vectors per decoded byte.
    // The workspace and the side buffer are BamState's own, and the reader's column vectors are provisioned with BAM's own sizing
    // — exg_rd_bam.cpp —: the sizing fields behind the divisor are not read for BAM and hold 1, like a format there is none of)
    {EXG_FMT_BAM, "bam", "exg: scan bam batch", EXG_BAM_COLUMNS,
     {str("name", false, false), i32("flag", false), str("reference", true, false), i32("start", true), i32("end", true),
      str("mapping_quality", true, false), str("cigar", false, false), str("mate_reference", true, false), str("sequence", false, false),
      str("quality_score", false, false)},
     32, 1, 1, 1, 1, 0},
    // order pinned by test_bed_io.test:4-18; names and types as exon 0.2.6 is recalled to declare them ([RECALLED])
    // (256: 9 B of vectors + 1.5 B of workspace per byte of an input slot, two slots, and a slot is a batch + 1 MiB of prefetch
    // slack: measured 17.0 MiB under a 16 MiB cap with batches of 256 KiB — a quarter of VCF's batch stays under it)
    {EXG_FMT_BED, "bed", "exg: scan bed batch", EXG_BED_COLUMNS,
     {str("reference_sequence_name", false), i64("start", false), i64("end", false), str("name", true), i64("score", true), str("strand", true),
      i64("thick_start", true), i64("thick_end", true), str("color", true), i64("block_count", true), str("block_sizes", true),
      str("block_starts", true)},
     256, 16, 1, 2u * 16384u, 1, 2},
    // BAM's ten columns in BAM's order, with its names, types and nullability (test_sam_record_scan.test:6-17 pins a full row);
    // every string is a slice of the input: no side buffer
    // (128: ~2 B of vectors — 124 B a row, a row per 64 bytes — and ~0.5 B of workspace per byte of an input slot, two slots, a
    // slot a batch + 1 MiB of prefetch slack: measured 6.98 MiB under a 16 MiB cap with batches of 128 KiB
    // (test_sam_gpu.py::test_reader_memory_cap prints it).  Rows: a line under 64 bytes would be unusual; the
    // densest valid line is eleven one-byte fields: 21 bytes + LF)
    {EXG_FMT_SAM, "sam", "exg: scan sam batch", EXG_SAM_COLUMNS,
     {str("name", false), i32("flag", false), str("reference", true), i32("start", true), i32("end", true), str("mapping_quality", true),
      str("cigar", false), str("mate_reference", true), str("sequence", false), str("quality_score", false)},
     128, 64, 22, 2u * 16384u, 1, 0},
    // test_gtf_scan.test:6-16 pins a row; names, types and nullability as INTEGRATION.md states them.  The scan leaves the ninth
    // field as one string per row; `attributes` is built from it behind the row selection (exg_gtf_attributes) and leaves as a MAP
    // whose keys and values point into the input
    // (128: SAM's budget — ~1.5 B of vectors (92 B a row, a row per 64 bytes), ~0.5 B of workspace and the row map's scratch per byte
    // of an input slot, two slots, a slot a batch + 1 MiB of prefetch slack; the attributes' children are a batch's own pooled
    // scratch, ~1.3 B per byte of attribute text (tests/test_gtf_gpu.py::test_reader_memory_cap prints the peak).  Rows: the scan
    // numbers rows by lines — a feature line under 64 bytes would be unusual, the densest line is `#` + LF)
    {EXG_FMT_GTF, "gtf", "exg: scan gtf batch", EXG_GTF_COLUMNS,
     {str("seqname", false), str("source", false), str("type", false), i64("start", false), i64("end", false), f32("score", true), str("strand", true),
      str("frame", true), {"attributes", EXG_TYPE_MAP, false, 0, true, true, false, kNotParsed}},
     128, 64, 2, 2u * 16384u, 1, 0},
};
constexpr int kNFormats = (int)(sizeof kFormats / sizeof kFormats[0]);
inline constexpr FormatDesc kNoFormat = {0, "", "", 0, {}, 1, 1, 1, 1, 1, 0};

// the place of EXG_FMT_* `format` in kFormats (-1: none)
constexpr int index_of(int format) {
    for (int k = 0; k < kNFormats; k++)
        if (kFormats[k].format == format) return k;
    return -1;
}
constexpr const FormatDesc &find(int format) { return index_of(format) < 0 ? kNoFormat : kFormats[index_of(format)]; }

// the type tree of a flat column is the column itself: one exg_type leaf per table entry (exg_schema.tree; the trees of the
// nested VCF columns come from the file's header: nested_schema)
struct FlatTrees {
    exg_type t[kNFormats][kMaxColumns];
};
constexpr FlatTrees flat_trees() {
    FlatTrees r = {};
    for (int k = 0; k < kNFormats; k++)
        for (int c = 0; c < kFormats[k].n_columns; c++) r.t[k][c] = {kFormats[k].col[c].type, kFormats[k].col[c].nullable, kFormats[k].col[c].name, 0, nullptr};
    return r;
}
inline constexpr FlatTrees kFlatTrees = flat_trees();
// MAP(VARCHAR, VARCHAR): LIST's layout over a STRUCT of key and value (GTF attributes)
inline constexpr exg_type kMapKeyValue[2] = {{EXG_TYPE_VARCHAR, 0, "key", 0, nullptr}, {EXG_TYPE_VARCHAR, 0, "value", 0, nullptr}};
inline constexpr exg_type kMapEntries[1] = {{EXG_TYPE_STRUCT, 0, "entries", 2, kMapKeyValue}};
inline constexpr exg_type kGtfAttributes = {EXG_TYPE_MAP, 0, "attributes", 1, kMapEntries};

// the masks the stages used to spell as literals
static_assert(find(EXG_FMT_FASTQ).payload_mask() == 0xF && find(EXG_FMT_FASTQ).string_mask() == 0xF, "FASTQ: four strings into the input");
static_assert(find(EXG_FMT_FASTA).payload_mask() == 0x3 && find(EXG_FMT_FASTA).string_mask() == 0x7, "FASTA: id and description point into the input");
static_assert(find(EXG_FMT_VCF).payload_mask() == 0x1DD && find(EXG_FMT_VCF).nested_mask() == 0x1D4, "VCF: all but pos / qual; id alt filter info formats");
static_assert((find(EXG_FMT_VCF).string_mask() | find(EXG_FMT_VCF).nested_mask()) == 0x1DD && find(EXG_FMT_VCF).string_mask() == 0x9, "VCF: chrom and ref are flat");
static_assert(find(EXG_FMT_VCF).validity_mask() == 0x120 && find(EXG_FMT_VCF).nullable_mask() == 0x1F4, "VCF: the scan writes qual's and formats' validity");
static_assert(find(EXG_FMT_BED).payload_mask() == 0xD29 && find(EXG_FMT_BED).string_mask() == 0xD29, "BED: the VARCHAR columns 0, 3, 5, 8, 10, 11");
static_assert(find(EXG_FMT_BED).validity_mask() == 0xFF8 && find(EXG_FMT_BED).mask_of_type(EXG_TYPE_BIGINT) == 0x2D6, "BED: columns 3..11 are nullable, six are BIGINT");
static_assert(find(EXG_FMT_BAM).mask_of_type(EXG_TYPE_INTEGER) == 0x1A && find(EXG_FMT_BAM).nullable_mask() == 0xBC, "BAM: flag start end; reference start end mapping_quality mate_reference");
static_assert(find(EXG_FMT_BAM).payload_mask() == 0 && find(EXG_FMT_BAM).validity_mask() == 0xBC, "BAM: no string points into the input");
static_assert(find(EXG_FMT_SAM).payload_mask() == 0x3E5 && find(EXG_FMT_SAM).string_mask() == 0x3E5, "SAM: all seven VARCHAR columns point into the input");
static_assert(find(EXG_FMT_SAM).mask_of_type(EXG_TYPE_INTEGER) == 0x1A && find(EXG_FMT_SAM).nullable_mask() == 0xBC && find(EXG_FMT_SAM).validity_mask() == 0xBC, "SAM: BAM's schema");
static_assert(find(EXG_FMT_FASTQ).validity_mask() == 0x2 && find(EXG_FMT_FASTA).validity_mask() == 0x2, "description");
static_assert(find(EXG_FMT_GTF).payload_mask() == 0x1C7 && find(EXG_FMT_GTF).string_mask() == 0xC7 && find(EXG_FMT_GTF).nested_mask() == 0x100, "GTF: five flat strings and the attributes point into the input");
static_assert(find(EXG_FMT_GTF).validity_mask() == 0xE0 && find(EXG_FMT_GTF).nullable_mask() == 0xE0, "GTF: score, strand and frame are nullable");
static_assert(find(EXG_FMT_GTF).mask_of_type(EXG_TYPE_BIGINT) == 0x18 && find(EXG_FMT_GTF).mask_of_type(EXG_TYPE_FLOAT) == 0x20 && find(EXG_FMT_GTF).scan_elem(5) == 4, "GTF: start and end are BIGINT, score a flat FLOAT");
}  // namespace format_detail

// the description of EXG_FMT_* `format` (an unknown one: no columns)
inline const FormatDesc &format_desc(int format) { return format_detail::find(format); }
// ... and the exg_type leaf of its flat column c
inline const exg_type *flat_tree(int format, int c) { return &format_detail::kFlatTrees.t[format_detail::index_of(format)][c]; }
// ... the tree of GTF's attributes column
inline const exg_type *gtf_attributes_tree() { return &format_detail::kGtfAttributes; }
// ... of a file_format spelled in lower case (NULL: not one of them)
inline const FormatDesc *format_named(const char *lower) {
    // ("sam" is not answered here: exg_open takes it in a branch of its own, where it was refused by name until the tokeniser was
    // built, and checks there that the file is text — a BAM file handed over as "sam" is still refused)
    for (const FormatDesc &f : format_detail::kFormats)
        if (f.format != EXG_FMT_SAM && strcmp(f.name, lower) == 0) return &f;
    return nullptr;
}

}  // namespace exg_rd
