/*
 * exon_gpu.h — C-ABI of the MI355X-native record-scan engine (libexon_gpu.so).
 *
 * Drop-in boundary for ONE path of wheretrue/exon-duckdb: the read_fasta /
 * read_fastq / read_vcf_file_records table functions that tokenise raw file
 * bytes into DuckDB DataChunks.  Plain C, plain pointers and sizes; no torch,
 * no HIP and no DuckDB types appear in any signature.
 *
 * Three layers, lowest first:
 *
 *   (1) exg_*_scan  — device level.  Input bytes are already resident in HBM;
 *       output column vectors (arrays of 16-byte duckdb::string_t + validity
 *       words) are written to HBM.  This is the hot path bench.py measures.
 *       Replaces the per-batch work of the reference's Rust side:
 *       exon `BatchReader::read_batch` + noodles line readers + Arrow builders
 *       (external crates, reached through rust/src/arrow_reader.rs:116-153)
 *       and the Arrow->DataChunk conversion at
 *       exon/src/exon/arrow_table_function/module.cpp:257-294 (Scan).
 *
 *   (2) exg_open / exg_next_chunk — reader level.  File on the host ->
 *       pinned staging -> HBM -> kernels -> DataChunk-shaped host buffers.
 *       Replaces `new_reader` + the ArrowArrayStream it returns
 *       (exon/include/rust.hpp:41-46, rust/src/arrow_reader.rs:38-166).
 *
 *   (3) replacement_scan — same name, argument and result struct as the reference's FFI
 *       (exon/include/rust.hpp:11-13, :48), so the reference's ReplacementScan glue
 *       (module.cpp:320-382) binds to it unchanged; and `new_reader` (exon/include/rust.hpp:41-46),
 *       the reference's own entry point: an Arrow C stream with the reference's schema, built on the
 *       device (INTEGRATION.md also shows the binding that replaces its two call sites,
 *       module.cpp:98-102 and :239-243, with the faster chunk boundary exg_open).
 *
 * Error convention: every function returns 0 on success or a negative
 * EXG_E_* code; nothing throws across this boundary.  Parse errors found by a
 * kernel are reported through exg_scan_result (error_code > 0 = EXG_PE_*).
 */
#ifndef EXON_GPU_H
#define EXON_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 9 still: read_bed_file (EXG_FMT_BED, exg_bed_scan, EXG_PE_BED_*), the sequence scalars (exg_sequence_op,
 * EXG_SEQ_*, EXG_PE_SEQ_*), the alignment scores (exg_align_score, EXG_PE_ALIGN_TOO_LONG) and read_sam_file_records
 * (EXG_FMT_SAM, exg_sam_scan, EXG_PE_SAM_*), the CIGAR scalars (exg_cigar_op, EXG_CIGAR_*, EXG_PE_CIGAR_*) and the alignment
 * strings (exg_align_string; no new error code) and the GFF attributes (exg_gff_attributes, EXG_PE_GFF_ATTRIBUTES) are pure
 * additions — no existing struct, constant or entry point changed. */
#define EXG_ABI_VERSION 9

/* DuckDB v0.8.1 STANDARD_VECTOR_SIZE; the reference asks the Rust side for
 * batches of exactly this many rows (module.cpp:83, :233). */
#define EXG_VECTOR_SIZE 2048

/* ---- API status codes (negative) ---------------------------------------- */
#define EXG_OK 0
#define EXG_E_INVALID_ARG (-1)
#define EXG_E_NO_DEVICE (-2)   /* HIP runtime / GPU missing: the product path fails loudly */
#define EXG_E_HIP (-3)         /* a HIP call failed; see exg_last_error_message() */
#define EXG_E_IO (-4)
#define EXG_E_UNSUPPORTED (-5) /* e.g. xz: no device decoder, and there is no CPU fallback */
#define EXG_E_PARSE (-6)       /* reader level: a record failed to parse */
#define EXG_E_CAPACITY (-7)    /* output arrays too small */
#define EXG_E_NOMEM (-8)

/* ---- parse error codes (positive; exg_scan_result.error_code) ----------- */
/* Mirrors the io::Error cases of the noodles readers at the pinned versions
 * (rust/Cargo.lock:1991-2194); each is a named oracle test. */
#define EXG_PE_NONE 0
#define EXG_PE_FASTQ_NAME_PREFIX 1    /* line 1 of a record does not start with '@' */
#define EXG_PE_FASTQ_PLUS_PREFIX 2    /* line 3 of a record does not start with '+' */
#define EXG_PE_UNEXPECTED_EOF 3       /* file ends inside a record (before line 3) */
#define EXG_PE_INVALID_UTF8 4         /* a field is not valid UTF-8 */
#define EXG_PE_FASTA_MISSING_PREFIX 5 /* definition line does not start with '>' */
#define EXG_PE_FASTA_MISSING_NAME 6   /* '>' followed by whitespace / nothing */
#define EXG_PE_FASTA_EMPTY_DEF 7      /* empty definition line */
#define EXG_PE_VCF_MISSING_FIELD 8    /* data line with fewer than 8 tab-separated fields */
#define EXG_PE_VCF_BAD_POS 9          /* POS is not a decimal integer */
#define EXG_PE_VCF_BAD_QUAL 10        /* QUAL is neither '.' nor a float */
#define EXG_PE_VCF_NO_HEADER 11       /* no '#CHROM' header line */
#define EXG_PE_FIELD_TOO_LONG 12      /* a field exceeds 2^32-1 bytes (string_t length is u32) */
#define EXG_PE_VCF_INFO 13            /* an INFO value does not parse as the type its ##INFO line declares */
#define EXG_PE_VCF_FORMAT 14          /* a sample value does not parse as the type its ##FORMAT line declares */
#define EXG_PE_BAM_BLOCK_SIZE 15      /* BAM: block_size < 32 (the fixed fields alone are 32 bytes) */
#define EXG_PE_BAM_TRUNCATED 16       /* BAM: a record runs past the end of the stream */
#define EXG_PE_BAM_READ_NAME 17       /* BAM: l_read_name = 0, or the name is not NUL-terminated */
#define EXG_PE_BAM_REFERENCE_ID 18    /* BAM: refID / next_refID is not in [-1, n_ref) */
#define EXG_PE_BAM_FIELD_LENGTHS 19   /* BAM: the declared field lengths do not fit in block_size */
#define EXG_PE_BAM_CIGAR_OP 20        /* BAM: a CIGAR operation code above 8 */
#define EXG_PE_BAM_QUALITY 21         /* BAM: a quality byte above 93 (and the qualities are not all 0xFF = absent) */
#define EXG_PE_BED_FIELD_COUNT 22     /* BED: a line with a field count other than 3, 4, 5, 6, 7, 8, 9 or 12 */
#define EXG_PE_BED_REFERENCE_NAME 23  /* BED: empty reference sequence name */
#define EXG_PE_BED_POSITION 24        /* BED: start, end, thick_start, thick_end or block_count is not an integer in range */
#define EXG_PE_BED_SCORE 25           /* BED: score is neither `0` nor an integer in 1..1000 */
#define EXG_PE_BED_STRAND 26          /* BED: strand is not `+`, `-` or `.` */
#define EXG_PE_BED_COLOR 27           /* BED: color is neither `0` nor r,g,b with three decimals in 0..255 */
#define EXG_PE_BED_BLOCKS 28          /* BED: block_sizes / block_starts hold fewer than block_count integers */
/* (29 stays unassigned: it is what callers probe to see "unknown parse error") */
#define EXG_PE_SEQ_INVALID_CHARACTER 30 /* sequence scalars: a byte outside the function's alphabet */
#define EXG_PE_SEQ_LENGTH 31          /* translate_dna_to_aa: the length is not a multiple of 3 */
#define EXG_PE_SEQ_CODON 32           /* translate_dna_to_aa: three bytes that are not a codon over A, C, G, T */
#define EXG_PE_ALIGN_TOO_LONG 33      /* exg_align_score: |text| + |pattern| of a row exceeds max_pair_bytes */
/* (34 stays unassigned, like 29: callers probe it to see "unknown parse error") */
#define EXG_PE_SAM_FIELD_COUNT 35     /* SAM: a line with fewer than 11 tab-separated fields (an empty line among them) */
#define EXG_PE_SAM_EMPTY_FIELD 36     /* SAM: one of the eleven mandatory fields is empty */
#define EXG_PE_SAM_HEADER_LINE 37     /* SAM: a line that starts with '@' behind the header */
#define EXG_PE_SAM_FLAG 38            /* SAM: FLAG is not made of digits only, or above 65535 */
#define EXG_PE_SAM_POSITION 39        /* SAM: POS is not made of digits only, or above 2^31 - 1 */
#define EXG_PE_SAM_MAPQ 40            /* SAM: MAPQ is not made of digits only, or above 255 */
#define EXG_PE_SAM_CIGAR 41           /* SAM: CIGAR is neither `*` nor [digits, one of MIDNSHP=X]+ with lengths <= 2^28 - 1 */
#define EXG_PE_SAM_LENGTHS 42         /* SAM: SEQ and QUAL are both present and differ in length */
/* (43 stays unassigned, like 29 and 34: callers probe it to see "unknown parse error") */
#define EXG_PE_CIGAR_INVALID 44       /* CIGAR scalars: a row is not [digits, one of MIDNSHP=X]+ with lengths <= 2^28 - 1 */
#define EXG_PE_CIGAR_RANGE 45         /* extract_from_cigar: the leading and trailing insertions exceed the sequence */
/* (46 is unassigned) */
#define EXG_PE_BCF_RECORD_LENGTH 47   /* BCF: l_shared < 24 (the fixed fields alone are 24 bytes) */
#define EXG_PE_BCF_TRUNCATED 48       /* BCF: a record runs past the end of the stream */
#define EXG_PE_BCF_TYPE 49            /* BCF: a typed value of type 4, 6 or 8 .. 15, or no integer where a key / a length stands */
#define EXG_PE_BCF_RESERVED_VALUE 50  /* BCF: one of the reserved integer values (0x82 .. 0x87 and their wider forms), or a negative GT value */
#define EXG_PE_BCF_OVERRUN 51         /* BCF: a typed value runs past l_shared / l_indiv */
#define EXG_PE_BCF_CHROM 52           /* BCF: CHROM is not an index of the header's contig dictionary */
#define EXG_PE_BCF_DICT_INDEX 53      /* BCF: a FILTER / INFO / FORMAT key is not an index of the header's string dictionary */
#define EXG_PE_BCF_NO_ALLELE 54       /* BCF: n_allele = 0 (a record has at least REF) */
#define EXG_PE_BCF_SAMPLE_COUNT 55    /* BCF: n_sample differs from the header's sample count */
/* (56 stays unassigned, like 29, 34, 43 and 46: callers probe it to see "unknown parse error") */
#define EXG_PE_GTF_FIELD_COUNT 57     /* GTF: a line with fewer than 9 tab-separated fields (an empty line among them) */
#define EXG_PE_GTF_EMPTY_FIELD 58     /* GTF: seqname or type is empty */
#define EXG_PE_GTF_POSITION 59        /* GTF: start or end is not made of digits only, is 0 or above 2^63 - 1 */
#define EXG_PE_GTF_SCORE 60           /* GTF: score is neither `.` nor a float literal */
#define EXG_PE_GTF_STRAND 61          /* GTF: strand is not `+`, `-`, `?` or `.` */
#define EXG_PE_GTF_FRAME 62           /* GTF: frame is not `0`, `1`, `2` or `.` */
#define EXG_PE_GTF_ATTRIBUTES 63      /* GTF (exg_gtf_attributes): an entry without a value, an unterminated quote, a quote that does
                                       * not begin a value, or bytes behind a closing quote other than spaces and `;` */
/* (64 stays unassigned, like 29, 34, 43, 46 and 56: callers probe it to see "unknown parse error") */
#define EXG_PE_GFF_ATTRIBUTES 65      /* GFF (exg_gff_attributes, gff_parse_attributes): a segment between `;` that is not
                                       * key=value behind its trim — no `=`, no key, no value, a third piece — or an empty field */

/* ---- duckdb::string_t, bit-for-bit (v0.8.1 duckdb/common/types/string_type.hpp)
 * length <= 12: bytes inlined, zero padded.  Otherwise 4-byte prefix + pointer.
 * Rows that are NULL hold 16 zero bytes. */
typedef union exg_string_t {
    struct {
        uint32_t length;
        char prefix[4];
        uint64_t ptr; /* payload_base + byte offset of the field in the input */
    } pointer;
    struct {
        uint32_t length;
        char inlined[12];
    } inlined;
} exg_string_t;

#define EXG_INLINE_LENGTH 12

/* ---- formats ------------------------------------------------------------- */
#define EXG_FMT_FASTA 1
#define EXG_FMT_FASTQ 2
#define EXG_FMT_VCF 3
#define EXG_FMT_BAM 4 /* reader level + exg_bam_scan; the chunk boundary only (new_reader refuses it) */
#define EXG_FMT_BED 5 /* reader level + exg_bed_scan; the chunk boundary only (new_reader refuses it) */
#define EXG_FMT_SAM 6 /* reader level + exg_sam_scan; the chunk boundary only (new_reader refuses it) */
#define EXG_FMT_BCF 7 /* reader level (file_format "bcf": records become VCF lines on the device, exg_bcf_to_vcf, and take the
                       * VCF path from there: both boundaries, the schema of the file's own header) */
#define EXG_FMT_GTF 8 /* reader level + exg_gtf_scan / exg_gtf_attributes; the chunk boundary only (new_reader refuses it) */

/* ---- scan flags ------------------------------------------------------------ */
#define EXG_F_BOF 1u /* a line starts at d_input[0] (start of file, or a record-aligned batch) */
#define EXG_F_EOF 2u /* d_input[n_bytes-1] is the last byte of the file */
#define EXG_F_NO_STORE 4u /* COUNT(*) path: parse and validate every record, write no column (capacity ignored) */
#define EXG_F_ALL 7u      /* any other bit is refused (EXG_E_INVALID_ARG) */

/* result flags */
#define EXG_RF_NON_ASCII 1u /* a byte >= 0x80 was seen; the fields of the records around it were validated as UTF-8 */
#define EXG_RF_HEAD_UNRESOLVED 2u /* first owned record starts before d_input[0]: host must stitch */
#define EXG_RF_FALLBACK 4u  /* the fused kernels gave the launch up and the general kernels ran (no input shape does that any more:
                             * kept for EXG_ALGO_AUTO's gate) */
#define EXG_RF_CAPACITY 8u  /* more records than capacity_records: the surplus was not written */
#define EXG_RF_INDEX_OVERFLOW 16u /* general path: more lines than the workspace can index (enlarge d_workspace) */
#define EXG_RF_QUAL_RANGE 32u /* VCF: more QUAL literals of one launch needed the exact big-integer parser (> 19 digits astride a float
                                 rounding boundary) than its list holds (one per 32 bytes of input, at most 4096); the next was rejected */

#define EXG_RF_ROWS_SKIPPED 128u /* GTF: at least one line of the buffer gave no row (a `#` line): d_keep says which rows are features */
/* algorithm selector (exg_*_scan_args.algo) */
#define EXG_RF_REDO 64u     /* the lean scan marked super-tiles — a record / line that begins more than 1 KiB in front of the 16 KiB
                             * half it ends in (long reads, multi-sample VCF), more lines in a half than its list holds (reads
                             * below ~45 bp), or a byte >= 0x80 (UTF-8 validation) — and the any-shape run behind it redid them: the output is complete; a caller
                             * with more batches of the same input does better with EXG_ALGO_FUSED_FULL from here on */
#define EXG_ALGO_AUTO 0
#define EXG_ALGO_MULTIPASS 1 /* count -> scan -> index -> fields: 4 launches, reads the input ~3x */
#define EXG_ALGO_FUSED 2     /* single pass: the lean scan, then the any-shape scan over the super-tiles the lean one marked */
#define EXG_ALGO_FUSED_FULL 3 /* single pass: the any-shape scan alone (any record length / line density; 17 % below the lean scan
                               * on 150 bp reads: 2.65 against 2.27 ms per 10 GB) */
#define EXG_ALGO_FUSED_INDEX 4 /* exg_vcf_scan only — wide lines (cohort VCFs: hundreds of bytes to 10 kB a line): the any-shape scan
                               * only notes where every line ends (8 bytes a line, in the workspace), the rows are parsed by a
                               * kernel of their own behind it, a thread per line.  Same rows, flags and errors as
                               * EXG_ALGO_FUSED_FULL; slower than it on short lines */

/* Written by the device (64 bytes, 8-byte aligned), copied back by exg_fetch_result. */
typedef struct exg_scan_result {
    uint64_t n_records;      /* records owned by this buffer (end at offset >= lead) */
    uint64_t n_lines;        /* '\n' count in [lead, n_bytes) (+1 for an unterminated last line at EOF) */
    uint64_t consumed_bytes; /* offset just past the last complete owned record */
    uint64_t error_offset;   /* byte offset (in d_input) of the first failing line; ~0 if none */
    uint64_t error_record;   /* index (within this buffer's output) of the first failing record */
    uint32_t error_code;     /* EXG_PE_* */
    uint32_t flags;          /* EXG_RF_* */
    uint64_t payload_bytes;  /* FASTA: bytes written to the compacted sequence payload */
    uint64_t redo_tiles;     /* EXG_RF_REDO: super-tiles (FASTQ: 48 KiB, VCF: 32 KiB of input each) the any-shape run redid behind the
                              * lean scan — few: the odd long read in a short-read file, cheaper redone than scanned any-shape
                              * throughout; most of them: an input of that shape (EXG_ALGO_FUSED_FULL from here on) */
} exg_scan_result;

/* FASTQ: 4 VARCHAR columns name, description, sequence, quality_scores
 * (order pinned by test/sql/exondb-release-with-deb-info/test_fastq_scan.test:35-41). */
typedef struct exg_fastq_scan_args {
    const void *d_input;       /* device pointer, 16-byte aligned, readable up to round_up(n_bytes,16) */
    uint64_t n_bytes;          /* halo + shard */
    uint64_t lead;             /* halo: records whose last line ends before this offset belong to the previous shard */
    uint64_t first_line_index; /* number of '\n' in the file before d_input[lead] (gives the 4-line phase) */
    uint64_t payload_base;     /* string_t.ptr = payload_base + offset in d_input */
    uint32_t flags;            /* EXG_F_* */
    uint32_t algo;             /* EXG_ALGO_* */
    exg_string_t *d_name;      /* device, capacity_records entries each */
    exg_string_t *d_description;
    exg_string_t *d_sequence;
    exg_string_t *d_quality;
    uint64_t *d_description_validity; /* device, ceil(capacity/64) words, bit r = row r valid */
    uint64_t capacity_records;
    void *d_workspace; /* device, exg_scan_workspace_bytes(EXG_FMT_FASTQ, n_bytes), 256-byte aligned (any hipMalloc pointer is) */
    uint64_t workspace_bytes;
    exg_scan_result *d_result; /* device, 64 bytes */
    void *stream;              /* hipStream_t (NULL = default stream) */
} exg_fastq_scan_args;

/* VCF: one row per data line; the 8 fixed columns (+ the FORMAT/samples rest)
 * as raw field slices, POS parsed to int64, QUAL to float32. */
typedef struct exg_vcf_scan_args {
    const void *d_input;
    uint64_t n_bytes;
    uint64_t lead;
    uint64_t payload_base;
    uint32_t flags;
    uint32_t algo;
    exg_string_t *d_fields[9]; /* chrom,pos,id,ref,alt,qual,filter,info,formats(rest) — any may be NULL (projection) */
    int64_t *d_pos;            /* parsed POS, may be NULL */
    float *d_qual;             /* parsed QUAL, may be NULL */
    uint64_t *d_qual_validity; /* '.' => NULL */
    uint64_t *d_formats_validity;
    uint64_t capacity_records;
    void *d_workspace;
    uint64_t workspace_bytes;
    exg_scan_result *d_result;
    void *stream;
} exg_vcf_scan_args;

/* FASTA: id, description, sequence.  The sequence is the concatenation of the
 * record's lines with terminators removed, so it is materialised in a
 * compacted payload buffer (d_seq_payload); id/description point into d_input.
 * A buffer begins with a record (lead = 0, EXG_F_BOF).  Without EXG_F_EOF it is a batch of a longer input: the last
 * record in it is still open (its sequence may go on behind the buffer) and is left to the next batch — n_records,
 * the columns and payload_bytes are those of the records in front of it, consumed_bytes = where its '>' line begins
 * (0 records when the buffer holds only that one: widen the batch — a FASTA record can be as long as the input). */
typedef struct exg_fasta_scan_args {
    const void *d_input;
    uint64_t n_bytes;
    uint64_t lead;
    uint64_t payload_base;     /* for id/description */
    uint64_t seq_payload_base; /* string_t.ptr of sequences = seq_payload_base + offset in d_seq_payload */
    uint32_t flags;
    uint32_t algo;
    exg_string_t *d_id;
    exg_string_t *d_description;
    exg_string_t *d_sequence;
    uint64_t *d_description_validity;
    uint8_t *d_seq_payload; /* device, >= n_bytes */
    uint64_t capacity_records;
    void *d_workspace;
    uint64_t workspace_bytes;
    exg_scan_result *d_result;
    void *stream;
} exg_fasta_scan_args;

/* BAM (SAM v1 §4.2): the DECODED bytes of a BAM file behind its header — block_size-prefixed binary records without a
 * delimiter — in HBM, d_input[0] being a record start.  Ten columns (the reference's read_bam_file_records, order pinned by
 * test_bam_record_scan.test:5-17; types as exon 0.2.x is recalled to declare them — INTEGRATION.md):
 *   0 name VARCHAR, 1 flag INTEGER, 2 reference VARCHAR?, 3 start INTEGER?, 4 end INTEGER?, 5 mapping_quality VARCHAR?,
 *   6 cigar VARCHAR, 7 mate_reference VARCHAR, 8 sequence VARCHAR, 9 quality_score VARCHAR
 * Three of them do not exist as text in the file and are PRODUCED into a side buffer (d_side): the sequence (4-bit packed),
 * the qualities (raw bytes, +33) and the CIGAR (uint32 operations, rendered as <len><op>); the name is copied there too.
 * A string_t of more than 12 bytes points at side_base + its offset in d_side; reference / mate_reference point into the
 * table of reference names (ref_names_base + d_ref_offsets[refID]).  The CIGAR is rendered as stored: the CG:B,I
 * convention for more than 65535 operations is not resolved.  Trailing aux fields are skipped unread.
 *
 * Records are found by speculation over fixed tiles (a plausible record header with a plausible successor) and a stitch
 * that accepts a tile only when the chain from d_input[0] lands exactly on its speculated entry; every other tile the chain
 * enters is walked again from the true entry (tiles_rewalked).  The rows are exactly the serial chain's, whatever the
 * bytes look like.
 *
 * Without EXG_F_EOF the tail behind the last complete record is left to the next batch (consumed_bytes); with it, a tail is
 * EXG_PE_BAM_TRUNCATED.  EXG_F_NO_STORE: records are found and validated, nothing else is written.  The rows in front of the
 * first failing record are produced (n_records = its ordinal).  Synchronises the stream (twice: the row count and the
 * side-buffer size come back to the host between the passes). */
typedef struct exg_bam_scan_result { /* 64 bytes, written by the device */
    uint64_t n_records;      /* rows produced: the complete records of the buffer, or those in front of the first error */
    uint64_t consumed_bytes; /* offset just past the last complete record (where the next batch begins) */
    uint64_t side_bytes;     /* bytes of d_side the rows need (> side_capacity with EXG_RF_CAPACITY: nothing was written) */
    uint64_t error_record;   /* ordinal (within this buffer) of the first failing record */
    uint64_t error_offset;   /* its byte offset in d_input */
    uint32_t error_code;     /* EXG_PE_BAM_* */
    uint32_t flags;          /* EXG_RF_CAPACITY: more records than capacity_records, or side_bytes > side_capacity */
    uint64_t tiles;          /* tiles of 32 KiB the buffer was cut into */
    uint64_t tiles_rewalked; /* tiles whose speculated entry was not the chain's: walked again from the true entry */
} exg_bam_scan_result;

#define EXG_BAM_COLUMNS 10
typedef struct exg_bam_scan_args {
    const void *d_input; /* device, any alignment */
    uint64_t n_bytes;
    uint32_t flags;      /* EXG_F_EOF | EXG_F_NO_STORE */
    int32_t n_ref;       /* references in the file's header */
    uint64_t columns;    /* bit c: produce column c (0 = all); every record is validated whatever is selected */
    const uint8_t *d_ref_names;    /* device: the reference names, closed up (no NULs) */
    const uint64_t *d_ref_offsets; /* device: n_ref + 1 offsets into d_ref_names */
    uint64_t ref_names_base;       /* string_t.ptr of a reference name = ref_names_base + its offset */
    void *d_columns[EXG_BAM_COLUMNS];      /* device: exg_string_t[capacity_records] (VARCHAR) / int32_t[] (INTEGER); NULL = not produced */
    uint64_t *d_validity[EXG_BAM_COLUMNS]; /* device: ceil(capacity / 64) words for columns 2, 3, 4, 5, 7 (when produced) */
    uint8_t *d_side;        /* device, side_capacity bytes */
    uint64_t side_capacity;
    uint64_t side_base;     /* string_t.ptr = side_base + offset in d_side */
    uint64_t capacity_records;
    void *d_workspace;      /* device, exg_scan_workspace_bytes(EXG_FMT_BAM, n_bytes), 256-byte aligned */
    uint64_t workspace_bytes;
    exg_bam_scan_result *d_result; /* device, 64 bytes */
    void *stream;
} exg_bam_scan_args;

/* BED (read_bed_file): one row per line, twelve columns (order pinned by test_bed_io.test:4-18; the value rules are
 * INTEGRATION.md's):
 *   0 reference_sequence_name VARCHAR, 1 start BIGINT (field 2 + 1), 2 end BIGINT, 3 name VARCHAR?, 4 score BIGINT?,
 *   5 strand VARCHAR?, 6 thick_start BIGINT? (field 7 + 1), 7 thick_end BIGINT?, 8 color VARCHAR?, 9 block_count BIGINT?,
 *   10 block_sizes VARCHAR?, 11 block_starts VARCHAR?
 * Every line of the input is a record (no header, no comments); a line has 3..9 or 12 tab-separated fields, the columns
 * behind its last field are NULL.  Strings are zero-copy slices of the input (payload_base + offset; up to 12 bytes
 * inlined): there is no side buffer.  A NULL value holds zeros (16 bytes / 8 bytes).  lead, flags and the result block
 * are exg_vcf_scan's: a line belongs to the buffer it ENDS in at an offset >= lead; EXG_RF_HEAD_UNRESOLVED when the first
 * owned line begins in front of d_input[0]; the rows in front of the first failing line are produced.
 * algo: EXG_ALGO_MULTIPASS is the general path (line index + a thread per line reading global memory);
 * EXG_ALGO_AUTO / EXG_ALGO_FUSED / EXG_ALGO_FUSED_FULL all run the single-pass any-shape scan (there is no lean instance);
 * EXG_ALGO_FUSED_INDEX is EXG_E_INVALID_ARG. */
#define EXG_BED_COLUMNS 12
typedef struct exg_bed_scan_args {
    const void *d_input; /* device pointer, 16-byte aligned, readable up to round_up(n_bytes,16) */
    uint64_t n_bytes;
    uint64_t lead;
    uint64_t payload_base;
    uint32_t flags;
    uint32_t algo;
    void *d_columns[EXG_BED_COLUMNS];      /* device: exg_string_t[capacity_records] for columns 0, 3, 5, 8, 10, 11; int64_t[] for 1, 2, 4,
                                            * 6, 7, 9.  NULL = not produced, still validated */
    uint64_t *d_validity[EXG_BED_COLUMNS]; /* device: ceil(capacity / 64) words for columns 3..11 (when produced) */
    uint64_t capacity_records;
    void *d_workspace; /* device, exg_scan_workspace_bytes(EXG_FMT_BED, n_bytes), 256-byte aligned */
    uint64_t workspace_bytes;
    exg_scan_result *d_result; /* device, 64 bytes */
    void *stream;
} exg_bed_scan_args;

/* SAM (read_sam_file_records): one row per alignment line, the ten columns of read_bam_file_records in the same order, with
 * the same names, types and nullability (test_sam_record_scan.test:6-17; the value rules are INTEGRATION.md's):
 *   0 name VARCHAR, 1 flag INTEGER, 2 reference VARCHAR?, 3 start INTEGER?, 4 end INTEGER?, 5 mapping_quality VARCHAR?,
 *   6 cigar VARCHAR, 7 mate_reference VARCHAR?, 8 sequence VARCHAR, 9 quality_score VARCHAR
 * The input holds alignment lines only: the header (the leading '@' lines) is skipped by the caller (the reader does it at
 * open).  A line has 11 or more tab-separated fields; fields 12 and up are not read.  Every string is a zero-copy slice of
 * the input (payload_base + offset; up to 12 bytes inlined): there is no side buffer.  mate_reference `=` is a string_t on
 * RNAME's bytes; mapping_quality points behind the field's leading zeros.  A NULL value holds zeros (16 bytes / 4 bytes).
 * lead, flags, algo and the result block are exg_bed_scan's: EXG_ALGO_MULTIPASS is the general path, EXG_ALGO_AUTO /
 * EXG_ALGO_FUSED / EXG_ALGO_FUSED_FULL all run the single-pass any-shape scan (there is no lean instance),
 * EXG_ALGO_FUSED_INDEX is EXG_E_INVALID_ARG. */
#define EXG_SAM_COLUMNS 10
typedef struct exg_sam_scan_args {
    const void *d_input; /* device pointer, 16-byte aligned, readable up to round_up(n_bytes,16) */
    uint64_t n_bytes;
    uint64_t lead;
    uint64_t payload_base;
    uint32_t flags;
    uint32_t algo;
    void *d_columns[EXG_SAM_COLUMNS];      /* device: exg_string_t[capacity_records] for columns 0, 2, 5, 6, 7, 8, 9; int32_t[] for 1, 3, 4.
                                            * NULL = not produced, still validated */
    uint64_t *d_validity[EXG_SAM_COLUMNS]; /* device: ceil(capacity / 64) words for columns 2, 3, 4, 5, 7 (when produced) */
    uint64_t capacity_records;
    void *d_workspace; /* device, exg_scan_workspace_bytes(EXG_FMT_SAM, n_bytes), 256-byte aligned */
    uint64_t workspace_bytes;
    exg_scan_result *d_result; /* device, 64 bytes */
    void *stream;
} exg_sam_scan_args;

/* GTF (read_gtf): one row per feature line, nine columns (test_gtf_scan.test:6-16 pins a row; the value rules are
 * INTEGRATION.md's):
 *   0 seqname VARCHAR, 1 source VARCHAR, 2 type VARCHAR, 3 start BIGINT, 4 end BIGINT, 5 score FLOAT?, 6 strand VARCHAR?,
 *   7 frame VARCHAR?, 8 attributes — here the RAW ninth field as one string_t per row (everything behind the eighth tab);
 *   exg_gtf_attributes turns that column into the MAP(VARCHAR, VARCHAR) children.
 * A line has nine tab-separated fields; a line whose first byte is `#` gives no row.  The scan numbers rows by LINES:
 * n_records, capacity_records and the row indices of the columns count every line of the buffer, comment lines included (their
 * slots are not written).  d_keep, one validity-style word array, says which rows are feature lines (bit r set); the result
 * flag EXG_RF_ROWS_SKIPPED says that at least one is not.  With EXG_F_NO_STORE d_keep is not written (the flag still is).
 * Strings are zero-copy slices of the input (payload_base + offset; up to 12 bytes inlined).  A NULL value holds zeros.
 * score takes VCF QUAL's literal grammar and exact rounding (a literal of more than 19 digits astride a rounding boundary is
 * decided by a fix-up kernel behind the scan; more than 1024 of them in one launch: EXG_PE_GTF_SCORE).
 * lead, flags, algo and the result block are exg_bed_scan's: EXG_ALGO_MULTIPASS is the general path, EXG_ALGO_AUTO /
 * EXG_ALGO_FUSED / EXG_ALGO_FUSED_FULL all run the single-pass any-shape scan, EXG_ALGO_FUSED_INDEX is EXG_E_INVALID_ARG.  The
 * general path's line index is provisioned for a line per 16 bytes: a buffer of denser lines (runs of `#` lines) reports
 * EXG_RF_INDEX_OVERFLOW there and wants a larger workspace; the single-pass scan takes any density. */
#define EXG_GTF_COLUMNS 9
typedef struct exg_gtf_scan_args {
    const void *d_input; /* device pointer, 16-byte aligned, readable up to round_up(n_bytes,16) */
    uint64_t n_bytes;
    uint64_t lead;
    uint64_t payload_base;
    uint32_t flags;
    uint32_t algo;
    void *d_columns[EXG_GTF_COLUMNS];      /* device: exg_string_t[capacity_records] for columns 0, 1, 2, 6, 7, 8; int64_t[] for 3, 4;
                                            * float[] for 5.  NULL = not produced, still validated */
    uint64_t *d_validity[EXG_GTF_COLUMNS]; /* device: ceil(capacity / 64) words for columns 5, 6, 7 (when produced) */
    uint64_t *d_keep;                      /* device: ceil(capacity / 64) words, bit r = row r is a feature line; required unless
                                            * EXG_F_NO_STORE */
    uint64_t capacity_records;
    void *d_workspace; /* device, exg_scan_workspace_bytes(EXG_FMT_GTF, n_bytes), 256-byte aligned */
    uint64_t workspace_bytes;
    exg_scan_result *d_result; /* device, 64 bytes */
    void *stream;
} exg_gtf_scan_args;

/* BCF 2.2 records -> the VCF data lines they stand for (VCF 4.3 spec section 6.3), on decoded bytes resident in HBM.
 * d_input begins at a record start (the caller has taken the header off).  The lines of all records that lie completely
 * inside the buffer are written to d_output in order, each ended by LF, closed up.  The two dictionaries of the file's header
 * are tables of {offset, length} pairs (uint32 each; length 0xFFFFFFFF: no such entry) into their bytes: the contigs, and the
 * IDs of the FILTER / INFO / FORMAT lines (PASS = 0).  gt_index: the string dictionary's index of `GT` (~0: none).
 * Rendering rules: INTEGRATION.md (BCF).  A float is rendered with nine significant digits in a spelling the VCF path's
 * float parser reads back to the same bits.
 * Records are found like BAM's (speculation per 32 KiB tile, stitch from byte 0: exactly the serial chain).  The first
 * record in error ends the output: the lines in front of it are written, then error_code / error_record / error_offset say
 * which.  error_code is the first error a reader meets going left to right through that record (fixed fields, ID, alleles,
 * FILTER, each INFO entry with its elements, the FORMAT fields' descriptors, then the samples in order), not the lowest code
 * and not the order the device happens to look in.  Output that does not fit: EXG_RF_CAPACITY, the lines of the records that fit are written (nothing behind the last
 * of them), consumed_bytes is where the next call begins and text_bytes_needed what all of them take.  Without EXG_F_EOF the
 * tail behind the last complete record is left to the next call; with it, a tail is EXG_PE_BCF_TRUNCATED.
 * Synchronises the stream (once: the row count comes back to the host between discovery and rendering). */
typedef struct exg_bcf_to_vcf_result { /* 64 bytes, written by the device */
    uint64_t n_records;         /* records rendered */
    uint64_t consumed_bytes;    /* offset just past the last rendered record (the tail is the caller's carry) */
    uint64_t text_bytes_needed; /* text of all complete records in front of the first error */
    uint64_t text_bytes;        /* text written to d_output */
    uint64_t error_record;      /* ordinal (within this buffer) of the first failing record */
    uint64_t error_offset;      /* its byte offset in d_input */
    uint32_t error_code;        /* EXG_PE_BCF_* (0 while records in front of the failing one did not fit) */
    uint32_t flags;             /* EXG_RF_CAPACITY */
    uint64_t tiles_rewalked;    /* tiles whose speculated entry was not the chain's */
} exg_bcf_to_vcf_result;

typedef struct exg_bcf_to_vcf_args {
    const void *d_input; /* device, any alignment */
    uint64_t n_bytes;
    uint32_t flags;      /* EXG_F_EOF */
    uint32_t n_samples;  /* the header's sample count */
    const uint8_t *d_contig_bytes;
    const uint32_t *d_contig_table; /* device: n_contigs x {offset, length} */
    uint32_t n_contigs;
    uint32_t n_strings;
    const uint8_t *d_string_bytes;
    const uint32_t *d_string_table; /* device: n_strings x {offset, length} */
    uint32_t gt_index;
    uint32_t reserved;
    uint8_t *d_output; /* device, output_capacity bytes */
    uint64_t output_capacity;
    void *d_workspace; /* device, exg_bcf_workspace_bytes(n_bytes, n_samples), 256-byte aligned */
    uint64_t workspace_bytes;
    exg_bcf_to_vcf_result *d_result; /* device, 64 bytes */
    void *stream;
} exg_bcf_to_vcf_args;

/* ---- library / device ------------------------------------------------------ */
int exg_abi_version(void);
/* Number of visible HIP devices, or EXG_E_NO_DEVICE. Does not initialise a context. */
int exg_device_count(void);
/* Thread-local message for the last failing call on this thread. */
const char *exg_last_error_message(void);
const char *exg_parse_error_string(uint32_t pe_code);

/* ---- (1) device level -------------------------------------------------------- */
uint64_t exg_scan_workspace_bytes(int format, uint64_t n_bytes);
/* Enqueue on args->stream; asynchronous. */
int exg_fastq_scan(const exg_fastq_scan_args *args);
int exg_vcf_scan(const exg_vcf_scan_args *args);
int exg_fasta_scan(const exg_fasta_scan_args *args);
/* Synchronises args->stream (see exg_bam_scan_args).  The 64-byte result comes back with exg_fetch_result, like the others'. */
int exg_bam_scan(const exg_bam_scan_args *args);
/* Enqueue on args->stream; asynchronous (the result through exg_fetch_result). */
int exg_bed_scan(const exg_bed_scan_args *args);
/* Enqueue on args->stream; asynchronous (the result through exg_fetch_result). */
int exg_sam_scan(const exg_sam_scan_args *args);
/* Enqueue on args->stream; asynchronous (the result through exg_fetch_result). */
int exg_gtf_scan(const exg_gtf_scan_args *args);
/* BCF records -> VCF lines (see exg_bcf_to_vcf_args).  Synchronises args->stream. */
uint64_t exg_bcf_workspace_bytes(uint64_t n_bytes, uint32_t n_samples);
int exg_bcf_to_vcf(const exg_bcf_to_vcf_args *args);
/* the 64-byte result block of exg_bcf_to_vcf, brought to the host (synchronises `stream`) */
int exg_bcf_result(const exg_bcf_to_vcf_result *d_result, void *stream, exg_bcf_to_vcf_result *out);
/* Synchronising copy of the 64-byte result to the host. */
int exg_fetch_result(const exg_scan_result *d_result, void *stream, exg_scan_result *out);
/* '\n' count of d_input[begin,end) into *d_count (device u64); used for the shard phase exchange. */
int exg_count_newlines(const void *d_input, uint64_t begin, uint64_t end, uint64_t *d_count, void *stream);
/* The first FASTA record start ('>' at the beginning of a line) at an offset in [begin, end) of d_bytes into *d_pos (device
 * u64; ~0 when there is none).  The byte in front of `begin` is read (begin = 0: at_bof says whether d_bytes[0] begins a
 * line).  What a shard of a compressed FASTA needs at its ends: a record belongs to the shard its '>' line begins in. */
int exg_fasta_find_record(const void *d_bytes, uint64_t begin, uint64_t end, int at_bof, uint64_t *d_pos, void *stream);
/* FASTQ 4-line phase of the first line that starts at or after `lead`, decided from local
 * structure ('@' on line 0, '+' on line 2 for 8 consecutive records).  *d_phase (device u32)
 * receives 0..3, or 0xFFFFFFFF when no or several phases fit (caller falls back to counting). */
int exg_fastq_guess_phase(const void *d_input, uint64_t n_bytes, uint64_t lead, uint32_t *d_phase, void *stream);
/* ABI 9: which scan to launch FIRST on an input, from a sample of its bytes on the HOST (the reader looks at the first MiB behind the
 * header it has mapped anyway; host only, no device is touched): EXG_ALGO_FUSED for ordinary shapes (150 bp reads, 50-byte VCF lines),
 * EXG_ALGO_FUSED_FULL where the lean scan would mark most super-tiles (records of ~1 KiB and more, lines denser than its list holds,
 * bytes >= 0x80), EXG_ALGO_FUSED_INDEX for VCF lines of >= 640 bytes.  Before round 6 a reader found this out from its first
 * batches' results: lean + redo, then the any-shape scan, then (cohort VCFs) the indexed one; a file of one batch never got its scan.
 * The result flags of every batch still correct the choice (exg_reader_stats.scan_algo). */
int exg_scan_algo_hint(int format, const void *sample, uint64_t n_bytes);

/* ---- quality_score_string_to_list on device-resident columns ----------------------------------------
 * Replaces the scalar function of exon/src/exon/fastq_functions/module.cpp:28-54 (one INTEGER per byte of the
 * string, value = (char)c - 33, `char` signed as on x86-64) for a VARCHAR column that is still in HBM — the
 * quality_scores column exg_fastq_scan just wrote.  Output is DuckDB's LIST(INTEGER) layout: one
 * list_entry_t {offset, length} per row + the child INTEGER vector.  NULL rows (16 zero bytes) give empty
 * entries; the list column's validity is the input column's validity. */
typedef struct exg_list_entry_t {
    uint64_t offset; /* first child value of the row */
    uint64_t length;
} exg_list_entry_t;
typedef struct exg_quality_list_args {
    const exg_string_t *d_strings; /* device, n_rows entries */
    uint64_t n_rows;
    const void *d_payload;       /* device bytes the non-inlined strings point into */
    uint64_t payload_base;       /* string_t.ptr - payload_base = byte offset in d_payload */
    exg_list_entry_t *d_entries; /* out: device, n_rows entries */
    int32_t *d_values;           /* out: device, 16-byte aligned, values_capacity entries */
    uint64_t values_capacity;
    uint64_t *d_total; /* out: device u64, number of child values; > values_capacity => entries and values untouched */
    void *d_workspace; /* device, exg_quality_list_workspace_bytes(n_rows) */
    uint64_t workspace_bytes;
    void *stream;
} exg_quality_list_args;
uint64_t exg_quality_list_workspace_bytes(uint64_t n_rows);
/* Enqueue on args->stream; asynchronous. */
int exg_quality_score_list(const exg_quality_list_args *args);

/* ---- sequence scalars on device-resident columns --------------------------------------------------------
 * The scalar functions of exon/src/exon/sequence_functions/module.cpp:30-370 for a VARCHAR column that is still in HBM
 * (the sequence column a scan just wrote).  The rules are stated once, in exon_duckdb_amd/csrc/exg_seqfn.hpp
 * ("Sequence and SAM-flag scalars"); reverse_complement is what the reference COMPUTES (A->C, T->G, C->A,
 * G->T, order kept), not what its name says.
 *
 * Input: exg_string_t[n_rows] as the scans leave it (up to 12 bytes inlined, longer strings at payload_base + offset in
 * d_payload at any alignment, a NULL row = 16 zero bytes); the output column's validity is the input's.  n_rows < 2^32 - 1.
 * String ops: one string_t per row in d_out_strings — up to 12 bytes inlined and zero padded, longer rows as
 * {length, 4-byte prefix, out_base + offset} with the out-of-line rows packed into d_out_payload in row order without
 * gaps: offset(i) = the sum of the output lengths of the rows j < i whose output is longer than 12, total_bytes = that sum
 * over all rows (a translate_dna_to_aa row counts length / 3, whatever else is wrong with it).  total_bytes > out_capacity:
 * EXG_RF_CAPACITY, neither output buffer is touched and no row is validated.  GC_CONTENT: one float per row, 0 for a NULL
 * or empty row, (float)count / (float)length in one IEEE division otherwise.
 * Errors: the lowest failing row wins, in it the length error of translate_dna_to_aa, else the leftmost bad byte / codon.
 * With an error the result block is exact and the output buffers are unspecified.  Deterministic: byte-identical outputs for
 * identical inputs.  No host round trip between the passes. */
#define EXG_SEQ_COMPLEMENT 1
#define EXG_SEQ_REVERSE_COMPLEMENT 2
#define EXG_SEQ_TRANSCRIBE 3
#define EXG_SEQ_REVERSE_TRANSCRIBE 4
#define EXG_SEQ_TRANSLATE 5
#define EXG_SEQ_GC_CONTENT 6
typedef struct exg_seq_result { /* 64 bytes, written by the device */
    uint64_t total_bytes;   /* bytes of d_out_payload the rows need (string ops); 0 for GC_CONTENT */
    uint64_t error_row;     /* lowest failing row */
    uint64_t error_offset;  /* byte offset in that row of the bad byte / codon (0 for the length error) */
    uint64_t error_length;  /* that row's length */
    uint32_t error_code;    /* 0, EXG_PE_SEQ_INVALID_CHARACTER, EXG_PE_SEQ_LENGTH or EXG_PE_SEQ_CODON */
    uint32_t flags;         /* EXG_RF_CAPACITY: total_bytes > out_capacity, no output was written */
    uint8_t error_bytes[4]; /* the byte, or the three bytes of the codon */
    uint8_t pad[20];
} exg_seq_result;
typedef struct exg_sequence_op_args {
    uint32_t op;                   /* EXG_SEQ_* */
    const exg_string_t *d_strings; /* device, 16-byte aligned, n_rows entries */
    uint64_t n_rows;
    const void *d_payload;         /* device bytes the non-inlined strings point into */
    uint64_t payload_base;         /* string_t.ptr - payload_base = byte offset in d_payload */
    exg_string_t *d_out_strings;   /* string ops, out: device, 16-byte aligned, n_rows entries */
    uint8_t *d_out_payload;        /* string ops, out: device, 16-byte aligned, out_capacity bytes */
    uint64_t out_capacity;
    uint64_t out_base;             /* out string_t.ptr = out_base + offset in d_out_payload */
    float *d_out_float;            /* GC_CONTENT, out: device, n_rows entries */
    void *d_workspace;             /* device, 8-byte aligned, exg_sequence_workspace_bytes(op, n_rows) */
    uint64_t workspace_bytes;
    exg_seq_result *d_result;      /* device, 64 bytes, 8-byte aligned */
    void *stream;
} exg_sequence_op_args;
uint64_t exg_sequence_workspace_bytes(uint32_t op, uint64_t n_rows);
/* Enqueue on args->stream; asynchronous. */
int exg_sequence_op(const exg_sequence_op_args *args);
/* Synchronising copy of the 64-byte result to the host.  error_code != 0: EXG_E_PARSE, and the thread's last error message
 * is the reference's text (`Invalid character in sequence: X`, `Invalid sequence length: N`, `Invalid codon: XYZ`)
 * followed by ` in row <r>`; *out is filled either way. */
int exg_sequence_result(const exg_seq_result *d_result, void *stream, exg_seq_result *out);

/* ---- gap-affine alignment scores on device-resident columns ---------------------------------------------
 * alignment_score / alignment_score_wfa_gap_affine of exon/src/exon/alignment_functions/module.cpp:264-329 for two VARCHAR
 * columns that are still in HBM.  The rules are stated once, in exon_duckdb_amd/csrc/exg_alignfn.hpp (INTEGRATION.md,
 * "Alignment scores"): score = (float)(-(int32_t)penalty), penalty = the exact optimum over global alignments of 0 per equal
 * byte pair, mismatch per unequal pair, gap_opening + L * gap_extension per gap of L bytes (match = 0).  No heuristic.
 *
 * Input: two exg_string_t[n_rows] columns as the scans leave them, each with its own payload; a NULL row (16 zero bytes) is
 * an empty string.  n_rows < 2^32 - 1.  1 <= mismatch <= 1023, 0 <= gap_opening <= 1023, 1 <= gap_extension <= 1023,
 * max_pair_bytes <= 2^21: anything else is EXG_E_INVALID_ARG.
 * A row with |text| + |pattern| > max_pair_bytes is an error (EXG_PE_ALIGN_TOO_LONG): the lowest such row wins, the result
 * block is exact and the outputs are unspecified.  A row whose optimum exceeds a non-zero max_penalty gets -INFINITY, its
 * bit is cleared in d_out_valid (when given; the op clears bits only — the column's validity, the AND of the inputs', is
 * the caller's to put there) and it is counted in n_capped: the safety valve for dissimilar long pairs.
 * Deterministic; no host round trip between the passes; n_rows = 0 is valid. */
typedef struct exg_align_score_result { /* 64 bytes, written by the device */
    uint64_t n_capped;      /* rows whose optimum exceeds max_penalty */
    uint64_t error_row;     /* lowest row that is too long */
    uint64_t error_length;  /* its |text| + |pattern| */
    uint64_t error_limit;   /* max_pair_bytes of the call */
    uint64_t n_global;      /* rows whose wavefronts did not fit LDS and ran out of the workspace */
    uint32_t error_code;    /* 0 or EXG_PE_ALIGN_TOO_LONG */
    uint32_t flags;         /* 0 (bit 0: a score loop ran into its hard bound — a defect, never expected) */
    uint8_t pad[16];
} exg_align_score_result;
typedef struct exg_align_score_args {
    const exg_string_t *d_text;    /* device, 16-byte aligned, n_rows entries */
    const void *d_text_payload;    /* device bytes the non-inlined texts point into */
    uint64_t text_payload_base;    /* string_t.ptr - text_payload_base = byte offset in d_text_payload */
    const exg_string_t *d_pattern; /* likewise */
    const void *d_pattern_payload;
    uint64_t pattern_payload_base;
    uint64_t n_rows;
    uint32_t mismatch, gap_opening, gap_extension;
    uint32_t max_penalty;          /* 0 = none */
    uint64_t max_pair_bytes;       /* the longest |text| + |pattern| the workspace is sized for */
    float *d_out_float;            /* out: device, n_rows entries */
    uint64_t *d_out_valid;         /* optional: device validity words, bit (row & 63) of word row >> 6; may be NULL */
    void *d_workspace;             /* device, 16-byte aligned, exg_align_workspace_bytes(...) */
    uint64_t workspace_bytes;
    exg_align_score_result *d_result;    /* device, 64 bytes, 8-byte aligned */
    void *stream;
    uint32_t lanes;                /* lanes of a wave a pair gets while its wavefronts fit LDS: 0 = default, 16, 32 or 64 */
    uint32_t reserved;             /* 0 */
} exg_align_score_args;
uint64_t exg_align_workspace_bytes(uint64_t n_rows, uint64_t max_pair_bytes, uint32_t mismatch, uint32_t gap_opening,
                                   uint32_t gap_extension);
/* Enqueue on args->stream; asynchronous. */
int exg_align_score(const exg_align_score_args *args);
/* Synchronising copy of the 64-byte result to the host.  error_code != 0: EXG_E_PARSE, and the thread's last error message is
 * `Alignment pair too long: <n> bytes (at most <max_pair_bytes>) in row <r>`; *out is filled either way. */
int exg_align_result(const exg_align_score_result *d_result, void *stream, exg_align_score_result *out);

/* ---- gap-affine alignment CIGARs on device-resident columns ----------------------------------------------
 * alignment_string / alignment_string_wfa_gap_affine of exon/src/exon/alignment_functions/module.cpp:150-247 for two VARCHAR
 * columns that are still in HBM: the run-length CIGAR (M equal pair, X unequal pair, I consumes a text byte, D a pattern
 * byte) of ONE optimal global alignment.  Which optimum is the backtrace rule of exon_duckdb_amd/csrc/exg_alignfn.hpp
 * ("Alignment strings"); the result is a valid input of exg_cigar_op.  A match score below 0 is the caller's
 * to fold into the penalties (2x - 2a, 2o, 2e - a) as the host scalar does.
 *
 * The input side is exg_align_score's, with the same limits and the same too-long rule (EXG_PE_ALIGN_TOO_LONG, the lowest
 * row wins).  Output: d_out_strings[r] holds a CIGAR of up to 12 bytes inlined; a longer one has its 4-byte prefix and
 * ptr = out_payload_base + offset, where offset is the sum of the lengths of the longer-than-12 rows in front of it — the
 * layout is a function of the input alone, two launches are byte-identical in both arrays.  result.out_bytes is the payload
 * the call needs, exact even on overflow; out_bytes > out_capacity is an error (exg_align_string_result: EXG_E_CAPACITY),
 * nothing is written at or past d_out_payload + out_capacity and the strings are unspecified.  A run's text is at most twice
 * the bytes it covers, so out_capacity = 2 * sum(|text| + |pattern|) can never overflow.
 * A row whose optimum exceeds a non-zero max_penalty gets 16 zero bytes, its bit cleared in d_out_valid (when given),
 * -INFINITY in d_out_score (when given) and is counted in n_capped; a row at exactly the cap keeps its CIGAR.
 * d_out_score, optional: the float exg_align_score gives for the row.
 * The workspace keeps every wavefront of the pairs in flight (the reference's memory_high): it grows with the square of the
 * largest penalty a row may reach — max_penalty, or 2 * gap_opening + gap_extension * max_pair_bytes when that is 0 — so long
 * pairs want a max_penalty.  exg_align_string_workspace_bytes returns 0 for arguments exg_align_string refuses and for a
 * workspace above 2^48 bytes.  n_rows = 0 is valid. */
struct exg_align_string_result { /* 64 bytes, written by the device */
    uint64_t n_capped;      /* rows whose optimum exceeds max_penalty */
    uint64_t error_row;     /* lowest row that is too long */
    uint64_t error_length;  /* its |text| + |pattern| */
    uint64_t error_limit;   /* max_pair_bytes of the call */
    uint64_t n_global;      /* rows whose wavefront ring did not fit LDS */
    uint64_t out_bytes;     /* payload bytes the call needs: the lengths of the CIGARs longer than 12 bytes */
    uint32_t error_code;    /* 0 or EXG_PE_ALIGN_TOO_LONG */
    uint32_t flags;         /* 0 (bit 0: a score loop ran into its hard bound, bit 1: a history slot filled up, bit 2: a
                               backtrace met a contradiction — defects, never expected) */
    uint64_t out_capacity;  /* of the call: what exg_align_string_result compares out_bytes with */
};
typedef struct exg_align_string_args {
    const exg_string_t *d_text;    /* as in exg_align_score_args, up to max_pair_bytes */
    const void *d_text_payload;
    uint64_t text_payload_base;
    const exg_string_t *d_pattern;
    const void *d_pattern_payload;
    uint64_t pattern_payload_base;
    uint64_t n_rows;
    uint32_t mismatch, gap_opening, gap_extension;
    uint32_t max_penalty;          /* 0 = none */
    uint64_t max_pair_bytes;
    exg_string_t *d_out_strings;   /* out: device, 16-byte aligned, n_rows entries */
    uint8_t *d_out_payload;        /* out: device, out_capacity bytes; may be NULL when out_capacity is 0 */
    uint64_t out_capacity;
    uint64_t out_payload_base;     /* string_t.ptr of an out-of-line CIGAR = out_payload_base + its offset in d_out_payload */
    float *d_out_score;            /* optional: device, n_rows entries */
    uint64_t *d_out_valid;         /* optional: device validity words; bits are cleared only */
    void *d_workspace;             /* device, 16-byte aligned, exg_align_string_workspace_bytes(...) */
    uint64_t workspace_bytes;
    struct exg_align_string_result *d_result; /* device, 64 bytes, 8-byte aligned */
    void *stream;
    uint32_t lanes;                /* as in exg_align_score_args */
    uint32_t reserved;             /* 0 */
} exg_align_string_args;
uint64_t exg_align_string_workspace_bytes(uint64_t n_rows, uint64_t max_pair_bytes, uint32_t mismatch, uint32_t gap_opening,
                                          uint32_t gap_extension, uint32_t max_penalty, uint64_t out_capacity);
/* Enqueue on args->stream; asynchronous. */
int exg_align_string(const exg_align_string_args *args);
/* Synchronising copy of the 64-byte result to the host; *out is filled either way.  error_code != 0: EXG_E_PARSE with the text
 * of exg_align_result.  out_bytes > the call's out_capacity: EXG_E_CAPACITY, `exg_align_string: the CIGARs take <out_bytes>
 * payload bytes, out_capacity is <out_capacity>`. */
int exg_align_string_result(const struct exg_align_string_result *d_result, void *stream, struct exg_align_string_result *out);

/* ---- CIGAR scalars on device-resident columns -------------------------------------------------------------
 * parse_cigar(VARCHAR) -> LIST(STRUCT(op VARCHAR, len INTEGER)) and extract_from_cigar(VARCHAR, VARCHAR) ->
 * STRUCT(sequence_start INTEGER, sequence_end INTEGER, sequence VARCHAR) of exon/src/exon/sam_functions/module.cpp:32-131 for
 * the cigar (and sequence) column a BAM or SAM scan just wrote.  The rules are stated once, in
 * exon_duckdb_amd/csrc/exg_cigarfn.hpp ("CIGAR scalars"): a row is [digits, one of MIDNSHP=X]+ with every
 * length <= 2^28 - 1 in value; the empty string and `*` are the CIGAR without operations.
 *
 * Input: exg_string_t[n_rows] columns as the scans leave them (up to 12 bytes inlined, longer strings at payload_base + offset
 * in their payload at any alignment); a NULL row = 16 zero bytes = the empty string.  n_rows < 2^32 - 1.
 * PARSE: the two children hold the operations of all rows in row order without gaps: d_out_op[k] is an inlined string_t of
 * length 1 (the letter, eleven zero bytes behind it), d_out_len[k] the length; d_out_entries[r] = {operations in front of row
 * r, operations of row r}, also for a row without any.  total_ops > ops_capacity: EXG_RF_CAPACITY, neither child is touched,
 * total_ops is exact and the rows are validated all the same; ops_capacity = 0 with NULL children is the counting call of a
 * two-call protocol.  total_ops counts every operation letter, those of a failing row too.
 * EXTRACT: start = the first operation's length if it is I, else 0; end = |sequence| - the last operation's length if it is
 * I, else |sequence| ({0, |sequence|} for the CIGAR without operations); d_out_sequence[r] is the slice [start, end): up to
 * 12 bytes inlined and zero padded, a longer one {length, its first four bytes, the input's ptr + start} — a zero-copy slice
 * of the caller's sequence payload under the same sequence_payload_base.  No output payload.
 * Errors: the lowest failing row wins; in it the leftmost offset at which a left-to-right parser stops (a bad byte or an
 * operation letter without digits: its offset; digits up to the end of the row: the row's length; a length above the bound:
 * the digit at which the value first exceeds it), then — EXTRACT — the range error (start > end, or |sequence| > 2^31 - 1).
 * With an error the result block is exact and the outputs are unspecified.  Deterministic: byte-identical outputs for
 * identical inputs.  No host round trip between the passes; n_rows = 0 is valid.
 * (`exg_cigar_result` names the struct as a tag and the function: write `struct exg_cigar_result`.) */
#define EXG_CIGAR_PARSE 1
#define EXG_CIGAR_EXTRACT 2
struct exg_cigar_result { /* 64 bytes, written by the device */
    uint64_t total_ops;    /* PARSE: operations of all rows; 0 for EXTRACT */
    uint64_t error_row;    /* lowest failing row */
    uint64_t error_offset; /* EXG_PE_CIGAR_INVALID: the byte offset in that row's CIGAR (the row's length: digits up to its end) */
    uint64_t n_rows;
    uint32_t error_code;   /* 0, EXG_PE_CIGAR_INVALID or EXG_PE_CIGAR_RANGE */
    uint32_t flags;        /* EXG_RF_CAPACITY: total_ops > ops_capacity, no child was written; EXG_RF_INDEX_OVERFLOW: the rows
                            * longer than 12 bytes hold more bytes than the workspace was sized for — nothing was done */
    uint8_t error_byte;    /* the byte at error_offset (0 when that is the row's length) */
    uint8_t pad[23];
};
typedef struct exg_cigar_op_args {
    uint32_t op;                      /* EXG_CIGAR_* */
    const exg_string_t *d_cigar;      /* device, 16-byte aligned, n_rows entries */
    const void *d_cigar_payload;      /* device bytes the non-inlined CIGARs point into */
    uint64_t cigar_payload_base;      /* string_t.ptr - cigar_payload_base = byte offset in d_cigar_payload */
    const exg_string_t *d_sequence;   /* EXTRACT: device, 16-byte aligned, n_rows entries */
    const void *d_sequence_payload;   /* EXTRACT: device bytes the non-inlined sequences point into */
    uint64_t sequence_payload_base;
    uint64_t n_rows;
    exg_list_entry_t *d_out_entries;  /* PARSE, out: device, 8-byte aligned, n_rows entries (may be NULL in the counting call) */
    exg_string_t *d_out_op;           /* PARSE, out: device, 16-byte aligned, ops_capacity entries */
    int32_t *d_out_len;               /* PARSE, out: device, 4-byte aligned, ops_capacity entries */
    uint64_t ops_capacity;
    int32_t *d_out_start;             /* EXTRACT, out: device, n_rows entries */
    int32_t *d_out_end;               /* EXTRACT, out: device, n_rows entries */
    exg_string_t *d_out_sequence;     /* EXTRACT, out: device, 16-byte aligned, n_rows entries */
    void *d_workspace;                /* device, 8-byte aligned, exg_cigar_workspace_bytes(...) */
    uint64_t workspace_bytes;
    struct exg_cigar_result *d_result; /* device, 64 bytes, 8-byte aligned */
    void *stream;
} exg_cigar_op_args;
/* cigar_payload_bytes: an upper bound of the summed lengths of the rows longer than 12 bytes — the size of the buffer
 * d_cigar_payload points into, unless rows share bytes (PARSE keeps one counter per 4 KiB of them; EXTRACT ignores it). */
uint64_t exg_cigar_workspace_bytes(uint32_t op, uint64_t n_rows, uint64_t cigar_payload_bytes);
/* Enqueue on args->stream; asynchronous. */
int exg_cigar_op(const exg_cigar_op_args *args);
/* Synchronising copy of the 64-byte result to the host.  error_code != 0: EXG_E_PARSE, and the thread's last error message
 * is `Invalid CIGAR string in row <r> at byte <k>` or `CIGAR insertions exceed the sequence in row <r>`; *out is filled
 * either way. */
int exg_cigar_result(const struct exg_cigar_result *d_result, void *stream, struct exg_cigar_result *out);

/* ---- GTF attributes on a device-resident column -------------------------------------------------------------
 * The ninth field of GTF lines (column 8 of exg_gtf_scan, or any exg_string_t column) -> the children of a
 * MAP(VARCHAR, VARCHAR): for row j of the call (row d_row_map[j] of the column when a row map is given) the entries
 * `key value` of the field in file order, a repeated key being a second entry.  The grammar is INTEGRATION.md's (GTF):
 * entries are separated by `;` outside quotes, a value is `"..."` (quotes not part of it, `;` and spaces allowed inside) or a
 * run of bytes that are neither space, `;` nor `"`; blank segments are skipped.  Keys and values are zero-copy slices of the
 * input's bytes under the same payload_base (up to 12 bytes inlined): there is no output payload.
 * d_out_entries[j] = {entries in front of row j, entries of row j} — with chunk_rows != 0 the offset is relative to the
 * first entry of the row's chunk of chunk_rows rows and d_out_chunk_base[c] (ceil(n_rows / chunk_rows) + 1 words) is where
 * chunk c's entries begin in the children (the layout of exg_vector LIST children).  total_entries > entries_capacity:
 * EXG_RF_CAPACITY, neither child is touched, total_entries is exact (when no row fails) and the rows are validated all the same;
 * entries_capacity = 0 with NULL children is the counting call of a two-call protocol.
 * Errors: the lowest failing row wins, in it the leftmost offset at which a left-to-right parser stops (an unterminated
 * quote: the offset of the quote; an entry without a value at the end of the field: the field's length, byte 0).  With an
 * error the result block is exact and the outputs are unspecified.  A wavefront takes a row, 64 bytes a step.
 * Deterministic; no host round trip between the passes; n_rows = 0 is valid; n_rows < 2^32 - 1. */
struct exg_gtf_attributes_result { /* 64 bytes, written by the device */
    uint64_t total_entries; /* entries of all rows */
    uint64_t error_row;     /* lowest failing row (an index of the call's rows) */
    uint64_t error_offset;  /* byte offset in that row's field */
    uint64_t n_rows;
    uint32_t error_code;    /* 0 or EXG_PE_GTF_ATTRIBUTES */
    uint32_t flags;         /* EXG_RF_CAPACITY: total_entries > entries_capacity, no child was written */
    uint8_t error_byte;     /* the byte at error_offset (0 when that is the field's length) */
    uint8_t pad[23];
};
typedef struct exg_gtf_attributes_args {
    const exg_string_t *d_strings;   /* device, 16-byte aligned */
    const void *d_payload;           /* device bytes the non-inlined strings point into */
    uint64_t payload_base;           /* string_t.ptr - payload_base = byte offset in d_payload */
    const uint32_t *d_row_map;       /* optional: device, n_rows row numbers of d_strings (NULL: rows 0 .. n_rows - 1) */
    uint64_t n_rows;
    uint64_t chunk_rows;             /* 0, or rows per chunk (list offsets relative to the chunk's first entry) */
    exg_list_entry_t *d_out_entries; /* out: device, 8-byte aligned, n_rows entries (may be NULL in the counting call) */
    uint64_t *d_out_chunk_base;      /* out: device, ceil(n_rows / chunk_rows) + 1 words; NULL when chunk_rows is 0 */
    exg_string_t *d_out_keys;        /* out: device, 16-byte aligned, entries_capacity entries */
    exg_string_t *d_out_values;      /* out: device, 16-byte aligned, entries_capacity entries */
    uint64_t entries_capacity;
    void *d_workspace;               /* device, 8-byte aligned, exg_gtf_attributes_workspace_bytes(n_rows) */
    uint64_t workspace_bytes;
    struct exg_gtf_attributes_result *d_result; /* device, 64 bytes, 8-byte aligned */
    void *stream;
} exg_gtf_attributes_args;
uint64_t exg_gtf_attributes_workspace_bytes(uint64_t n_rows);
/* Enqueue on args->stream; asynchronous. */
int exg_gtf_attributes(const exg_gtf_attributes_args *args);
/* Synchronising copy of the 64-byte result to the host.  error_code != 0: EXG_E_PARSE, and the thread's last error message is
 * `Invalid GTF attributes in row <r> at byte <k>`; *out is filled either way. */
int exg_gtf_attributes_result(const struct exg_gtf_attributes_result *d_result, void *stream, struct exg_gtf_attributes_result *out);

/* ---- GFF attributes on a device-resident column -------------------------------------------------------------
 * gff_parse_attributes(VARCHAR) -> MAP(VARCHAR, VARCHAR) (reference exon/src/exon/gff_functions/module.cpp:29-84) on a column
 * of GFF3 ninth fields (column 8 of exg_gtf_scan over a GFF3 file — the eight leading columns are the same —, or any
 * exg_string_t column): for row j of the call (row d_row_map[j] of the column when a row map is given) the entries key=value of
 * the field in field order, a repeated key being a second entry.  The grammar is INTEGRATION.md's (GFF attributes): the field is
 * cut at every `;` and segments of zero bytes are dropped; a segment loses its leading and trailing ' ' \t \n \v \f \r, is cut
 * at every `=`, pieces of zero bytes are dropped, and exactly two pieces must remain — neither trimmed on its own, nothing
 * percent-decoded.  Keys and values are zero-copy slices of the input's bytes under the same payload_base (up to 12 bytes
 * inlined; a token of an inlined row is inlined): there is no output payload.
 * The arguments are exg_gtf_attributes_args' field for field — d_out_entries, chunk_rows / d_out_chunk_base, the capacity
 * protocol (total_entries > entries_capacity: EXG_RF_CAPACITY, neither child is touched, total_entries is exact when no row
 * fails and the rows are validated all the same; entries_capacity = 0 with NULL children is the counting call) — so a reader
 * can feed either op.
 * Errors: the lowest failing row wins, in it the leftmost failing segment: error_offset = the offset in the field of the
 * segment's first byte behind the trim (of the segment's first byte when the trim leaves nothing), error_length = its length
 * behind the trim; a field without any segment (empty, or `;` only) fails as a whole: offset 0, its length.  With an error the
 * result block is exact and the outputs are unspecified.  A wavefront takes a row, 64 bytes a step.
 * Deterministic; no host round trip between the passes; n_rows = 0 is valid; n_rows < 2^32 - 1. */
struct exg_gff_attributes_result { /* 64 bytes, written by the device */
    uint64_t total_entries; /* entries of all rows */
    uint64_t error_row;     /* lowest failing row (an index of the call's rows) */
    uint64_t error_offset;  /* byte offset in that row's field */
    uint64_t n_rows;
    uint32_t error_code;    /* 0 or EXG_PE_GFF_ATTRIBUTES */
    uint32_t flags;         /* EXG_RF_CAPACITY: total_entries > entries_capacity, no child was written */
    uint32_t error_length;  /* bytes of the failing segment behind its trim */
    uint8_t pad[20];
};
typedef struct exg_gff_attributes_args {
    const exg_string_t *d_strings;   /* device, 16-byte aligned */
    const void *d_payload;           /* device bytes the non-inlined strings point into */
    uint64_t payload_base;           /* string_t.ptr - payload_base = byte offset in d_payload */
    const uint32_t *d_row_map;       /* optional: device, n_rows row numbers of d_strings (NULL: rows 0 .. n_rows - 1) */
    uint64_t n_rows;
    uint64_t chunk_rows;             /* 0, or rows per chunk (list offsets relative to the chunk's first entry) */
    exg_list_entry_t *d_out_entries; /* out: device, 8-byte aligned, n_rows entries (may be NULL in the counting call) */
    uint64_t *d_out_chunk_base;      /* out: device, ceil(n_rows / chunk_rows) + 1 words; NULL when chunk_rows is 0 */
    exg_string_t *d_out_keys;        /* out: device, 16-byte aligned, entries_capacity entries */
    exg_string_t *d_out_values;      /* out: device, 16-byte aligned, entries_capacity entries */
    uint64_t entries_capacity;
    void *d_workspace;               /* device, 8-byte aligned, exg_gff_attributes_workspace_bytes(n_rows) */
    uint64_t workspace_bytes;
    struct exg_gff_attributes_result *d_result; /* device, 64 bytes, 8-byte aligned */
    void *stream;
} exg_gff_attributes_args;
uint64_t exg_gff_attributes_workspace_bytes(uint64_t n_rows);
/* Enqueue on args->stream; asynchronous. */
int exg_gff_attributes(const exg_gff_attributes_args *args);
/* Synchronising copy of the 64-byte result to the host.  error_code != 0: EXG_E_PARSE, and the thread's last error message is
 * `Invalid GFF attribute in row <r> at byte <k>`; *out is filled either way. */
int exg_gff_attributes_result(const struct exg_gff_attributes_result *d_result, void *stream, struct exg_gff_attributes_result *out);

/* ---- region predicate on device-resident VCF columns --------------------------------------------------------
 * Which rows of a scanned VCF batch overlap a region (the row rule of vcf_query; the rules live once in csrc/exg_vcf_region.hpp):
 * row r is kept when its chrom equals the name byte for byte (the lengths are equal too: `1` is not `10`), pos <= end and
 * row_end >= start, where row_end is the integer of the INFO key `END=` — at the start of INFO or right behind a `;`, digits up
 * to the next `;` or the field's end (at most 18); `SVEND=` is not it; `END` without a value, `END=.`, anything that is not such
 * an integer, or no END key at all: pos + len(ref) - 1.  A row whose pos lies in [start, end] is kept without a look at INFO.
 * Coordinates are 1-based and closed; end = INT64_MAX is unbounded.
 * d_chrom, d_ref, d_info: the columns 0, 3 and 7 exg_vcf_scan writes (d_info: the raw INFO text); d_pos: its parsed POS.
 * d_keep: (n_rows + 63) / 64 whole words, bit r % 64 of word r / 64 = row r is kept, the tail bits of the last word zero — what
 * the reader's row selection takes beside a `filters` predicate.  A lane takes a row; no workspace, no result block.
 * Asynchronous on args->stream; n_rows = 0 is valid (nothing is written). */
typedef struct exg_vcf_region_args {
    const exg_string_t *d_chrom; /* device, 16-byte aligned */
    const exg_string_t *d_ref;   /* device, 16-byte aligned */
    const int64_t *d_pos;        /* device, 8-byte aligned */
    const exg_string_t *d_info;  /* device, 16-byte aligned */
    const void *d_payload;       /* device bytes the non-inlined strings point into */
    uint64_t payload_base;       /* string_t.ptr - payload_base = byte offset in d_payload */
    uint64_t n_rows;
    const uint8_t *d_name;       /* device: the region's reference name, name_len bytes */
    uint32_t name_len;
    uint32_t reserved;           /* 0 */
    int64_t start, end;          /* 1-based, closed; 1 <= start <= end */
    uint64_t *d_keep;            /* out: device, 8-byte aligned, (n_rows + 63) / 64 words */
    void *stream;
} exg_vcf_region_args;
int exg_vcf_region_keep(const exg_vcf_region_args *args);

/* ---- device inflate (gzip / BGZF members; replaces flate2 behind rust/src/arrow_reader.rs:60-91) ---- */
typedef struct exg_inflate_member {
    uint64_t comp_off;  /* offset of the member's DEFLATE stream (after the gzip header) in d_comp */
    uint64_t comp_size; /* bytes available from comp_off */
    uint64_t out_off;   /* where its output starts in d_out */
    uint64_t out_cap;   /* bytes it may produce (ISIZE when known) */
} exg_inflate_member;
typedef struct exg_inflate_status {
    uint32_t code; /* 0 ok, 1 bad block, 2 bad code lengths, 3 bad symbol/distance, 4 output overflow */
    uint32_t pad;
    uint64_t produced; /* bytes written at out_off */
    uint64_t consumed; /* compressed bytes consumed from comp_off (byte aligned after the final block) */
} exg_inflate_status;
/* Host: index the gzip members of data[start, n) (RFC 1952 framing).  Members that carry their size (BGZF 'BC'
 * subfield) are all returned; a member of unknown size is returned last with *open_ended = 1 (inflate it, then
 * index again from comp_off + consumed + 8).  *total_out is in/out: running sum of the output offsets.
 * A header zlib refuses is refused (EXG_E_PARSE): wrong magic, CM != 8, a reserved FLG bit, an FHCRC that does not match. */
int exg_gzip_index(const uint8_t *data, uint64_t n, uint64_t start, exg_inflate_member *members, uint64_t cap,
                   uint64_t *n_members, uint64_t *total_out, int *open_ended);
/* One wavefront per member; d_members / d_status are device arrays; d_comp 16-byte aligned. Asynchronous. */
int exg_inflate_members(const void *d_comp, void *d_out, const exg_inflate_member *d_members,
                        exg_inflate_status *d_status, uint32_t n_members, void *stream);

/* CRC-32 (the gzip trailer's checksum) of inflated bytes in HBM — the reference's decoders verify it (flate2 GzDecoder /
 * noodles-bgzf: "corrupt gzip stream does not have a matching checksum"), and so does the reader for every member.
 * One wavefront per segment; exg_crc32_members takes the segments from an exg_inflate_members call (out_off, produced).
 * Longer outputs are cut into segments whose checksums the host combines (exg_crc32_combine = zlib's crc32_combine). */
typedef struct exg_crc_segment {
    uint64_t off; /* first byte in d_data */
    uint64_t len;
} exg_crc_segment;
int exg_crc32_segments(const void *d_data, const exg_crc_segment *d_segs, uint32_t n_segs, uint32_t *d_crc, void *stream);
int exg_crc32_members(const void *d_out, const exg_inflate_member *d_members, const exg_inflate_status *d_status, uint32_t n_members,
                      uint32_t *d_crc, void *stream);
uint32_t exg_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* ONE big DEFLATE stream (a single-member gzip file) decoded by many wavefronts: block starts are searched near
 * every chunk_bytes of compressed input, the chunks are decoded concurrently with an unknown window and stitched
 * (pugz / rapidgzip method).  d_comp: the compressed bytes on the device, 16-byte aligned; the stream starts at
 * comp_off, at most comp_size bytes are read.  On success *d_out is a block of the library's device pool (*produced bytes
 * + 64 zeroed) that the caller gives back with exg_free_device() — hipFree() works too: pool blocks are whole allocations —
 * and *consumed the compressed bytes used.  On an error nothing stays allocated.  Synchronises the stream. */
int exg_inflate_stream(const void *d_comp, uint64_t comp_off, uint64_t comp_size, uint64_t chunk_bytes, void **d_out,
                       uint64_t *produced, uint64_t *consumed, void *stream);
/* The same stream in ROUNDS, so that neither the compressed nor the inflated bytes of a big member have to be resident at
 * once (the reference streams any size through a BufReader: rust/src/arrow_reader.rs:116-153): a round decodes from
 * start_bit (a block boundary; 0 for the first round) to a block boundary near the end of the bytes that are there.
 * Bit positions are relative to comp_off.  partial != 0: more compressed bytes follow behind comp_size — the round ends at
 * (or just behind) the last block start found and does not look at the stream's end; need_more != 0 on return means no
 * block start was found in the window (call again with more bytes; nothing was produced).  d_window: 32768 bytes of device
 * memory that carry the LZ77 window from round to round (have_window = 0 for a member's first round; updated in place).
 * front_reserve bytes stay free in front of the output: d_out + front_reserve is its first byte (any value; a caller that
 * wants an address congruent to the stream offset mod 16 — the decoded segments of the reader — passes reserve + (offset & 15)
 * with a 16-byte aligned reserve). */
typedef struct exg_inflate_round_args {
    const void *d_comp;
    uint64_t comp_off, comp_size;
    uint64_t start_bit;
    uint64_t chunk_bytes;
    int partial;
    int have_window;
    void *d_window;
    uint64_t front_reserve;
    double ratio_hint; /* inflated / compressed bytes seen so far; 0 = unknown */
    void *stream;
    /* results */
    void *d_out;        /* pool block of out_alloc bytes: exg_free_device_sized(d_out, out_alloc) */
    uint64_t out_alloc;
    uint64_t produced;
    uint64_t end_bit;   /* where the next round starts */
    int final_block;    /* the member's final block was decoded: end_bit (rounded up to a byte) is followed by the trailer */
    int need_more;
} exg_inflate_round_args;
int exg_inflate_round(exg_inflate_round_args *args);
/* Give a device block the library handed out (exg_inflate_stream, exg_inflate_round, exg_zstd_decode, exg_bzip2_decode) back to its pool. */
void exg_free_device(void *d_ptr, uint64_t bytes);

/* ---- device zstd (RFC 8878 frames; replaces zstd 0.12.3 / libzstd 1.5.2 behind rust/src/arrow_reader.rs:73, :87-88;
 * pinned by test_fastq_scan.test:22-32, 55-59 and test_fasta_scan.test:22-26, 45-49) --------------------------------
 * All frames of the stream data[0, n) — concatenated frames and skippable frames included, as ZSTD_decompressStream
 * reads them.  h_comp: the compressed bytes on the host (only frame / block headers are read there: a zstd stream states
 * the size of every block, so the host finds all blocks by a pointer chase and the device entropy-decodes them all at
 * once); d_comp: the same bytes on the device, readable to n + 16.  On success *d_out is a block of the library's device
 * pool (*produced bytes + 64 zeroed): exg_free_device(*d_out, *produced + 64) — hipFree works too.  Every frame with a Content_Checksum is verified: XXH64 on the device up to
 * EXG_ZSTD_VERIFY_MAX bytes of content per frame (default 64 MiB: the hash is a serial recurrence, ~0.55 GB/s per frame on a
 * GPU), larger frames on the host from a copy that comes back in 32 MiB pieces (~20 GB/s; a reader does this on a thread
 * of its own while it scans, and reports a mismatch when the file's last batch is out).  Windows above
 * 128 MiB and dictionaries are refused like libzstd's defaults do.  Synchronises the stream.
 * Errors: EXG_E_PARSE, libzstd's wording in exg_last_error_message(). */
int exg_zstd_decode(const uint8_t *h_comp, const void *d_comp, uint64_t n, void **d_out, uint64_t *produced, void *stream);

/* ---- device bzip2 (replaces libbz2 behind compression='bzip2', rust/src/arrow_reader.rs:87-88) ----------------------
 * Every concatenated stream of d_comp[0, n) (device memory), as bz2.decompress reads them: blocks are found on the device
 * by their 48-bit magic and chained (a block counts only where the one in front ends), decoded one wavefront each, and
 * every block CRC and stream CRC is verified.  On success *d_out is a block of the library's device pool (*produced
 * bytes + 64 zeroed): exg_free_device(*d_out, *produced + 64).  Synchronises the stream; on an error nothing stays
 * allocated.  Errors: EXG_E_PARSE with libbz2's categories in exg_last_error_message() — "not a bzip2 stream",
 * "data error in block N: <reason>" (a CRC mismatch included), "unexpected end of stream".  Randomised blocks
 * (bzip2 < 0.9.5) are refused as a data error. */
int exg_bzip2_decode(const void *d_comp, uint64_t n, void **d_out, uint64_t *produced, void *stream);

/* ---- (2) reader level ----------------------------------------------------------- */
typedef struct exg_reader exg_reader;

typedef struct exg_open_args {
    const char *path;        /* local file or directory (the reference lists directories: test_fasta_scan.test:55-59) */
    const char *file_format; /* "fasta" | "fastq" | "vcf" | "bam" | "bed" | "sam" | "bcf" | "gtf" (the reference's file_type strings,
                              * exon_extension.cpp:47-58; any case).  A BAM file is always read as gzip members (BGZF), whatever
                              * `compression` says, and as ONE shard (shard_count > 1: EXG_E_UNSUPPORTED).  "bed": text without a
                              * header, every line a record; "sam": the leading '@' lines are skipped at open, every line behind
                              * them is a record; both: batches, decoders, shards and fan-out as for VCF */
    const char *compression; /* NULL = infer from extension like arrow_reader.rs:60-75; "gzip","zstd","uncompressed",... */
    uint64_t batch_rows;     /* rows per chunk; 0 => EXG_VECTOR_SIZE */
    int device;              /* HIP device ordinal */
    uint64_t device_batch_bytes; /* bytes shipped to HBM per launch; 0 => default */
    const char *filters;     /* NULL / "" or the predicate FilterToString renders (module.cpp:158-214), same grammar as
                              * new_reader's: evaluated on the device, only the rows where it is TRUE are copied back.
                              * Nested columns (VCF id / alt / filter / info / formats) are refused, like in new_reader. */
    uint32_t shard_index;    /* byte-range shards of every file: this reader yields the records / lines that */
    uint32_t shard_count;    /* END in its 1/shard_count of the bytes behind the header.  One process per GPU opens the same
                              * path with its rank: the shards partition the rows, in file order, with no exchange (the FASTQ
                              * 4-line phase at a cut is found from the bytes around it).  The first batch of a shard carries
                              * 1 MiB (EXG_SHARD_HALO) of the bytes in front of its cut; when the record that ends behind the
                              * cut begins further back, the halo grows until it holds it: a record of any length across a
                              * cut is found, like the unsharded scan finds it.  BGZF inputs are sharded by members (a member
                              * belongs to the shard in whose bytes its header begins; each rank uploads and inflates only its
                              * own members + a halo of members in front, a VCF also the leading members that hold the
                              * header), multi-frame zstd inputs by frames.  FASTA: a record belongs to the shard in whose
                              * bytes (bgzip: members' bytes, zstd: frames' bytes) its '>' line begins; a shard is that run of
                              * whole records.  Not sharded (EXG_E_UNSUPPORTED): gzip without member sizes.
                              * shard_count = 1: the whole input through this one reader and its device.
                              * shard_count = 0: the whole input, and the reader may FAN OUT by itself: on a box with several
                              * devices (and an input that can be sharded) it cuts the input into stripes of ~1 GiB, reads
                              * them with worker threads on all devices and hands their batches out here in file order
                              * (exg_count_only sums them) — one consumer-facing stream, N GPUs. */
    uint64_t columns;        /* projection (DuckDB's projection_pushdown: module.cpp:310, input.column_ids): bit c = column c of
                              * exg_schema_of is wanted; 0 = all.  Every column is still tokenised, typed and validated on
                              * the device — a malformed INFO value is an error whether the column is selected or not, like in
                              * the reference, which parses everything and projects afterwards — but only the wanted ones are
                              * copied back: exg_chunk.vectors[c] of the others is NULL.  read_vcf's nested columns are
                              * two thirds of its bytes over PCIe.  Every bit is a column: ~0 = all, like 0. */
    uint64_t flags;          /* ABI 9 (a word of its own: ABI 8 kept this hint in bit 63 of `columns`, where columns = ~0 for "all"
                              * set it by accident).  EXG_OPEN_CHUNKS: the caller is going to pull chunks (exg_next_chunk), not
                              * exg_count_only — what a table function knows at init_global (column_ids != {ROW_ID}).  A compressed
                              * input's decoded segments then travel to the host from the FIRST one on, beside the decoder; without
                              * the hint that begins with the first exg_next_chunk call, and the segments decoded before it (one or
                              * two, up to 1 GiB each for zstd) are copied behind their scan. */
} exg_open_args;
#define EXG_OPEN_CHUNKS 1ull

#define EXG_TYPE_VARCHAR 1
#define EXG_TYPE_BIGINT 2
#define EXG_TYPE_FLOAT 3
#define EXG_TYPE_INTEGER 4 /* int32_t */
#define EXG_TYPE_BOOLEAN 5 /* one byte per value (DuckDB BOOLEAN) */
#define EXG_TYPE_LIST 6    /* data = exg_list_entry_t[] (DuckDB list_entry_t), children[0] = the elements */
#define EXG_TYPE_STRUCT 7  /* no data of its own; children = the fields, each as long as the parent */
#define EXG_TYPE_MAP 8     /* DuckDB MAP: LIST's layout — data = exg_list_entry_t[], children[0] = a STRUCT of `key` and `value` */

/* The full type of a column.  The VCF columns carry the reference's schema (what DuckDB's Arrow conversion makes of
 * exon's Arrow schema, exon/src/exon/arrow_table_function/module.cpp:126-147; pinned by test_vcf_record_scan.test:10-19):
 * id / alt / filter LIST(VARCHAR), info STRUCT(<##INFO keys>), formats LIST(STRUCT(<##FORMAT keys>)), a key with
 * Number != 1 being a LIST of its type. */
typedef struct exg_type {
    int type; /* EXG_TYPE_* */
    int nullable;
    const char *name; /* column / field name; "item" for list elements */
    int n_children;
    const struct exg_type *children;
} exg_type;

/* One DuckDB vector of a chunk, same shape as its exg_type: flat data + validity (bit i = element i valid; NULL = all
 * valid) + children.  LIST: data = exg_list_entry_t[length] whose offsets are relative to children[0] as handed out
 * here (the child vector of THIS chunk).  STRUCT: data = NULL.  All memory is owned by the chunk's keepalive. */
typedef struct exg_vector {
    void *data;
    uint64_t *validity;
    uint64_t length;
    int n_children;
    const struct exg_vector *children;
} exg_vector;

typedef struct exg_schema {
    int n_columns;
    const char *names[16]; /* owned by the reader */
    int types[16];         /* EXG_TYPE_* of the column itself */
    int nullable[16];
    const exg_type *tree[16]; /* the column's full type (owned by the reader) */
} exg_schema;

typedef struct exg_chunk {
    uint64_t n_rows;           /* 0 => end of stream */
    int n_columns;
    void *data[16];            /* host pointers: exg_string_t[n_rows] / int64_t[] / float[] / exg_list_entry_t[] (STRUCT: NULL) */
    uint64_t *validity[16];    /* NULL => all valid; else ceil(n_rows/64) words */
    void *keepalive;           /* opaque; payload + vectors stay valid until exg_release_chunk */
    const exg_vector *vectors[16]; /* every column as a vector tree (data / validity above are vectors[c]'s own); NULL (and
                                * data[c] NULL) for a column outside exg_open_args.columns */
    uint64_t batch_no;         /* which device batch of this reader the rows come from (0, 1, ...: non-decreasing; what the
                                * table function reports as DuckDB's batch index, module.cpp has none: MaxThreads() == 1) */
} exg_chunk;

int exg_open(const exg_open_args *args, exg_reader **out);
/* How many byte-range shards a scan of this input is worth, and on which device each runs: what the table function's
 * init_global asks (MaxThreads() = *n_shards; init_local i opens shard i with device = devices[i]) — the in-process form
 * of SURVEY §8 E1: one host thread and one GPU per shard, nothing exchanged.  One shard per visible device when the input
 * can be sharded (text FASTQ / VCF / FASTA; BGZF FASTQ / VCF / FASTA, by members; multi-frame zstd, by frames) and holds
 * >= 256 MiB per shard, else 1 (single-member gzip, a single zstd frame).
 * EXON_GPU_SHARDS=n forces n (several shards on one device: how the tests exercise it on a 1-GPU box). */
int exg_plan_shards(const exg_open_args *args, uint32_t *n_shards, int *devices, uint32_t devices_cap);
/* VCF: opens the first file (the INFO / FORMAT keys of its header are the schema), so it can fail like a scan can. */
int exg_schema_of(exg_reader *r, exg_schema *out);
int exg_next_chunk(exg_reader *r, exg_chunk *out);
void exg_release_chunk(exg_reader *r, exg_chunk *chunk);
/* COUNT(*) fast path: no column is materialised. */
int exg_count_only(exg_reader *r, uint64_t *n_rows);
const char *exg_reader_error(exg_reader *r);
/* What a reader holds and has done so far.  Memory does not grow with the input: plain files travel in device batches,
 * compressed ones are decoded into a bounded stream of segments (like the reference's BufReader + convert_stream,
 * rust/src/arrow_reader.rs:60-91, 116-153).  EXG_DEVICE_MEM_CAP_MB=<MiB> (read at exg_open) sizes both from a budget. */
typedef struct exg_reader_stats {
    uint64_t device_bytes_now;   /* device memory held on behalf of this reader (pool size classes) */
    uint64_t device_bytes_peak;  /* ... its high-water mark */
    uint64_t device_mem_cap;     /* EXG_DEVICE_MEM_CAP_MB in bytes, 0 = not set */
    uint64_t device_batch_bytes; /* bytes per device batch / decoded segment */
    uint64_t device_batches;     /* scans launched */
    uint64_t decoded_segments;   /* segments of a compressed input consumed */
    uint64_t scan_algo;          /* EXG_ALGO_* the next device batch starts with: EXG_ALGO_FUSED until a batch came back with
                                  * EXG_RF_REDO (long reads, reads below ~45 bp, multi-sample VCF lines, bytes >= 0x80), then
                                  * EXG_ALGO_FUSED_FULL for the rest of the input (a fan-out reader: 0) */
    uint64_t input_bytes;        /* ABI 8: size of the reader's input files on disk (all files of a directory; a shard: the whole
                                  * files), what TableFunction::cardinality estimates rows from (module.cpp:307) */
    uint64_t input_compression;  /* ABI 8: 0 plain text, 1 gzip / BGZF, 2 zstd, 3 bzip2 (input_bytes are compressed bytes then) */
    uint64_t nested_ns;          /* ABI 9: read_vcf — wall time the reader's thread spent making the nested columns (id / alt / filter /
                                  * info / formats) of its batches on the device, counting passes, prefix sums and children, up to the
                                  * point where their vectors start for the host (exg_vcf_nested.hpp) */
    uint64_t host_vector_bytes;  /* ABI 9: bytes of column vectors (flat and nested, validity included) sent to the host so far —
                                  * what a scan INTO DataChunks pays on the D2H link next to a decoded input's own bytes */
    uint64_t bam_tiles;          /* read_bam_file_records: tiles of all device batches so far (exg_bam_scan_result.tiles) ... */
    uint64_t bam_tiles_rewalked; /* ... and those that were walked a second time (words that were reserved: the layout is ABI 9's) */
    uint64_t reserved[1];        /* [0]: region_members — a region reader (exg_open_region): the BGZF members its plan had inflated so
                                  * far, the leading members that hold the header and the members of its ranges both counted (a
                                  * member in both counts twice: it is inflated twice); a member read behind a range only to
                                  * complete that range's last line is not part of the plan and is not counted.  Else 0 */
} exg_reader_stats;
int exg_reader_stats_of(exg_reader *r, exg_reader_stats *out);

/* ---- region queries: a tabix index, its planner, and a reader over the members it selects ------------------ */
typedef struct exg_virtual_chunk {
    uint64_t begin, end; /* BGZF virtual offsets: (offset of a member in the file << 16) | offset in its inflated bytes */
} exg_virtual_chunk;
typedef struct exg_region {
    int64_t start, end; /* 1-based, closed; end = INT64_MAX: to the end of the sequence */
    uint32_t ref_id;    /* the reference's number in the index */
    uint32_t name_len;
    char name[256];     /* the reference's name, NUL-terminated */
} exg_region;
/* Host only.  index_bytes: the INFLATED bytes of a .tbi (format 2, VCF; anything truncated or whose counts the bytes do not hold:
 * EXG_E_PARSE, never a read outside [index_bytes, index_bytes + n)).  region: `name`, `name:start` or `name:start-end`, split at
 * the LAST colon, the whole string first tried as a name (csrc/exg_tabix.hpp: G1 .. G5); empty, or a name the index does not
 * hold: EXG_E_INVALID_ARG with a message that names it.  The chunks to read, sorted and merged (P1 .. P6), go to out[0 .. cap):
 * *n_chunks is always their number; they are written only when all of them fit, else EXG_E_CAPACITY — except in the counting
 * call (out = NULL, cap = 0), which returns EXG_OK.  resolved (optional): what the region came to. */
int exg_tabix_query(const uint8_t *index_bytes, uint64_t n, const char *region, exg_virtual_chunk *out, uint64_t cap, uint64_t *n_chunks,
                    exg_region *resolved);
/* vcf_query(path, region): exg_open for a BGZF-compressed VCF with a tabix index beside it (<path>.tbi), reading only the members
 * the index selects for `region`.  file_format must be "vcf", the path one BGZF file, shard_count 1 (0 or more: EXG_E_UNSUPPORTED);
 * the index is inflated by the device inflater (no zlib), planned by exg_tabix_query's planner, and every chunk is checked against
 * the file — a virtual offset outside it or not on a member header is a stale or foreign index: EXG_E_IO.  The rows that leave are
 * those exg_vcf_region_keep keeps, ANDed with args->filters when there are any; projection, nested columns, the memory cap and
 * exg_count_only are read_vcf's.  exg_reader_stats.reserved[0] counts the members inflated. */
int exg_open_region(const exg_open_args *args, const char *region, exg_reader **out);
/* Device buffers, pinned host blocks and HIP streams of closed readers are recycled process-wide (size classes, at most
 * EXG_POOL_MAX_GB = 64 GB of HBM): this gives them back (the extension's unload / idle path). */
void exg_trim_pools(void);
void exg_close(exg_reader *r);

/* ---- (3) reference-FFI compatible ------------------------------------------------------ */
/* exon/include/rust.hpp:11-13 */
typedef struct ReplacementScanResult {
    const char *file_type; /* "FASTA" | "FASTQ" | "VCF" | "BAM" | "BED" (static storage) or NULL */
} ReplacementScanResult;
/* exon/include/rust.hpp:48, rust/src/arrow_reader.rs:173-197: last extension, skipping one
 * compression extension (gz, gzip, zst, zstd, bz2, bzip2, xz). */
ReplacementScanResult replacement_scan(const char *uri);

/* The Arrow C data / stream interface (the published ABI the reference exchanges batches through:
 * `struct ArrowArrayStream stream;` at exon/src/exon/arrow_table_function/module.cpp:82, 228). */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
#define ARROW_FLAG_DICTIONARY_ORDERED 1
#define ARROW_FLAG_NULLABLE 2
#define ARROW_FLAG_MAP_KEYS_SORTED 4
struct ArrowSchema {
    const char *format;
    const char *name;
    const char *metadata;
    int64_t flags;
    int64_t n_children;
    struct ArrowSchema **children;
    struct ArrowSchema *dictionary;
    void (*release)(struct ArrowSchema *);
    void *private_data;
};
struct ArrowArray {
    int64_t length;
    int64_t null_count;
    int64_t offset;
    int64_t n_buffers;
    int64_t n_children;
    const void **buffers;
    struct ArrowArray **children;
    struct ArrowArray *dictionary;
    void (*release)(struct ArrowArray *);
    void *private_data;
};
#endif
#ifndef ARROW_C_STREAM_INTERFACE
#define ARROW_C_STREAM_INTERFACE
struct ArrowArrayStream {
    int (*get_schema)(struct ArrowArrayStream *, struct ArrowSchema *out);
    int (*get_next)(struct ArrowArrayStream *, struct ArrowArray *out);
    const char *(*get_last_error)(struct ArrowArrayStream *);
    void (*release)(struct ArrowArrayStream *);
    void *private_data;
};
#endif

/* exon/include/rust.hpp:7-9 */
typedef struct ReaderResult {
    const char *error; /* NULL on success; else a heap C string the caller may free() (the reference leaks it) */
} ReaderResult;

/* exon/include/rust.hpp:41-46, rust/src/arrow_reader.rs:38-166 — the reference's own entry point,
 * same name, same arguments, same results: fills *stream_ptr with a stream of record batches of at
 * most batch_size rows (a multiple of 64).  The tokenising, the typed VCF columns (LIST / STRUCT),
 * the `filters` predicate and the Arrow buffers themselves (offsets, values, validity) are produced
 * on the device; the host only copies them back and wires the ArrowArray structs.
 *   compression: NULL = by extension (:60-75), else DataFusion's FileCompressionType names (:77-91)
 *   file_format: "fasta" | "fastq" | "vcf" ("bam", "bed", "sam" and "gtf" are refused: they are served at the chunk boundary, exg_open, only)
 *   filters:     NULL / "" or the predicate text FilterToString renders (module.cpp:158-214):
 *                <column> (= | != | <> | < | <= | > | >=) <literal>, <column> IS [NOT] NULL, AND, OR
 *                with SQL precedence; it is applied as `SELECT * FROM exon_table WHERE <filters>` (:125-141). */
ReaderResult new_reader(struct ArrowArrayStream *stream_ptr, const char *uri, uintptr_t batch_size,
                        const char *compression, const char *file_format, const char *filters);

/* exon/include/rust.hpp:23-25, 60-63, rust/src/vcf_query_reader.rs:31-36 — the reference's entry point behind vcf_query, same
 * name, same arguments: new_reader's VCF stream over a region reader (exg_open_region: uri is a BGZF VCF with <uri>.tbi beside
 * it, query a region). */
typedef struct VCFReaderResult {
    const char *error; /* NULL on success; else a heap C string the caller may free() */
} VCFReaderResult;
/* the library's entry: the error string, or NULL */
const char *exg_vcf_query_reader(struct ArrowArrayStream *stream_ptr, const char *uri, const char *query, uintptr_t batch_size);
/* the reference's name and signature over it, for the glue that calls it (the library itself exports exg_* names, replacement_scan
 * and new_reader only) */
static inline VCFReaderResult vcf_query_reader(struct ArrowArrayStream *stream_ptr, const char *uri, const char *query, uintptr_t batch_size) {
    VCFReaderResult res;
    res.error = exg_vcf_query_reader(stream_ptr, uri, query, batch_size);
    return res;
}

#ifdef __cplusplus
}
#endif
#endif /* EXON_GPU_H */
