"""ctypes mirror of include/exon_gpu.h (keep in sync with the header; tests check sizes)."""
import ctypes as C

EXG_ABI_VERSION = 9
EXG_TYPE_VARCHAR, EXG_TYPE_BIGINT, EXG_TYPE_FLOAT, EXG_TYPE_INTEGER, EXG_TYPE_BOOLEAN, EXG_TYPE_LIST, EXG_TYPE_STRUCT = 1, 2, 3, 4, 5, 6, 7
EXG_TYPE_MAP = 8   # LIST's layout over a STRUCT of key and value
EXG_VECTOR_SIZE = 2048
EXG_OPEN_CHUNKS = 1   # exg_open_args.flags

EXG_OK = 0
EXG_E_INVALID_ARG, EXG_E_NO_DEVICE, EXG_E_HIP, EXG_E_IO = -1, -2, -3, -4
EXG_E_UNSUPPORTED, EXG_E_PARSE, EXG_E_CAPACITY, EXG_E_NOMEM = -5, -6, -7, -8

EXG_PE_NONE = 0
EXG_PE_FASTQ_NAME_PREFIX = 1
EXG_PE_FASTQ_PLUS_PREFIX = 2
EXG_PE_UNEXPECTED_EOF = 3
EXG_PE_INVALID_UTF8 = 4
EXG_PE_FASTA_MISSING_PREFIX = 5
EXG_PE_FASTA_MISSING_NAME = 6
EXG_PE_FASTA_EMPTY_DEF = 7
EXG_PE_VCF_MISSING_FIELD = 8
EXG_PE_VCF_BAD_POS = 9
EXG_PE_VCF_BAD_QUAL = 10
EXG_PE_VCF_NO_HEADER = 11
EXG_PE_FIELD_TOO_LONG = 12
EXG_PE_VCF_INFO = 13
EXG_PE_VCF_FORMAT = 14
EXG_PE_BAM_BLOCK_SIZE = 15
EXG_PE_BAM_TRUNCATED = 16
EXG_PE_BAM_READ_NAME = 17
EXG_PE_BAM_REFERENCE_ID = 18
EXG_PE_BAM_FIELD_LENGTHS = 19
EXG_PE_BAM_CIGAR_OP = 20
EXG_PE_BAM_QUALITY = 21
EXG_PE_BED_FIELD_COUNT = 22
EXG_PE_BED_REFERENCE_NAME = 23
EXG_PE_BED_POSITION = 24
EXG_PE_BED_SCORE = 25
EXG_PE_BED_STRAND = 26
EXG_PE_BED_COLOR = 27
EXG_PE_BED_BLOCKS = 28
EXG_PE_SEQ_INVALID_CHARACTER = 30   # (29 is unassigned)
EXG_PE_SEQ_LENGTH = 31
EXG_PE_SEQ_CODON = 32
EXG_PE_ALIGN_TOO_LONG = 33
EXG_PE_SAM_FIELD_COUNT = 35   # (34 is unassigned)
EXG_PE_SAM_EMPTY_FIELD = 36
EXG_PE_SAM_HEADER_LINE = 37
EXG_PE_SAM_FLAG = 38
EXG_PE_SAM_POSITION = 39
EXG_PE_SAM_MAPQ = 40
EXG_PE_SAM_CIGAR = 41
EXG_PE_SAM_LENGTHS = 42
EXG_PE_CIGAR_INVALID = 44   # (43 is unassigned)
EXG_PE_CIGAR_RANGE = 45
EXG_PE_BCF_RECORD_LENGTH = 47   # (46 is unassigned)
EXG_PE_BCF_TRUNCATED = 48
EXG_PE_BCF_TYPE = 49
EXG_PE_BCF_RESERVED_VALUE = 50
EXG_PE_BCF_OVERRUN = 51
EXG_PE_BCF_CHROM = 52
EXG_PE_BCF_DICT_INDEX = 53
EXG_PE_BCF_NO_ALLELE = 54
EXG_PE_BCF_SAMPLE_COUNT = 55
EXG_PE_GTF_FIELD_COUNT = 57   # (56 is unassigned)
EXG_PE_GTF_EMPTY_FIELD = 58
EXG_PE_GTF_POSITION = 59
EXG_PE_GTF_SCORE = 60
EXG_PE_GTF_STRAND = 61
EXG_PE_GTF_FRAME = 62
EXG_PE_GTF_ATTRIBUTES = 63
EXG_PE_GFF_ATTRIBUTES = 65    # (64 stays unassigned)

EXG_FMT_FASTA, EXG_FMT_FASTQ, EXG_FMT_VCF, EXG_FMT_BAM, EXG_FMT_BED, EXG_FMT_SAM = 1, 2, 3, 4, 5, 6
EXG_FMT_BCF = 7
EXG_FMT_GTF = 8
EXG_GTF_COLUMNS = 9
EXG_BAM_COLUMNS = 10
EXG_BED_COLUMNS = 12
EXG_SAM_COLUMNS = 10
EXG_F_BOF, EXG_F_EOF, EXG_F_NO_STORE = 1, 2, 4
EXG_RF_NON_ASCII, EXG_RF_HEAD_UNRESOLVED, EXG_RF_FALLBACK, EXG_RF_CAPACITY, EXG_RF_INDEX_OVERFLOW = 1, 2, 4, 8, 16
EXG_RF_QUAL_RANGE = 32
EXG_RF_REDO = 64
EXG_RF_ROWS_SKIPPED = 128
EXG_ALGO_AUTO, EXG_ALGO_MULTIPASS, EXG_ALGO_FUSED, EXG_ALGO_FUSED_FULL, EXG_ALGO_FUSED_INDEX = 0, 1, 2, 3, 4

EXG_SEQ_COMPLEMENT, EXG_SEQ_REVERSE_COMPLEMENT, EXG_SEQ_TRANSCRIBE, EXG_SEQ_REVERSE_TRANSCRIBE = 1, 2, 3, 4
EXG_SEQ_TRANSLATE, EXG_SEQ_GC_CONTENT = 5, 6
EXG_CIGAR_PARSE, EXG_CIGAR_EXTRACT = 1, 2

EXG_SYNTH_FASTQ_SEED = 0xE0A5EED0001
EXG_SYNTH_VCF_SEED = 0xE0A5EED0002
EXG_SYNTH_FASTQ_RECORD_BYTES = 332


class ScanResult(C.Structure):
    _fields_ = [
        ("n_records", C.c_uint64),
        ("n_lines", C.c_uint64),
        ("consumed_bytes", C.c_uint64),
        ("error_offset", C.c_uint64),
        ("error_record", C.c_uint64),
        ("error_code", C.c_uint32),
        ("flags", C.c_uint32),
        ("payload_bytes", C.c_uint64),
        ("redo_tiles", C.c_uint64),
    ]


class FastqScanArgs(C.Structure):
    _fields_ = [
        ("d_input", C.c_void_p),
        ("n_bytes", C.c_uint64),
        ("lead", C.c_uint64),
        ("first_line_index", C.c_uint64),
        ("payload_base", C.c_uint64),
        ("flags", C.c_uint32),
        ("algo", C.c_uint32),
        ("d_name", C.c_void_p),
        ("d_description", C.c_void_p),
        ("d_sequence", C.c_void_p),
        ("d_quality", C.c_void_p),
        ("d_description_validity", C.c_void_p),
        ("capacity_records", C.c_uint64),
        ("d_workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
        ("d_result", C.c_void_p),
        ("stream", C.c_void_p),
    ]


class VcfScanArgs(C.Structure):
    _fields_ = [
        ("d_input", C.c_void_p),
        ("n_bytes", C.c_uint64),
        ("lead", C.c_uint64),
        ("payload_base", C.c_uint64),
        ("flags", C.c_uint32),
        ("algo", C.c_uint32),
        ("d_fields", C.c_void_p * 9),
        ("d_pos", C.c_void_p),
        ("d_qual", C.c_void_p),
        ("d_qual_validity", C.c_void_p),
        ("d_formats_validity", C.c_void_p),
        ("capacity_records", C.c_uint64),
        ("d_workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
        ("d_result", C.c_void_p),
        ("stream", C.c_void_p),
    ]


class FastaScanArgs(C.Structure):
    _fields_ = [
        ("d_input", C.c_void_p),
        ("n_bytes", C.c_uint64),
        ("lead", C.c_uint64),
        ("payload_base", C.c_uint64),
        ("seq_payload_base", C.c_uint64),
        ("flags", C.c_uint32),
        ("algo", C.c_uint32),
        ("d_id", C.c_void_p),
        ("d_description", C.c_void_p),
        ("d_sequence", C.c_void_p),
        ("d_description_validity", C.c_void_p),
        ("d_seq_payload", C.c_void_p),
        ("capacity_records", C.c_uint64),
        ("d_workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
        ("d_result", C.c_void_p),
        ("stream", C.c_void_p),
    ]


class BamScanResult(C.Structure):
    _fields_ = [
        ("n_records", C.c_uint64),
        ("consumed_bytes", C.c_uint64),
        ("side_bytes", C.c_uint64),
        ("error_record", C.c_uint64),
        ("error_offset", C.c_uint64),
        ("error_code", C.c_uint32),
        ("flags", C.c_uint32),
        ("tiles", C.c_uint64),
        ("tiles_rewalked", C.c_uint64),
    ]


class BamScanArgs(C.Structure):
    _fields_ = [
        ("d_input", C.c_void_p),
        ("n_bytes", C.c_uint64),
        ("flags", C.c_uint32),
        ("n_ref", C.c_int32),
        ("columns", C.c_uint64),
        ("d_ref_names", C.c_void_p),
        ("d_ref_offsets", C.c_void_p),
        ("ref_names_base", C.c_uint64),
        ("d_columns", C.c_void_p * 10),
        ("d_validity", C.c_void_p * 10),
        ("d_side", C.c_void_p),
        ("side_capacity", C.c_uint64),
        ("side_base", C.c_uint64),
        ("capacity_records", C.c_uint64),
        ("d_workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
        ("d_result", C.c_void_p),
        ("stream", C.c_void_p),
    ]


class BedScanArgs(C.Structure):
    _fields_ = [
        ("d_input", C.c_void_p),
        ("n_bytes", C.c_uint64),
        ("lead", C.c_uint64),
        ("payload_base", C.c_uint64),
        ("flags", C.c_uint32),
        ("algo", C.c_uint32),
        ("d_columns", C.c_void_p * 12),
        ("d_validity", C.c_void_p * 12),
        ("capacity_records", C.c_uint64),
        ("d_workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
        ("d_result", C.c_void_p),
        ("stream", C.c_void_p),
    ]


class SamScanArgs(C.Structure):
    _fields_ = [
        ("d_input", C.c_void_p),
        ("n_bytes", C.c_uint64),
        ("lead", C.c_uint64),
        ("payload_base", C.c_uint64),
        ("flags", C.c_uint32),
        ("algo", C.c_uint32),
        ("d_columns", C.c_void_p * 10),
        ("d_validity", C.c_void_p * 10),
        ("capacity_records", C.c_uint64),
        ("d_workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
        ("d_result", C.c_void_p),
        ("stream", C.c_void_p),
    ]


class QualityListArgs(C.Structure):
    _fields_ = [
        ("d_strings", C.c_void_p),
        ("n_rows", C.c_uint64),
        ("d_payload", C.c_void_p),
        ("payload_base", C.c_uint64),
        ("d_entries", C.c_void_p),
        ("d_values", C.c_void_p),
        ("values_capacity", C.c_uint64),
        ("d_total", C.c_void_p),
        ("d_workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
        ("stream", C.c_void_p),
    ]


class SeqResult(C.Structure):
    _fields_ = [
        ("total_bytes", C.c_uint64),
        ("error_row", C.c_uint64),
        ("error_offset", C.c_uint64),
        ("error_length", C.c_uint64),
        ("error_code", C.c_uint32),
        ("flags", C.c_uint32),
        ("error_bytes", C.c_uint8 * 4),
        ("pad", C.c_uint8 * 20),
    ]


class SequenceOpArgs(C.Structure):
    _fields_ = [
        ("op", C.c_uint32),
        ("d_strings", C.c_void_p),
        ("n_rows", C.c_uint64),
        ("d_payload", C.c_void_p),
        ("payload_base", C.c_uint64),
        ("d_out_strings", C.c_void_p),
        ("d_out_payload", C.c_void_p),
        ("out_capacity", C.c_uint64),
        ("out_base", C.c_uint64),
        ("d_out_float", C.c_void_p),
        ("d_workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
        ("d_result", C.c_void_p),
        ("stream", C.c_void_p),
    ]


class AlignScoreResult(C.Structure):
    _fields_ = [
        ("n_capped", C.c_uint64),
        ("error_row", C.c_uint64),
        ("error_length", C.c_uint64),
        ("error_limit", C.c_uint64),
        ("n_global", C.c_uint64),
        ("error_code", C.c_uint32),
        ("flags", C.c_uint32),
        ("pad", C.c_uint8 * 16),
    ]


class AlignScoreArgs(C.Structure):
    _fields_ = [
        ("d_text", C.c_void_p),
        ("d_text_payload", C.c_void_p),
        ("text_payload_base", C.c_uint64),
        ("d_pattern", C.c_void_p),
        ("d_pattern_payload", C.c_void_p),
        ("pattern_payload_base", C.c_uint64),
        ("n_rows", C.c_uint64),
        ("mismatch", C.c_uint32),
        ("gap_opening", C.c_uint32),
        ("gap_extension", C.c_uint32),
        ("max_penalty", C.c_uint32),
        ("max_pair_bytes", C.c_uint64),
        ("d_out_float", C.c_void_p),
        ("d_out_valid", C.c_void_p),
        ("d_workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
        ("d_result", C.c_void_p),
        ("stream", C.c_void_p),
        ("lanes", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class AlignStringResult(C.Structure):
    _fields_ = [
        ("n_capped", C.c_uint64),
        ("error_row", C.c_uint64),
        ("error_length", C.c_uint64),
        ("error_limit", C.c_uint64),
        ("n_global", C.c_uint64),
        ("out_bytes", C.c_uint64),
        ("error_code", C.c_uint32),
        ("flags", C.c_uint32),
        ("out_capacity", C.c_uint64),
    ]


class AlignStringArgs(C.Structure):
    _fields_ = [
        ("d_text", C.c_void_p),
        ("d_text_payload", C.c_void_p),
        ("text_payload_base", C.c_uint64),
        ("d_pattern", C.c_void_p),
        ("d_pattern_payload", C.c_void_p),
        ("pattern_payload_base", C.c_uint64),
        ("n_rows", C.c_uint64),
        ("mismatch", C.c_uint32),
        ("gap_opening", C.c_uint32),
        ("gap_extension", C.c_uint32),
        ("max_penalty", C.c_uint32),
        ("max_pair_bytes", C.c_uint64),
        ("d_out_strings", C.c_void_p),
        ("d_out_payload", C.c_void_p),
        ("out_capacity", C.c_uint64),
        ("out_payload_base", C.c_uint64),
        ("d_out_score", C.c_void_p),
        ("d_out_valid", C.c_void_p),
        ("d_workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
        ("d_result", C.c_void_p),
        ("stream", C.c_void_p),
        ("lanes", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class GtfScanArgs(C.Structure):
    _fields_ = [
        ("d_input", C.c_void_p),
        ("n_bytes", C.c_uint64),
        ("lead", C.c_uint64),
        ("payload_base", C.c_uint64),
        ("flags", C.c_uint32),
        ("algo", C.c_uint32),
        ("d_columns", C.c_void_p * EXG_GTF_COLUMNS),
        ("d_validity", C.c_void_p * EXG_GTF_COLUMNS),
        ("d_keep", C.c_void_p),
        ("capacity_records", C.c_uint64),
        ("d_workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
        ("d_result", C.c_void_p),
        ("stream", C.c_void_p),
    ]


class GtfAttributesResult(C.Structure):
    _fields_ = [
        ("total_entries", C.c_uint64),
        ("error_row", C.c_uint64),
        ("error_offset", C.c_uint64),
        ("n_rows", C.c_uint64),
        ("error_code", C.c_uint32),
        ("flags", C.c_uint32),
        ("error_byte", C.c_uint8),
        ("pad", C.c_uint8 * 23),
    ]


class GtfAttributesArgs(C.Structure):
    _fields_ = [
        ("d_strings", C.c_void_p),
        ("d_payload", C.c_void_p),
        ("payload_base", C.c_uint64),
        ("d_row_map", C.c_void_p),
        ("n_rows", C.c_uint64),
        ("chunk_rows", C.c_uint64),
        ("d_out_entries", C.c_void_p),
        ("d_out_chunk_base", C.c_void_p),
        ("d_out_keys", C.c_void_p),
        ("d_out_values", C.c_void_p),
        ("entries_capacity", C.c_uint64),
        ("d_workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
        ("d_result", C.c_void_p),
        ("stream", C.c_void_p),
    ]


class GffAttributesResult(C.Structure):
    _fields_ = [
        ("total_entries", C.c_uint64),
        ("error_row", C.c_uint64),
        ("error_offset", C.c_uint64),
        ("n_rows", C.c_uint64),
        ("error_code", C.c_uint32),
        ("flags", C.c_uint32),
        ("error_length", C.c_uint32),
        ("pad", C.c_uint8 * 20),
    ]


class GffAttributesArgs(C.Structure):
    """exg_gff_attributes_args: exg_gtf_attributes_args field for field"""
    _fields_ = list(GtfAttributesArgs._fields_)


class CigarResult(C.Structure):
    _fields_ = [
        ("total_ops", C.c_uint64),
        ("error_row", C.c_uint64),
        ("error_offset", C.c_uint64),
        ("n_rows", C.c_uint64),
        ("error_code", C.c_uint32),
        ("flags", C.c_uint32),
        ("error_byte", C.c_uint8),
        ("pad", C.c_uint8 * 23),
    ]


class CigarOpArgs(C.Structure):
    _fields_ = [
        ("op", C.c_uint32),
        ("d_cigar", C.c_void_p),
        ("d_cigar_payload", C.c_void_p),
        ("cigar_payload_base", C.c_uint64),
        ("d_sequence", C.c_void_p),
        ("d_sequence_payload", C.c_void_p),
        ("sequence_payload_base", C.c_uint64),
        ("n_rows", C.c_uint64),
        ("d_out_entries", C.c_void_p),
        ("d_out_op", C.c_void_p),
        ("d_out_len", C.c_void_p),
        ("ops_capacity", C.c_uint64),
        ("d_out_start", C.c_void_p),
        ("d_out_end", C.c_void_p),
        ("d_out_sequence", C.c_void_p),
        ("d_workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
        ("d_result", C.c_void_p),
        ("stream", C.c_void_p),
    ]


class OpenArgs(C.Structure):
    _fields_ = [("path", C.c_char_p), ("file_format", C.c_char_p), ("compression", C.c_char_p), ("batch_rows", C.c_uint64),
                ("device", C.c_int), ("device_batch_bytes", C.c_uint64), ("filters", C.c_char_p),
                ("shard_index", C.c_uint32), ("shard_count", C.c_uint32), ("columns", C.c_uint64), ("flags", C.c_uint64)]


class VirtualChunk(C.Structure):
    _fields_ = [("begin", C.c_uint64), ("end", C.c_uint64)]


class Region(C.Structure):
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("ref_id", C.c_uint32), ("name_len", C.c_uint32), ("name", C.c_char * 256)]


class VcfRegionArgs(C.Structure):
    _fields_ = [("d_chrom", C.c_void_p), ("d_ref", C.c_void_p), ("d_pos", C.c_void_p), ("d_info", C.c_void_p), ("d_payload", C.c_void_p),
                ("payload_base", C.c_uint64), ("n_rows", C.c_uint64), ("d_name", C.c_void_p), ("name_len", C.c_uint32), ("reserved", C.c_uint32),
                ("start", C.c_int64), ("end", C.c_int64), ("d_keep", C.c_void_p), ("stream", C.c_void_p)]


REGION_UNBOUNDED = (1 << 63) - 1


class BcfToVcfResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("consumed_bytes", C.c_uint64), ("text_bytes_needed", C.c_uint64), ("text_bytes", C.c_uint64),
                ("error_record", C.c_uint64), ("error_offset", C.c_uint64), ("error_code", C.c_uint32), ("flags", C.c_uint32),
                ("tiles_rewalked", C.c_uint64)]


class BcfToVcfArgs(C.Structure):
    _fields_ = [("d_input", C.c_void_p), ("n_bytes", C.c_uint64), ("flags", C.c_uint32), ("n_samples", C.c_uint32),
                ("d_contig_bytes", C.c_void_p), ("d_contig_table", C.c_void_p), ("n_contigs", C.c_uint32), ("n_strings", C.c_uint32),
                ("d_string_bytes", C.c_void_p), ("d_string_table", C.c_void_p), ("gt_index", C.c_uint32), ("reserved", C.c_uint32),
                ("d_output", C.c_void_p), ("output_capacity", C.c_uint64), ("d_workspace", C.c_void_p), ("workspace_bytes", C.c_uint64),
                ("d_result", C.c_void_p), ("stream", C.c_void_p)]


class InflateMember(C.Structure):
    _fields_ = [("comp_off", C.c_uint64), ("comp_size", C.c_uint64), ("out_off", C.c_uint64), ("out_cap", C.c_uint64)]


class InflateStatus(C.Structure):
    _fields_ = [("code", C.c_uint32), ("pad", C.c_uint32), ("produced", C.c_uint64), ("consumed", C.c_uint64)]


# every symbol include/exon_gpu.h declares -> (restype, argtypes); None = not yet bound by name only
SIGNATURES = {
    "exg_abi_version": (C.c_int, []),
    "exg_scan_algo_hint": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64]),
    "exg_device_count": (C.c_int, []),
    "exg_last_error_message": (C.c_char_p, []),
    "exg_parse_error_string": (C.c_char_p, [C.c_uint32]),
    "exg_scan_workspace_bytes": (C.c_uint64, [C.c_int, C.c_uint64]),
    "exg_fastq_scan": (C.c_int, [C.POINTER(FastqScanArgs)]),
    "exg_vcf_scan": (C.c_int, [C.POINTER(VcfScanArgs)]),
    "exg_fasta_scan": (C.c_int, [C.POINTER(FastaScanArgs)]),
    "exg_bam_scan": (C.c_int, [C.POINTER(BamScanArgs)]),
    "exg_bed_scan": (C.c_int, [C.POINTER(BedScanArgs)]),
    "exg_sam_scan": (C.c_int, [C.POINTER(SamScanArgs)]),
    "exg_gtf_scan": (C.c_int, [C.POINTER(GtfScanArgs)]),
    "exg_gtf_attributes_workspace_bytes": (C.c_uint64, [C.c_uint64]),
    "exg_gtf_attributes": (C.c_int, [C.POINTER(GtfAttributesArgs)]),
    "exg_gtf_attributes_result": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(GtfAttributesResult)]),
    "exg_gff_attributes_workspace_bytes": (C.c_uint64, [C.c_uint64]),
    "exg_gff_attributes": (C.c_int, [C.POINTER(GffAttributesArgs)]),
    "exg_gff_attributes_result": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(GffAttributesResult)]),
    "exg_bcf_workspace_bytes": (C.c_uint64, [C.c_uint64, C.c_uint32]),
    "exg_bcf_to_vcf": (C.c_int, [C.POINTER(BcfToVcfArgs)]),
    "exg_bcf_result": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(BcfToVcfResult)]),
    "exg_gzip_index": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                 C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "exg_inflate_members": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "exg_zstd_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p]),
    "exg_bzip2_decode": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p]),
    "exg_fetch_result": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ScanResult)]),
    "exg_count_newlines": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "exg_quality_list_workspace_bytes": (C.c_uint64, [C.c_uint64]),
    "exg_quality_score_list": (C.c_int, [C.POINTER(QualityListArgs)]),
    "exg_sequence_workspace_bytes": (C.c_uint64, [C.c_uint32, C.c_uint64]),
    "exg_sequence_op": (C.c_int, [C.POINTER(SequenceOpArgs)]),
    "exg_sequence_result": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SeqResult)]),
    "exg_align_workspace_bytes": (C.c_uint64, [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]),
    "exg_align_score": (C.c_int, [C.POINTER(AlignScoreArgs)]),
    "exg_align_result": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(AlignScoreResult)]),
    "exg_align_string_workspace_bytes": (C.c_uint64, [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64]),
    "exg_align_string": (C.c_int, [C.POINTER(AlignStringArgs)]),
    "exg_align_string_result": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(AlignStringResult)]),
    "exg_cigar_workspace_bytes": (C.c_uint64, [C.c_uint32, C.c_uint64, C.c_uint64]),
    "exg_cigar_op": (C.c_int, [C.POINTER(CigarOpArgs)]),
    "exg_cigar_result": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(CigarResult)]),
    "exg_plan_shards": (C.c_int, [C.POINTER(OpenArgs), C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.c_uint32]),
    "exg_vcf_region_keep": (C.c_int, [C.POINTER(VcfRegionArgs)]),
    "exg_tabix_query": (C.c_int, [C.c_char_p, C.c_uint64, C.c_char_p, C.POINTER(VirtualChunk), C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(Region)]),
    "exg_open_region": (C.c_int, [C.POINTER(OpenArgs), C.c_char_p, C.POINTER(C.c_void_p)]),
    "exg_vcf_query_reader": (C.c_void_p, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t]),
}


class ReaderStats(C.Structure):
    _fields_ = [("device_bytes_now", C.c_uint64), ("device_bytes_peak", C.c_uint64), ("device_mem_cap", C.c_uint64),
                ("device_batch_bytes", C.c_uint64), ("device_batches", C.c_uint64), ("decoded_segments", C.c_uint64),
                ("scan_algo", C.c_uint64), ("input_bytes", C.c_uint64), ("input_compression", C.c_uint64),
                ("nested_ns", C.c_uint64), ("host_vector_bytes", C.c_uint64), ("bam_tiles", C.c_uint64),
                ("bam_tiles_rewalked", C.c_uint64), ("reserved", C.c_uint64 * 1)]

# libexon_tf_test.so (csrc/testing/): test / bench scaffolding — synthetic inputs generated in HBM, consumers that drain a
# reader's chunks (counting, or folding every row into a digest), host-only introspection, the host-pipeline probe
TEST_SIGNATURES = {
    "exg_synth_fastq": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]),
    "exg_synth_vcf": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]),
    "exg_synth_fasta": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]),
    "exon_tf_support_error": (C.c_char_p, []),
    "exon_tf_drain_chunks": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "exon_tf_drain_arrow_vcf": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    "exon_tf_drain_formats_digest": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "exon_tf_expect_vcf_formats_file": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "exon_tf_drain_arrow_fastq": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
    "exon_tf_drain_digest": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint64)]),
    "exon_tf_drain_digest_from": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "exon_tf_synth_fastq150_host": (None, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]),
    "exon_tf_expect_fastq150": (C.c_uint64, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]),
    "exon_tf_expect_fastq_file": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "exon_tf_expect_vcf_file": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "exon_tf_filter_explain": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]),
    "exon_tf_vcf_header_explain": (C.c_int, [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]),
    "exon_tf_sequence_fn": (C.c_int, [C.c_uint32, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64]),
    "exon_tf_sam_flag": (C.c_int, [C.c_uint32, C.c_int32]),
    "exon_tf_alignment_score_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "exon_tf_alignment_score": (C.c_int, [C.c_int, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                          C.c_char_p, C.c_uint64, C.POINTER(C.c_float), C.c_char_p, C.c_uint64]),
    "exon_tf_alignment_string": (C.c_int, [C.c_int, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                           C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_char_p, C.c_uint64]),
    "exon_tf_alignment_string_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32,
                                                 C.c_void_p, C.c_uint64, C.c_void_p]),
    "exon_tf_parse_cigar": (C.c_int, [C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint64), C.c_char_p, C.c_uint64]),
    "exon_tf_extract_from_cigar": (C.c_int, [C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_uint64), C.c_char_p, C.c_uint64]),
    "exon_tf_gff_parse_attributes": (C.c_int, [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_char_p, C.c_uint64]),
    "exon_tf_parse_cigar_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "exon_tf_link_probe": (C.c_int, [C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_double)]),
    "exon_tf_host_pipeline_probe": (C.c_double, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double]),
    "exon_tf_host_zero_bounce_probe": (C.c_double, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double)]),
}
