// exg_api.hip — C-ABI entry points of the device level (include/exon_gpu.h, layer 1) and the
// library plumbing (errors, device probe, result fetch).
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include "exg_arrow.hpp"
#include "exg_bam.hpp"
#include "exg_fastq.hpp"
#include "exg_rd_format.hpp"

namespace exg {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

uint64_t gtf_slow_list_bytes();  // exg_gtf.hip: the tail of the GTF scan's workspace

}  // namespace exg

using namespace exg;

// A reader keeps six to eight HIP streams busy on its device (its scan stream, the upload stream, three decoder lanes, the
// decoded segments' host copies, a checksum stage); HIP maps streams onto GPU_MAX_HW_QUEUES = 4 hardware queues by default and
// streams that share one wait for each other's packets: measured on a BGZF FASTQ read into DataChunks, the 0.1 ms scan of a
// batch sat 23-28 ms behind the decoder lanes' kernels and the 5 ms host copies (EXG_TRACE).  The runtime reads the
// variable at the process's first HIP call.  Until round 5 a constructor of this library called setenv() for it: in a DuckDB
// process that is already multi-threaded when `LOAD exon` runs that is a data race with every getenv (glibc may move `environ`),
// and it changed the queue mapping of every other HIP user of the process.  The library does not touch the environment any
// more: whoever starts the process exports GPU_MAX_HW_QUEUES=8 (bench.py and the Python loader do, before HIP
// is initialised).

extern "C" int exg_abi_version(void) { return EXG_ABI_VERSION; }

extern "C" const char *exg_last_error_message(void) { return g_err; }

extern "C" int exg_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("no HIP device visible (%s): libexon_gpu has no CPU fallback", hipGetErrorString(e));
        return EXG_E_NO_DEVICE;
    }
    return n;
}

extern "C" const char *exg_parse_error_string(uint32_t code) {
    switch (code) {
        case EXG_PE_NONE: return "ok";
        case EXG_PE_FASTQ_NAME_PREFIX: return "invalid name prefix";           // noodles-fastq InvalidData
        case EXG_PE_FASTQ_PLUS_PREFIX: return "invalid description prefix";    // noodles-fastq InvalidData
        case EXG_PE_UNEXPECTED_EOF: return "unexpected end of file";
        case EXG_PE_INVALID_UTF8: return "invalid utf-8";
        case EXG_PE_FASTA_MISSING_PREFIX: return "missing prefix ('>')";
        case EXG_PE_FASTA_MISSING_NAME: return "missing name";
        case EXG_PE_FASTA_EMPTY_DEF: return "empty input";
        case EXG_PE_VCF_MISSING_FIELD: return "missing field";
        case EXG_PE_VCF_BAD_POS: return "invalid position";
        case EXG_PE_VCF_BAD_QUAL: return "invalid quality score";
        case EXG_PE_VCF_NO_HEADER: return "missing header";
        case EXG_PE_FIELD_TOO_LONG: return "field longer than 4 GiB";
        case EXG_PE_VCF_INFO: return "invalid info field value";
        case EXG_PE_VCF_FORMAT: return "invalid genotype field value";
        case EXG_PE_BAM_BLOCK_SIZE: return "block_size below 32";
        case EXG_PE_BAM_TRUNCATED: return "record runs past the end of the stream";
        case EXG_PE_BAM_READ_NAME: return "empty read name or read name without its NUL";
        case EXG_PE_BAM_REFERENCE_ID: return "reference id outside the header's reference list";
        case EXG_PE_BAM_FIELD_LENGTHS: return "field lengths exceed block_size";
        case EXG_PE_BAM_CIGAR_OP: return "invalid CIGAR operation";
        case EXG_PE_BAM_QUALITY: return "quality score above 93";
        case EXG_PE_BED_FIELD_COUNT: return "invalid number of BED fields (3 to 9, or 12)";
        case EXG_PE_BED_REFERENCE_NAME: return "missing reference sequence name";
        case EXG_PE_BED_POSITION: return "invalid BED position or block count";
        case EXG_PE_BED_SCORE: return "invalid BED score";
        case EXG_PE_BED_STRAND: return "invalid strand";
        case EXG_PE_BED_COLOR: return "invalid color";
        case EXG_PE_BED_BLOCKS: return "invalid block sizes or block starts";
        case EXG_PE_SEQ_INVALID_CHARACTER: return "invalid character in sequence";
        case EXG_PE_SEQ_LENGTH: return "invalid sequence length";
        case EXG_PE_SEQ_CODON: return "invalid codon";
        case EXG_PE_ALIGN_TOO_LONG: return "alignment pair too long";
        case EXG_PE_SAM_FIELD_COUNT: return "fewer than 11 SAM fields";
        case EXG_PE_SAM_EMPTY_FIELD: return "empty SAM field";
        case EXG_PE_SAM_HEADER_LINE: return "header line behind the SAM header";
        case EXG_PE_SAM_FLAG: return "invalid SAM flag";
        case EXG_PE_SAM_POSITION: return "invalid SAM position";
        case EXG_PE_SAM_MAPQ: return "invalid SAM mapping quality";
        case EXG_PE_SAM_CIGAR: return "invalid SAM CIGAR";
        case EXG_PE_SAM_LENGTHS: return "sequence and quality scores differ in length";
        case EXG_PE_CIGAR_INVALID: return "invalid CIGAR string";
        case EXG_PE_CIGAR_RANGE: return "CIGAR insertions exceed the sequence";
        case EXG_PE_BCF_RECORD_LENGTH: return "l_shared below 24";
        case EXG_PE_BCF_TRUNCATED: return "BCF record runs past the end of the stream";
        case EXG_PE_BCF_TYPE: return "invalid BCF value type";
        case EXG_PE_BCF_RESERVED_VALUE: return "reserved BCF integer value";
        case EXG_PE_BCF_OVERRUN: return "BCF value runs past its record";
        case EXG_PE_BCF_CHROM: return "CHROM outside the header's contigs";
        case EXG_PE_BCF_DICT_INDEX: return "key outside the header's dictionary";
        case EXG_PE_BCF_NO_ALLELE: return "BCF record without alleles";
        case EXG_PE_BCF_SAMPLE_COUNT: return "sample count differs from the header's";
        case EXG_PE_GTF_FIELD_COUNT: return "fewer than 9 GTF fields";
        case EXG_PE_GTF_EMPTY_FIELD: return "empty GTF seqname or type";
        case EXG_PE_GTF_POSITION: return "invalid GTF start or end";
        case EXG_PE_GTF_SCORE: return "invalid GTF score";
        case EXG_PE_GTF_STRAND: return "invalid GTF strand";
        case EXG_PE_GTF_FRAME: return "invalid GTF frame";
        case EXG_PE_GTF_ATTRIBUTES: return "invalid GTF attributes";
        case EXG_PE_GFF_ATTRIBUTES: return "invalid GFF attribute";
        default: return "unknown parse error";
    }
}

extern "C" uint64_t exg_scan_workspace_bytes(int format, uint64_t n_bytes) {
    if (format == EXG_FMT_BAM) return exg::bam::workspace_bytes(n_bytes);
    if (format == EXG_FMT_BED) {
        // the single-pass scan needs the per-tile arrays only; the general path's line index is provisioned for one line per
        // 16 bytes (a BED3 line is 16 bytes and more), never less than min(n, 1 Mi) lines: half a byte per input byte where
        // the other text formats take one.  A denser input is reported (EXG_RF_INDEX_OVERFLOW: a larger workspace indexes it)
        const FastqWsLayout l = fastq_ws_layout(n_bytes, 0);
        const uint64_t small = n_bytes < (1ull << 20) ? n_bytes : (1ull << 20);
        const uint64_t lines = (n_bytes / 16 > small ? n_bytes / 16 : small) + 8;
        return l.off_nl_pos + (lines + 2) * 8;
    }
    if (format == EXG_FMT_SAM) {
        // as for BED: the per-tile arrays, and a line index for one line per 22 bytes — the densest valid line is eleven
        // one-byte fields, 21 bytes ("q\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*"), + LF —, never less than min(n, 1 Mi) lines.  A denser
        // input holds a line that is in error; when the index overflows in front of it, EXG_RF_INDEX_OVERFLOW says so
        const FastqWsLayout l = fastq_ws_layout(n_bytes, 0);
        const uint64_t small = n_bytes < (1ull << 20) ? n_bytes : (1ull << 20);
        const uint64_t lines = (n_bytes / 22 > small ? n_bytes / 22 : small) + 8;
        return l.off_nl_pos + (lines + 2) * 8;
    }
    if (format == EXG_FMT_GTF) {
        // as for BED: the per-tile arrays and a line index for one line per 16 bytes (a feature line is 18 bytes and more; a run
        // of `#` lines is denser: the general path then says EXG_RF_INDEX_OVERFLOW, the single-pass scan has no index), and
        // behind them the list of score literals the exact float parser decides (exg_gtf.hpp)
        const FastqWsLayout l = fastq_ws_layout(n_bytes, 0);
        const uint64_t small = n_bytes < (1ull << 20) ? n_bytes : (1ull << 20);
        const uint64_t lines = (n_bytes / 16 > small ? n_bytes / 16 : small) + 8;
        return ((l.off_nl_pos + (lines + 2) * 8 + 255) & ~255ull) + gtf_slow_list_bytes();
    }
    return fastq_ws_layout(n_bytes, 0, exg_rd::format_desc(format).line_index_arrays).total_bytes;  // (FASTA keeps four arrays)
}

extern "C" int exg_fetch_result(const exg_scan_result *d_result, void *stream, exg_scan_result *out) {
    if (!d_result || !out) {
        set_error("exg_fetch_result: null pointer");
        return EXG_E_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    EXG_HIP_CHECK(hipMemcpyAsync(out, d_result, sizeof(*out), hipMemcpyDeviceToHost, s));
    EXG_HIP_CHECK(hipStreamSynchronize(s));
    return EXG_OK;
}

extern "C" int exg_fastq_scan(const exg_fastq_scan_args *a) {
    if (!a || !a->d_result || !a->d_workspace || ((uintptr_t)a->d_workspace & 255) || (a->n_bytes && !a->d_input) || ((uintptr_t)a->d_input & 15) ||
        a->lead > a->n_bytes) {
        set_error("exg_fastq_scan: bad arguments (null pointer, unaligned input or workspace, or lead > n_bytes)");
        return EXG_E_INVALID_ARG;
    }
    if (a->flags & ~EXG_F_ALL) {
        set_error("exg_fastq_scan: unknown flag bits 0x%x", a->flags & ~EXG_F_ALL);
        return EXG_E_INVALID_ARG;
    }
    if (a->capacity_records && !(a->flags & EXG_F_NO_STORE) &&
        (!a->d_name || !a->d_description || !a->d_sequence || !a->d_quality || !a->d_description_validity)) {
        set_error("exg_fastq_scan: null output column");
        return EXG_E_INVALID_ARG;
    }
    FastqWsLayout l = fastq_ws_layout(a->n_bytes, a->workspace_bytes);
    if (a->workspace_bytes < fastq_ws_layout(a->n_bytes, 0).off_nl_pos + 64) {
        set_error("exg_fastq_scan: workspace too small (%llu bytes, need %llu)",
                  (unsigned long long)a->workspace_bytes,
                  (unsigned long long)exg_scan_workspace_bytes(EXG_FMT_FASTQ, a->n_bytes));
        return EXG_E_INVALID_ARG;
    }
    FastqDev dev;
    dev.d_in = (const uint8_t *)a->d_input;
    dev.n_bytes = a->n_bytes;
    dev.lead = a->lead;
    dev.first_line_index = a->first_line_index;
    dev.payload_base = a->payload_base;
    dev.flags = a->flags;
    dev.pad = 0;
    dev.d_name = a->d_name;
    dev.d_desc = a->d_description;
    dev.d_seq = a->d_sequence;
    dev.d_qual = a->d_quality;
    dev.d_desc_valid = a->d_description_validity;
    dev.capacity = a->capacity_records;
    hipStream_t stream = (hipStream_t)a->stream;
    uint8_t *ws = (uint8_t *)a->d_workspace;
    if (a->capacity_records && !(a->flags & EXG_F_NO_STORE))
        EXG_HIP_CHECK(hipMemsetAsync(a->d_description_validity, 0, (size_t)((a->capacity_records + 63) / 64) * 8, stream));
    switch (a->algo) {
        case EXG_ALGO_MULTIPASS:
            return run_fastq_multipass(a, dev, ws, l, stream, false);
        case EXG_ALGO_FUSED:
            return run_fastq_fused(a, dev, ws, l, stream, false);
        case EXG_ALGO_FUSED_FULL:
            return run_fastq_fused(a, dev, ws, l, stream, true);
        case EXG_ALGO_AUTO: {
            int rc = run_fastq_fused(a, dev, ws, l, stream, false);
            if (rc) return rc;
            // general kernels, gated on the device by the fused kernel's overflow word
            return run_fastq_multipass(a, dev, ws, l, stream, true);
        }
        default:
            set_error("exg_fastq_scan: unknown algo %u", a->algo);
            return EXG_E_INVALID_ARG;
    }
}

// ---- quality_score_string_to_list --------------------------------------------------------------------------------
// workspace: goff (n + 1 u64) | scan scratch
extern "C" uint64_t exg_quality_list_workspace_bytes(uint64_t n_rows) {
    return (n_rows + 1 + arrow::scan_tmp_entries(n_rows)) * 8 + 64;
}

extern "C" int exg_quality_score_list(const exg_quality_list_args *a) {
    if (!a || !a->d_total || !a->d_workspace || (a->n_rows && (!a->d_strings || !a->d_entries)) ||
        (a->values_capacity && !a->d_values) || ((uintptr_t)a->d_values & 15) || ((uintptr_t)a->d_workspace & 7)) {
        set_error("exg_quality_score_list: bad arguments (null pointer or unaligned values / workspace)");
        return EXG_E_INVALID_ARG;
    }
    if (a->workspace_bytes < exg_quality_list_workspace_bytes(a->n_rows)) {
        set_error("exg_quality_score_list: workspace too small (%llu bytes, need %llu)", (unsigned long long)a->workspace_bytes,
                  (unsigned long long)exg_quality_list_workspace_bytes(a->n_rows));
        return EXG_E_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)a->stream;
    uint64_t *d_goff = (uint64_t *)a->d_workspace;
    uint64_t *d_tmp = d_goff + a->n_rows + 1;
    if (!a->n_rows) {
        EXG_HIP_CHECK(hipMemsetAsync(a->d_total, 0, 8, s));
        return EXG_OK;
    }
    const arrow::StrCol col{a->d_strings, (const uint8_t *)a->d_payload, a->payload_base};
    arrow::utf8_goff_from_col(col, nullptr, a->n_rows, d_goff, d_tmp, s);
    EXG_HIP_CHECK(hipMemcpyAsync(a->d_total, d_goff + a->n_rows, 8, hipMemcpyDeviceToDevice, s));
    arrow::quality_list(col, a->n_rows, d_goff, (arrow::ListEntry *)a->d_entries, a->d_values, a->values_capacity, s);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}
