"""Device-level scans on torch-owned HBM buffers (torch = allocator + streams only)."""
import ctypes as C

import numpy as np

try:  # torch (allocator + streams) brings a HIP runtime of its own: it must be in the process BEFORE libexon_gpu.so binds to
    import torch as _torch_module  # one, so the module that needs it imports it first (see _lib.load_library)
except ImportError:  # pragma: no cover
    _torch_module = None

from . import abi
from ._lib import ExgError, check, load_library, load_test_library


def _torch():
    import torch

    if not torch.cuda.is_available():
        raise ExgError(abi.EXG_E_NO_DEVICE, "no GPU visible to torch: the record scan has no CPU fallback")
    return torch


def stream_ptr():
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def upload(data: bytes, device="cuda", pad=64):
    """Host bytes -> 16-byte-aligned device uint8 tensor, zero padded (API contract: readable to
    round_up(n,16))."""
    torch = _torch()
    n = len(data)
    t = torch.zeros(n + pad + 16, dtype=torch.uint8, device=device)
    if n:
        t[:n].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    assert t.data_ptr() % 16 == 0
    return t


def _check_synth(rc):
    if rc != 0:
        raise ExgError(rc, (load_test_library().exon_tf_support_error() or b"").decode("utf-8", "replace"))


def synth_fastq(n_bytes, file_offset=0, seed=abi.EXG_SYNTH_FASTQ_SEED, device="cuda"):
    """file bytes [file_offset, file_offset + n_bytes) of the synthetic FASTQ-150 file, generated in HBM by the test / bench
    scaffolding library (csrc/testing/exg_synth.hip)"""
    torch = _torch()
    lib = load_test_library()
    t = torch.empty(((n_bytes + 15) // 16) * 16 + 64, dtype=torch.uint8, device=device)
    t[n_bytes:].zero_()
    _check_synth(lib.exg_synth_fastq(C.c_void_p(t.data_ptr()), file_offset, n_bytes, seed, stream_ptr()))
    return t


def _synth_two_pass(fn, n_units, cap, seed, device):
    torch = _torch()
    out = torch.zeros(cap + 64, dtype=torch.uint8, device=device)
    n = C.c_uint64(0)
    _check_synth(fn(C.c_void_p(out.data_ptr()), cap, n_units, seed, C.byref(n), stream_ptr()))
    return out, int(n.value)


def synth_vcf(n_lines, seed=abi.EXG_SYNTH_VCF_SEED, device="cuda"):
    """VCF-8 of SURVEY.md §8 D2 generated in HBM -> (uint8 tensor, n_bytes); same bytes as the oracle's synth_vcf."""
    return _synth_two_pass(load_test_library().exg_synth_vcf, n_lines, 1024 + 64 * n_lines, seed, device)


def synth_fasta(n_records, seed=0xE0A5EED0003, device="cuda"):
    """FASTA of SURVEY.md §8 D2 generated in HBM -> (uint8 tensor, n_bytes)."""
    return _synth_two_pass(load_test_library().exg_synth_fasta, n_records, 4096 + 3200 * n_records, seed, device)


class FastqScan:
    """Reusable output + workspace buffers for exg_fastq_scan on one device buffer size."""

    def __init__(self, n_bytes, capacity_records=None, device="cuda"):
        torch = _torch()
        self.lib = load_library()
        self.n_bytes = n_bytes
        self.capacity = int(capacity_records if capacity_records is not None else n_bytes // 4 + 16)
        cap = max(self.capacity, 1)
        self.cols = [torch.empty((cap, 2), dtype=torch.int64, device=device) for _ in range(4)]
        self.validity = torch.empty(((cap + 63) // 64,), dtype=torch.int64, device=device)
        self.ws_bytes = int(self.lib.exg_scan_workspace_bytes(abi.EXG_FMT_FASTQ, n_bytes))
        self.ws = torch.empty((self.ws_bytes + 255) // 8, dtype=torch.int64, device=device)
        self.result = torch.zeros(8, dtype=torch.int64, device=device)
        self.args = abi.FastqScanArgs()

    def launch(self, d_input, n_bytes=None, lead=0, first_line_index=0, payload_base=0,
               flags=abi.EXG_F_BOF | abi.EXG_F_EOF, algo=abi.EXG_ALGO_AUTO):
        a = self.args
        a.d_input = d_input.data_ptr()
        a.n_bytes = self.n_bytes if n_bytes is None else n_bytes
        a.lead = lead
        a.first_line_index = first_line_index
        a.payload_base = payload_base
        a.flags = flags
        a.algo = algo
        a.d_name, a.d_description, a.d_sequence, a.d_quality = (c.data_ptr() for c in self.cols)
        a.d_description_validity = self.validity.data_ptr()
        a.capacity_records = self.capacity
        a.d_workspace = self.ws.data_ptr()
        a.workspace_bytes = self.ws_bytes
        a.d_result = self.result.data_ptr()
        a.stream = stream_ptr().value
        check(self.lib.exg_fastq_scan(C.byref(a)))

    def fetch(self):
        r = abi.ScanResult()
        check(self.lib.exg_fetch_result(C.c_void_p(self.result.data_ptr()), stream_ptr(), C.byref(r)))
        return r

    def columns_host(self, n):
        """(4 x [n,16] uint8 string_t arrays, validity words) on the host."""
        cols = [c[:n].cpu().numpy().view(np.uint8).reshape(n, 16) for c in self.cols]
        words = self.validity[: (n + 63) // 64].cpu().numpy().view(np.uint64)
        return cols, words


def quality_score_string_to_list(strings, n_rows, d_payload, payload_base, values_capacity=None):
    """quality_score_string_to_list (reference fastq_functions/module.cpp:28-54) on a VARCHAR column that is still
    in HBM: `strings` is a [cap, 2] int64 tensor of string_t (e.g. FastqScan.cols[3]), `d_payload` the buffer its
    pointers address.  Returns (entries [n_rows, 2] int64 = DuckDB list_entry_t {offset, length}, values int32,
    total): total > len(values) means the capacity was too small and nothing was written."""
    torch = _torch()
    lib = load_library()
    dev = strings.device
    cap = int(values_capacity if values_capacity is not None else d_payload.numel())
    entries = torch.empty((max(n_rows, 1), 2), dtype=torch.int64, device=dev)
    values = torch.empty(max(cap, 4), dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    ws_bytes = int(lib.exg_quality_list_workspace_bytes(n_rows))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    a = abi.QualityListArgs()
    a.d_strings = strings.data_ptr()
    a.n_rows = n_rows
    a.d_payload = d_payload.data_ptr()
    a.payload_base = payload_base
    a.d_entries = entries.data_ptr()
    a.d_values = values.data_ptr()
    a.values_capacity = cap
    a.d_total = total.data_ptr()
    a.d_workspace = ws.data_ptr()
    a.workspace_bytes = ws_bytes
    a.stream = stream_ptr().value
    check(lib.exg_quality_score_list(C.byref(a)))
    t = int(total.item())
    return entries[:n_rows], values[:min(t, cap)], t


SEQ_OUT_BASE = 1 << 46   # string_t.ptr of sequence_op's out-of-line rows = SEQ_OUT_BASE + offset in out_payload


def sequence_op(op, strings, n_rows, d_payload, payload_base, out_capacity=None):
    """The sequence scalars (reference sequence_functions/module.cpp:30-370; op = abi.EXG_SEQ_*) on a VARCHAR column that
    is still in HBM: `strings` is a [cap, 2] int64 tensor of string_t (e.g. FastqScan.cols[2]), `d_payload` the buffer its
    pointers address.  String ops return (out_strings [n_rows, 2] int64, out_payload uint8, result): out-of-line rows
    point at SEQ_OUT_BASE + offset in out_payload; result.flags & EXG_RF_CAPACITY means out_capacity (default: the bytes of
    d_payload) was too small and nothing was written.  EXG_SEQ_GC_CONTENT returns (floats [n_rows] float32, result).
    An invalid row raises ExgError with the reference's text."""
    torch = _torch()
    lib = load_library()
    dev = strings.device
    gc = op == abi.EXG_SEQ_GC_CONTENT
    a = abi.SequenceOpArgs()
    a.op = op
    a.d_strings = strings.data_ptr()
    a.n_rows = n_rows
    a.d_payload = d_payload.data_ptr() if d_payload is not None else None
    a.payload_base = payload_base
    if gc:
        floats = torch.empty(max(n_rows, 1), dtype=torch.float32, device=dev)
        a.d_out_float = floats.data_ptr()
    else:
        cap = int(out_capacity if out_capacity is not None else (d_payload.numel() if d_payload is not None else 0))
        out_strings = torch.empty((max(n_rows, 1), 2), dtype=torch.int64, device=dev)
        out_payload = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
        a.d_out_strings, a.d_out_payload = out_strings.data_ptr(), out_payload.data_ptr()
        a.out_capacity, a.out_base = cap, SEQ_OUT_BASE
    ws_bytes = int(lib.exg_sequence_workspace_bytes(op, n_rows))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    result = torch.empty(8, dtype=torch.int64, device=dev)
    a.d_workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    a.d_result = result.data_ptr()
    a.stream = stream_ptr().value
    check(lib.exg_sequence_op(C.byref(a)))
    r = abi.SeqResult()
    check(lib.exg_sequence_result(C.c_void_p(result.data_ptr()), stream_ptr(), C.byref(r)))
    if gc:
        return floats[:n_rows], r
    return out_strings[:n_rows], out_payload[:min(int(r.total_bytes), cap)], r


def align_score(text, text_payload, text_payload_base, pattern, pattern_payload, pattern_payload_base, n_rows, max_pair_bytes,
                mismatch=4, gap_opening=6, gap_extension=2, max_penalty=0, valid=None, lanes=0):
    """alignment_score / alignment_score_wfa_gap_affine (reference alignment_functions/module.cpp:264-329) on two VARCHAR
    columns that are still in HBM: `text` and `pattern` are [cap, 2] int64 tensors of string_t (e.g. FastqScan.cols[2] of two
    scans), each with the buffer its pointers address.  Returns (scores [n_rows] float32, result): the exact optimum of the
    global gap-affine alignment as (float)(-penalty).  A row whose optimum exceeds a non-zero max_penalty gets -inf, its bit is
    cleared in `valid` (an int64 tensor of validity words, when given) and result.n_capped counts it.  A row with
    |text| + |pattern| > max_pair_bytes raises ExgError naming the lowest such row."""
    torch = _torch()
    lib = load_library()
    dev = text.device
    a = abi.AlignScoreArgs()
    a.d_text, a.d_pattern = text.data_ptr(), pattern.data_ptr()
    a.d_text_payload = text_payload.data_ptr() if text_payload is not None else None
    a.d_pattern_payload = pattern_payload.data_ptr() if pattern_payload is not None else None
    a.text_payload_base, a.pattern_payload_base = text_payload_base, pattern_payload_base
    a.n_rows = n_rows
    a.mismatch, a.gap_opening, a.gap_extension = mismatch, gap_opening, gap_extension
    a.max_penalty, a.max_pair_bytes, a.lanes = max_penalty, max_pair_bytes, lanes
    scores = torch.empty(max(n_rows, 1), dtype=torch.float32, device=dev)
    a.d_out_float = scores.data_ptr()
    a.d_out_valid = valid.data_ptr() if valid is not None else None
    ws_bytes = int(lib.exg_align_workspace_bytes(n_rows, max_pair_bytes, mismatch, gap_opening, gap_extension))
    ws = torch.empty(max(ws_bytes, 64) // 8 + 2, dtype=torch.int64, device=dev)
    result = torch.empty(8, dtype=torch.int64, device=dev)
    a.d_workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    a.d_result = result.data_ptr()
    a.stream = stream_ptr().value
    check(lib.exg_align_score(C.byref(a)))
    r = abi.AlignScoreResult()
    check(lib.exg_align_result(C.c_void_p(result.data_ptr()), stream_ptr(), C.byref(r)))
    return scores[:n_rows], r


ALIGN_OUT_BASE = 1 << 47   # string_t.ptr of align_string's out-of-line rows = ALIGN_OUT_BASE + offset in out_payload


def align_string(text, text_payload, text_payload_base, pattern, pattern_payload, pattern_payload_base, n_rows, max_pair_bytes,
                 out_capacity, mismatch=4, gap_opening=6, gap_extension=2, max_penalty=0, valid=None, lanes=0, want_score=False):
    """alignment_string / alignment_string_wfa_gap_affine (reference alignment_functions/module.cpp:150-247) on two VARCHAR
    columns that are still in HBM, addressed as in align_score.  Returns (out_strings [n_rows, 2] int64 = string_t, out_payload
    uint8, scores [n_rows] float32 or None, result): the run-length CIGAR of the optimal global alignment that the backtrace rule
    of csrc/exg_alignfn.hpp picks; a CIGAR longer than 12 bytes points at ALIGN_OUT_BASE + offset in out_payload, the offsets
    being the prefix sums of the long rows' lengths.  out_capacity = 2 * (the bytes of both columns) never overflows; a smaller
    one that does raises ExgError (EXG_E_CAPACITY) naming result.out_bytes.  The workspace grows with the square of the largest
    penalty a row may reach: give long pairs a max_penalty.  A row above it is NULL (16 zero bytes), its bit cleared in `valid`
    and counted in result.n_capped.  A row with |text| + |pattern| > max_pair_bytes raises ExgError naming the lowest such row."""
    torch = _torch()
    lib = load_library()
    dev = text.device
    a = abi.AlignStringArgs()
    a.d_text, a.d_pattern = text.data_ptr(), pattern.data_ptr()
    a.d_text_payload = text_payload.data_ptr() if text_payload is not None else None
    a.d_pattern_payload = pattern_payload.data_ptr() if pattern_payload is not None else None
    a.text_payload_base, a.pattern_payload_base = text_payload_base, pattern_payload_base
    a.n_rows = n_rows
    a.mismatch, a.gap_opening, a.gap_extension = mismatch, gap_opening, gap_extension
    a.max_penalty, a.max_pair_bytes, a.lanes = max_penalty, max_pair_bytes, lanes
    out_strings = torch.empty((max(n_rows, 1), 2), dtype=torch.int64, device=dev)
    out_payload = torch.empty(max(int(out_capacity), 16), dtype=torch.uint8, device=dev)
    scores = torch.empty(max(n_rows, 1), dtype=torch.float32, device=dev) if want_score else None
    a.d_out_strings, a.d_out_payload = out_strings.data_ptr(), out_payload.data_ptr()
    a.out_capacity, a.out_payload_base = int(out_capacity), ALIGN_OUT_BASE
    a.d_out_score = scores.data_ptr() if want_score else None
    a.d_out_valid = valid.data_ptr() if valid is not None else None
    ws_bytes = int(lib.exg_align_string_workspace_bytes(n_rows, max_pair_bytes, mismatch, gap_opening, gap_extension, max_penalty, int(out_capacity)))
    if not ws_bytes:
        raise ExgError(abi.EXG_E_INVALID_ARG, "align_string: parameters out of range, or a wavefront history above 2^48 bytes (set max_penalty)")
    ws = torch.empty(ws_bytes // 8 + 2, dtype=torch.int64, device=dev)
    result = torch.empty(8, dtype=torch.int64, device=dev)
    a.d_workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    a.d_result = result.data_ptr()
    a.stream = stream_ptr().value
    check(lib.exg_align_string(C.byref(a)))
    r = abi.AlignStringResult()
    check(lib.exg_align_string_result(C.c_void_p(result.data_ptr()), stream_ptr(), C.byref(r)))
    return out_strings[:n_rows], out_payload[:int(r.out_bytes)], (scores[:n_rows] if want_score else None), r


def _cigar_call(a, n_rows, cigar, cigar_payload, cigar_payload_base, cigar_payload_bytes):
    """the common half of a exg_cigar_op call: the cigar column, workspace and result block; runs it and fetches the result"""
    torch = _torch()
    lib = load_library()
    dev = cigar.device
    a.d_cigar, a.n_rows = cigar.data_ptr(), n_rows
    a.d_cigar_payload = cigar_payload.data_ptr() if cigar_payload is not None else None
    a.cigar_payload_base = cigar_payload_base
    if cigar_payload_bytes is None:
        cigar_payload_bytes = cigar_payload.numel() if cigar_payload is not None else 0
    ws_bytes = int(lib.exg_cigar_workspace_bytes(a.op, n_rows, cigar_payload_bytes))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    result = torch.empty(8, dtype=torch.int64, device=dev)
    a.d_workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    a.d_result = result.data_ptr()
    a.stream = stream_ptr().value
    check(lib.exg_cigar_op(C.byref(a)))
    r = abi.CigarResult()
    check(lib.exg_cigar_result(C.c_void_p(result.data_ptr()), stream_ptr(), C.byref(r)))
    return r


def parse_cigar(cigar, n_rows, cigar_payload, cigar_payload_base, ops_capacity=None, cigar_payload_bytes=None):
    """parse_cigar (reference sam_functions/module.cpp:32-77) on a cigar column that is still in HBM: `cigar` is a [cap, 2] int64
    tensor of string_t (BamScan.cols[6] / SamScan.cols[6]), `cigar_payload` the buffer its pointers address.  Returns (entries
    [n_rows, 2] int64 = DuckDB list_entry_t {offset, length}, op [total, 2] int64 = string_t of one letter, len [total] int32,
    result).  ops_capacity=None is the two-call form: a counting call, then the exact capacity; with a capacity given,
    result.flags & EXG_RF_CAPACITY means it was too small and the children were not written.  `cigar_payload_bytes`: an upper
    bound of the bytes of the rows longer than 12 (default: the payload tensor's size).  An invalid row raises ExgError."""
    torch = _torch()
    dev = cigar.device
    a = abi.CigarOpArgs()
    a.op = abi.EXG_CIGAR_PARSE
    if ops_capacity is None:
        ops_capacity = int(_cigar_call(a, n_rows, cigar, cigar_payload, cigar_payload_base, cigar_payload_bytes).total_ops)
    cap = int(ops_capacity)
    entries = torch.empty((max(n_rows, 1), 2), dtype=torch.int64, device=dev)
    op = torch.empty((max(cap, 1), 2), dtype=torch.int64, device=dev)
    length = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    a.d_out_entries, a.d_out_op, a.d_out_len, a.ops_capacity = entries.data_ptr(), op.data_ptr(), length.data_ptr(), cap
    r = _cigar_call(a, n_rows, cigar, cigar_payload, cigar_payload_base, cigar_payload_bytes)
    k = min(int(r.total_ops), cap)
    return entries[:n_rows], op[:k], length[:k], r


def extract_from_cigar(sequence, sequence_payload, sequence_payload_base, cigar, cigar_payload, cigar_payload_base, n_rows,
                       cigar_payload_bytes=None):
    """extract_from_cigar (reference sam_functions/module.cpp:79-131) on the sequence and cigar columns of a scan that are still
    in HBM ([cap, 2] int64 tensors of string_t, each with the buffer its pointers address).  Returns (start [n_rows] int32, end
    [n_rows] int32, slices [n_rows, 2] int64 = string_t, result): a slice of up to 12 bytes is inlined, a longer one points into
    the caller's sequence payload (sequence_payload_base + offset).  An invalid row raises ExgError."""
    torch = _torch()
    dev = cigar.device
    a = abi.CigarOpArgs()
    a.op = abi.EXG_CIGAR_EXTRACT
    a.d_sequence = sequence.data_ptr()
    a.d_sequence_payload = sequence_payload.data_ptr() if sequence_payload is not None else None
    a.sequence_payload_base = sequence_payload_base
    start = torch.empty(max(n_rows, 1), dtype=torch.int32, device=dev)
    end = torch.empty(max(n_rows, 1), dtype=torch.int32, device=dev)
    slices = torch.empty((max(n_rows, 1), 2), dtype=torch.int64, device=dev)
    a.d_out_start, a.d_out_end, a.d_out_sequence = start.data_ptr(), end.data_ptr(), slices.data_ptr()
    r = _cigar_call(a, n_rows, cigar, cigar_payload, cigar_payload_base, cigar_payload_bytes)
    return start[:n_rows], end[:n_rows], slices[:n_rows], r


class VcfScan:
    """Reusable output + workspace buffers for exg_vcf_scan."""

    FIELDS = ["chrom", "pos", "id", "ref", "alt", "qual", "filter", "info", "formats"]

    def __init__(self, n_bytes, capacity_records=None, device="cuda"):
        torch = _torch()
        self.lib = load_library()
        self.n_bytes = n_bytes
        self.capacity = int(capacity_records if capacity_records is not None else n_bytes // 8 + 16)
        cap = max(self.capacity, 1)
        self.cols = [torch.empty((cap, 2), dtype=torch.int64, device=device) for _ in range(9)]
        self.pos = torch.empty((cap,), dtype=torch.int64, device=device)
        self.qual = torch.empty((cap,), dtype=torch.float32, device=device)
        self.qual_valid = torch.empty(((cap + 63) // 64,), dtype=torch.int64, device=device)
        self.formats_valid = torch.empty(((cap + 63) // 64,), dtype=torch.int64, device=device)
        self.ws_bytes = int(self.lib.exg_scan_workspace_bytes(abi.EXG_FMT_VCF, n_bytes))
        self.ws = torch.empty((self.ws_bytes + 255) // 8, dtype=torch.int64, device=device)
        self.result = torch.zeros(8, dtype=torch.int64, device=device)
        self.args = abi.VcfScanArgs()

    def launch(self, d_input, n_bytes=None, lead=0, payload_base=0, flags=abi.EXG_F_BOF | abi.EXG_F_EOF,
               algo=abi.EXG_ALGO_AUTO, project=None):
        a = self.args
        a.d_input = d_input.data_ptr()
        a.n_bytes = self.n_bytes if n_bytes is None else n_bytes
        a.lead = lead
        a.payload_base = payload_base
        a.flags = flags
        a.algo = algo
        for k in range(9):
            a.d_fields[k] = self.cols[k].data_ptr() if (project is None or k in project) else None
        a.d_pos = self.pos.data_ptr()
        a.d_qual = self.qual.data_ptr()
        a.d_qual_validity = self.qual_valid.data_ptr()
        a.d_formats_validity = self.formats_valid.data_ptr()
        a.capacity_records = self.capacity
        a.d_workspace = self.ws.data_ptr()
        a.workspace_bytes = self.ws_bytes
        a.d_result = self.result.data_ptr()
        a.stream = stream_ptr().value
        check(self.lib.exg_vcf_scan(C.byref(a)))

    def fetch(self):
        r = abi.ScanResult()
        check(self.lib.exg_fetch_result(C.c_void_p(self.result.data_ptr()), stream_ptr(), C.byref(r)))
        return r

    def host(self, n):
        cols = [c[:n].cpu().numpy().view(np.uint8).reshape(n, 16) for c in self.cols]
        nw = (n + 63) // 64
        return dict(cols=cols, pos=self.pos[:n].cpu().numpy(), qual=self.qual[:n].cpu().numpy(),
                    qual_valid=self.qual_valid[:nw].cpu().numpy().view(np.uint64),
                    formats_valid=self.formats_valid[:nw].cpu().numpy().view(np.uint64))


class FastaScan:
    """Reusable output + workspace buffers for exg_fasta_scan (whole-file buffers)."""

    def __init__(self, n_bytes, capacity_records=None, device="cuda"):
        torch = _torch()
        self.lib = load_library()
        self.n_bytes = n_bytes
        self.capacity = int(capacity_records if capacity_records is not None else n_bytes // 2 + 16)
        cap = max(self.capacity, 1)
        self.cols = [torch.empty((cap, 2), dtype=torch.int64, device=device) for _ in range(3)]
        self.validity = torch.empty(((cap + 63) // 64,), dtype=torch.int64, device=device)
        self.payload = torch.empty((n_bytes + 64,), dtype=torch.uint8, device=device)
        self.ws_bytes = int(self.lib.exg_scan_workspace_bytes(abi.EXG_FMT_FASTA, n_bytes))
        self.ws = torch.empty((self.ws_bytes + 255) // 8, dtype=torch.int64, device=device)
        self.result = torch.zeros(8, dtype=torch.int64, device=device)
        self.args = abi.FastaScanArgs()

    def launch(self, d_input, payload_base=0, seq_payload_base=0, flags=abi.EXG_F_BOF | abi.EXG_F_EOF, lead=0,
               algo=abi.EXG_ALGO_AUTO):
        a = self.args
        a.d_input = d_input.data_ptr()
        a.n_bytes = self.n_bytes
        a.lead = lead
        a.payload_base = payload_base
        a.seq_payload_base = seq_payload_base
        a.flags = flags
        a.algo = algo
        a.d_id, a.d_description, a.d_sequence = (c.data_ptr() for c in self.cols)
        a.d_description_validity = self.validity.data_ptr()
        a.d_seq_payload = self.payload.data_ptr()
        a.capacity_records = self.capacity
        a.d_workspace = self.ws.data_ptr()
        a.workspace_bytes = self.ws_bytes
        a.d_result = self.result.data_ptr()
        a.stream = stream_ptr().value
        check(self.lib.exg_fasta_scan(C.byref(a)))

    def fetch(self):
        r = abi.ScanResult()
        check(self.lib.exg_fetch_result(C.c_void_p(self.result.data_ptr()), stream_ptr(), C.byref(r)))
        return r

    def host(self, n, payload_bytes):
        cols = [c[:n].cpu().numpy().view(np.uint8).reshape(n, 16) for c in self.cols]
        words = self.validity[: (n + 63) // 64].cpu().numpy().view(np.uint64)
        return cols, words, self.payload[:payload_bytes].cpu().numpy()


class BamScan:
    """exg_bam_scan on decoded BAM records resident in HBM (d_input[0] is a record start): buffers for all ten columns, the
    side buffer and the reference table; rows() decodes what came back into the tuples tests compare (bytes / int / None)."""
    SIDE_BASE, REF_BASE = 1 << 44, 1 << 45
    INT_COLS, NULLABLE = (1, 3, 4), (2, 3, 4, 5, 7)

    def __init__(self, n_bytes, refs=(), capacity_records=None, side_capacity=None, device="cuda"):
        torch = _torch()
        self.lib = load_library()
        self.n_bytes = n_bytes
        self.capacity = int(capacity_records if capacity_records is not None else n_bytes // 36 + 2)
        cap = max(self.capacity, 1)
        self.cols = [torch.empty((cap,), dtype=torch.int32, device=device) if c in self.INT_COLS else
                     torch.empty((cap, 2), dtype=torch.int64, device=device) for c in range(abi.EXG_BAM_COLUMNS)]
        self.validity = {c: torch.empty(((cap + 63) // 64,), dtype=torch.int64, device=device) for c in self.NULLABLE}
        self.side_capacity = int(side_capacity if side_capacity is not None else 3 * n_bytes + 64)
        self.side = torch.empty(max(self.side_capacity, 1), dtype=torch.uint8, device=device)
        self.ref_names = b"".join(name for name, _ in refs)
        offs = [0]
        for name, _ in refs:
            offs.append(offs[-1] + len(name))
        self.n_ref = len(refs)
        self.d_ref_names = upload(self.ref_names)
        self.d_ref_offsets = torch.tensor(offs, dtype=torch.int64, device=device)
        self.ws_bytes = int(self.lib.exg_scan_workspace_bytes(abi.EXG_FMT_BAM, n_bytes))
        self.ws = torch.empty((self.ws_bytes + 255) // 8, dtype=torch.int64, device=device)
        self.result = torch.zeros(8, dtype=torch.int64, device=device)
        self.args = abi.BamScanArgs()

    def launch(self, d_input, n_bytes=None, flags=abi.EXG_F_EOF, columns=0):
        a = self.args
        a.d_input = d_input.data_ptr() if hasattr(d_input, "data_ptr") else d_input
        a.n_bytes = self.n_bytes if n_bytes is None else n_bytes
        a.flags, a.n_ref, a.columns = flags, self.n_ref, columns
        a.d_ref_names, a.d_ref_offsets, a.ref_names_base = self.d_ref_names.data_ptr(), self.d_ref_offsets.data_ptr(), self.REF_BASE
        for c in range(abi.EXG_BAM_COLUMNS):
            a.d_columns[c] = self.cols[c].data_ptr()
            a.d_validity[c] = self.validity[c].data_ptr() if c in self.validity else None
        a.d_side, a.side_capacity, a.side_base = self.side.data_ptr(), self.side_capacity, self.SIDE_BASE
        a.capacity_records = self.capacity
        a.d_workspace, a.workspace_bytes = self.ws.data_ptr(), self.ws_bytes
        a.d_result = self.result.data_ptr()
        a.stream = stream_ptr().value
        check(self.lib.exg_bam_scan(C.byref(a)))

    def fetch(self):
        r = abi.BamScanResult()
        check(self.lib.exg_fetch_result(C.c_void_p(self.result.data_ptr()), stream_ptr(), C.cast(C.byref(r), C.POINTER(abi.ScanResult))))
        return r

    def rows(self, n, side_bytes):
        """the first n rows as tuples of the ten columns"""
        side = self.side[:side_bytes].cpu().numpy().tobytes()
        out = []
        for c in range(abi.EXG_BAM_COLUMNS):
            valid = None
            if c in self.validity:
                words = self.validity[c][: (n + 63) // 64].cpu().numpy().view(np.uint64)
                valid = np.unpackbits(words.view(np.uint8), bitorder="little")[:n]
            if c in self.INT_COLS:
                vals = self.cols[c][:n].cpu().numpy().tolist()
            else:
                raw = self.cols[c][:n].cpu().numpy().view(np.uint8).reshape(n, 16)
                lens = raw[:, :4].copy().view(np.uint32).reshape(n)
                ptrs = raw[:, 8:16].copy().view(np.uint64).reshape(n)
                vals = []
                for i in range(n):
                    ln = int(lens[i])
                    if ln <= 12:
                        vals.append(raw[i, 4:4 + ln].tobytes())
                        continue
                    p = int(ptrs[i])
                    if p >= self.REF_BASE:
                        vals.append(self.ref_names[p - self.REF_BASE:p - self.REF_BASE + ln])
                    else:
                        s = side[p - self.SIDE_BASE:p - self.SIDE_BASE + ln]
                        assert len(s) == ln and s[:4] == raw[i, 4:8].tobytes(), "string_t outside the side buffer, or a wrong prefix"
                        vals.append(s)
            out.append([v if valid is None or valid[i] else None for i, v in enumerate(vals)])
        return list(zip(*out))


class BedScan:
    """exg_bed_scan on BED text resident in HBM: buffers for all twelve columns; rows() decodes what came back into the
    tuples tests compare (bytes / int / None), the strings out of the input bytes the caller hands it."""
    NAMES = ["reference_sequence_name", "start", "end", "name", "score", "strand", "thick_start", "thick_end", "color",
             "block_count", "block_sizes", "block_starts"]
    INT_COLS, NULLABLE = (1, 2, 4, 6, 7, 9), tuple(range(3, 12))
    PAYLOAD_BASE = 1 << 44
    # what SamScan overrides: the column count, the integer columns' width, the format, the args struct and the entry point
    N_COLS, INT_DTYPE, FMT, ARGS, ENTRY = abi.EXG_BED_COLUMNS, "int64", abi.EXG_FMT_BED, abi.BedScanArgs, "exg_bed_scan"

    def __init__(self, n_bytes, capacity_records=None, device="cuda"):
        torch = _torch()
        self.lib = load_library()
        self.n_bytes = n_bytes
        self.capacity = int(capacity_records if capacity_records is not None else n_bytes // 2 + 16)
        cap = max(self.capacity, 1)
        self.cols = [torch.empty((cap,), dtype=getattr(torch, self.INT_DTYPE), device=device) if c in self.INT_COLS else
                     torch.empty((cap, 2), dtype=torch.int64, device=device) for c in range(self.N_COLS)]
        self.validity = {c: torch.empty(((cap + 63) // 64,), dtype=torch.int64, device=device) for c in self.NULLABLE}
        self.ws_bytes = int(self.lib.exg_scan_workspace_bytes(self.FMT, n_bytes))
        self.ws = torch.empty((self.ws_bytes + 255) // 8, dtype=torch.int64, device=device)
        self.result = torch.zeros(8, dtype=torch.int64, device=device)
        self.args = self.ARGS()

    def launch(self, d_input, n_bytes=None, lead=0, payload_base=None, flags=abi.EXG_F_BOF | abi.EXG_F_EOF,
               algo=abi.EXG_ALGO_AUTO, project=None):
        a = self.args
        a.d_input = d_input.data_ptr()
        a.n_bytes = self.n_bytes if n_bytes is None else n_bytes
        a.lead = lead
        a.payload_base = self.PAYLOAD_BASE if payload_base is None else payload_base
        a.flags, a.algo = flags, algo
        for c in range(self.N_COLS):
            on = project is None or c in project
            a.d_columns[c] = self.cols[c].data_ptr() if on else None
            a.d_validity[c] = self.validity[c].data_ptr() if on and c in self.validity else None
        a.capacity_records = self.capacity
        a.d_workspace, a.workspace_bytes = self.ws.data_ptr(), self.ws_bytes
        a.d_result = self.result.data_ptr()
        a.stream = stream_ptr().value
        check(getattr(self.lib, self.ENTRY)(C.byref(a)))

    def fetch(self):
        r = abi.ScanResult()
        check(self.lib.exg_fetch_result(C.c_void_p(self.result.data_ptr()), stream_ptr(), C.byref(r)))
        return r

    def host(self, n):
        """raw columns ([n,16] uint8 string_t / int64) and validity words of the first n rows"""
        nw = (n + 63) // 64
        cols = [self.cols[c][:n].cpu().numpy() if c in self.INT_COLS else self.cols[c][:n].cpu().numpy().view(np.uint8).reshape(n, 16)
                for c in range(self.N_COLS)]
        return cols, {c: v[:nw].cpu().numpy().view(np.uint64) for c, v in self.validity.items()}

    def rows(self, n, data: bytes, columns=None, payload_base=None):
        """the first n rows as tuples of the (selected) columns; `data`: the bytes d_input holds"""
        base = self.PAYLOAD_BASE if payload_base is None else payload_base
        cols, words = self.host(n)
        out = []
        for c in (range(self.N_COLS) if columns is None else columns):
            valid = np.unpackbits(words[c].view(np.uint8), bitorder="little")[:n] if c in words else None
            if c in self.INT_COLS:
                vals = cols[c].tolist()
            else:
                raw = cols[c]
                lens = raw[:, :4].copy().view(np.uint32).reshape(n)
                ptrs = raw[:, 8:16].copy().view(np.uint64).reshape(n)
                vals = []
                for i in range(n):
                    ln = int(lens[i])
                    if ln <= 12:
                        assert not raw[i, 4 + ln:].any(), "inlined string_t is not zero padded"
                        vals.append(raw[i, 4:4 + ln].tobytes())
                    else:
                        o = int(ptrs[i]) - base
                        s = data[o:o + ln]
                        assert 0 <= o and len(s) == ln and s[:4] == raw[i, 4:8].tobytes(), "string_t outside the input, or a wrong prefix"
                        vals.append(s)
            if valid is not None:
                for i in range(n):
                    if not valid[i]:
                        assert not np.asarray(cols[c][i]).any(), "a NULL value does not hold zeros"
                        vals[i] = None
            out.append(vals)
        return list(zip(*out))


class SamScan(BedScan):
    """exg_sam_scan on SAM alignment lines (no header) resident in HBM: BedScan's buffers and decoding with BAM's ten columns,
    the three INTEGER ones 4 bytes wide."""
    NAMES = ["name", "flag", "reference", "start", "end", "mapping_quality", "cigar", "mate_reference", "sequence", "quality_score"]
    INT_COLS, NULLABLE = (1, 3, 4), (2, 3, 4, 5, 7)
    N_COLS, INT_DTYPE, FMT, ARGS, ENTRY = abi.EXG_SAM_COLUMNS, "int32", abi.EXG_FMT_SAM, abi.SamScanArgs, "exg_sam_scan"


class GtfScan(BedScan):
    """exg_gtf_scan on GTF lines resident in HBM: BedScan's buffers and decoding with GTF's nine columns (start / end int64,
    score float32, column 8 the raw ninth field) and the keep words.  The scan numbers rows by LINES: rows(n, ...) gives the
    rows of the feature lines among the first n (those whose bit is set in d_keep); kept(n) says which they are.
    `workspace_bytes`: a workspace larger than exg_scan_workspace_bytes (the general path on runs of `#` lines)."""
    NAMES = ["seqname", "source", "type", "start", "end", "score", "strand", "frame", "attributes"]
    INT_COLS, NULLABLE = (3, 4), (5, 6, 7)
    N_COLS, INT_DTYPE, FMT, ARGS, ENTRY = abi.EXG_GTF_COLUMNS, "int64", abi.EXG_FMT_GTF, abi.GtfScanArgs, "exg_gtf_scan"

    def __init__(self, n_bytes, capacity_records=None, device="cuda", workspace_bytes=None):
        super().__init__(n_bytes, capacity_records, device)
        torch = _torch()
        cap = max(self.capacity, 1)
        self.cols[5] = torch.empty((cap,), dtype=torch.float32, device=device)
        self.keep = torch.zeros(((cap + 63) // 64,), dtype=torch.int64, device=device)
        if workspace_bytes is not None and workspace_bytes > self.ws_bytes:
            self.ws_bytes = int(workspace_bytes)
            self.ws = torch.empty((self.ws_bytes + 255) // 8, dtype=torch.int64, device=device)
        self.args.d_keep = self.keep.data_ptr()

    def kept(self, n):
        """bool per row of the first n: the line is a feature line"""
        words = self.keep[:(n + 63) // 64].cpu().numpy().view(np.uint64)
        return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)

    def host(self, n):
        nw = (n + 63) // 64
        cols = [self.cols[c][:n].cpu().numpy() if c in self.INT_COLS or c == 5 else self.cols[c][:n].cpu().numpy().view(np.uint8).reshape(n, 16)
                for c in range(self.N_COLS)]
        return cols, {c: v[:nw].cpu().numpy().view(np.uint64) for c, v in self.validity.items()}

    def rows(self, n, data: bytes, columns=None, payload_base=None):
        """the rows of the feature lines among the first n lines; score as the float32's bit pattern (an int), NULL as None"""
        base = self.PAYLOAD_BASE if payload_base is None else payload_base
        keep = self.kept(n)
        cols, words = self.host(n)
        out = []
        for c in (range(self.N_COLS) if columns is None else columns):
            valid = np.unpackbits(words[c].view(np.uint8), bitorder="little")[:n] if c in words else None
            if c in self.INT_COLS:
                vals = cols[c].tolist()
            elif c == 5:
                vals = cols[c].view(np.uint32).tolist()
            else:
                raw = cols[c]
                lens = raw[:, :4].copy().view(np.uint32).reshape(n)
                ptrs = raw[:, 8:16].copy().view(np.uint64).reshape(n)
                vals = []
                for i in range(n):
                    ln = int(lens[i])
                    if not keep[i]:
                        vals.append(None)
                    elif ln <= 12:
                        assert not raw[i, 4 + ln:].any(), "inlined string_t is not zero padded"
                        vals.append(raw[i, 4:4 + ln].tobytes())
                    else:
                        o = int(ptrs[i]) - base
                        s = data[o:o + ln]
                        assert 0 <= o and len(s) == ln and s[:4] == raw[i, 4:8].tobytes(), "string_t outside the input, or a wrong prefix"
                        vals.append(s)
            if valid is not None:
                for i in range(n):
                    if keep[i] and not valid[i]:
                        assert not np.asarray(cols[c][i]).any(), "a NULL value does not hold zeros"
                        vals[i] = None
            out.append(vals)
        return [row for row, k in zip(zip(*out), keep) if k]


def gtf_attributes(strings, n_rows, payload, payload_base, entries_capacity=None, row_map=None, chunk_rows=0):
    """exg_gtf_attributes on a column of GTF ninth fields that is still in HBM: `strings` is a [cap, 2] int64 tensor of string_t
    (GtfScan.cols[8]), `payload` the buffer its pointers address, `row_map` an optional int32 tensor of n_rows row numbers.
    Returns (entries [n_rows, 2] int64 = DuckDB list_entry_t {offset, length}, keys [total, 2] int64, values [total, 2] int64 —
    string_t that point into the same payload —, chunk_base or None, result).  entries_capacity=None is the two-call form: a
    counting call, then the exact capacity; with a capacity given, result.flags & EXG_RF_CAPACITY means it was too small and the
    children were not written.  An invalid row raises ExgError (the result block rides on it as .result)."""
    torch = _torch()
    lib = load_library()
    dev = strings.device
    a = abi.GtfAttributesArgs()
    a.d_strings = strings.data_ptr()
    a.d_payload = payload.data_ptr() if payload is not None else None
    a.payload_base = payload_base
    a.d_row_map = row_map.data_ptr() if row_map is not None else None
    a.n_rows = n_rows
    ws_bytes = int(lib.exg_gtf_attributes_workspace_bytes(n_rows))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    result = torch.empty(8, dtype=torch.int64, device=dev)
    a.d_workspace, a.workspace_bytes, a.d_result, a.stream = ws.data_ptr(), ws_bytes, result.data_ptr(), stream_ptr().value

    def call():
        check(lib.exg_gtf_attributes(C.byref(a)))
        r = abi.GtfAttributesResult()
        rc = lib.exg_gtf_attributes_result(C.c_void_p(result.data_ptr()), stream_ptr(), C.byref(r))
        if rc != 0:
            try:
                check(rc)
            except ExgError as e:
                e.result = r
                raise
        return r

    if entries_capacity is None:
        entries_capacity = int(call().total_entries)
    cap = int(entries_capacity)
    entries = torch.zeros((max(n_rows, 1), 2), dtype=torch.int64, device=dev)
    keys = torch.zeros((max(cap, 1), 2), dtype=torch.int64, device=dev)
    values = torch.zeros((max(cap, 1), 2), dtype=torch.int64, device=dev)
    bases = torch.zeros(((n_rows + chunk_rows - 1) // chunk_rows + 1,), dtype=torch.int64, device=dev) if chunk_rows else None
    a.d_out_entries, a.d_out_keys, a.d_out_values, a.entries_capacity = entries.data_ptr(), keys.data_ptr(), values.data_ptr(), cap
    a.chunk_rows, a.d_out_chunk_base = chunk_rows, bases.data_ptr() if chunk_rows else None
    r = call()
    k = min(int(r.total_entries), cap) if not (r.flags & abi.EXG_RF_CAPACITY) else 0
    return entries[:n_rows], keys[:k], values[:k], bases, r


def gff_attributes(strings, n_rows, payload, payload_base, entries_capacity=None, row_map=None, chunk_rows=0):
    """exg_gff_attributes (gff_parse_attributes, reference gff_functions/module.cpp:29-84) on a column of GFF3 ninth fields that
    is still in HBM: arguments and return value are gtf_attributes' — (entries [n_rows, 2] int64 = list_entry_t {offset, length},
    keys [total, 2] int64, values [total, 2] int64 — string_t slices of the same payload —, chunk_base or None, result).
    entries_capacity=None is the two-call form.  An invalid row raises ExgError; the result block rides on it as .result
    (error_row, error_offset and error_length: the failing segment behind its trim)."""
    torch = _torch()
    lib = load_library()
    dev = strings.device
    a = abi.GffAttributesArgs()
    a.d_strings = strings.data_ptr()
    a.d_payload = payload.data_ptr() if payload is not None else None
    a.payload_base = payload_base
    a.d_row_map = row_map.data_ptr() if row_map is not None else None
    a.n_rows = n_rows
    ws_bytes = int(lib.exg_gff_attributes_workspace_bytes(n_rows))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    result = torch.empty(8, dtype=torch.int64, device=dev)
    a.d_workspace, a.workspace_bytes, a.d_result, a.stream = ws.data_ptr(), ws_bytes, result.data_ptr(), stream_ptr().value

    def call():
        check(lib.exg_gff_attributes(C.byref(a)))
        r = abi.GffAttributesResult()
        rc = lib.exg_gff_attributes_result(C.c_void_p(result.data_ptr()), stream_ptr(), C.byref(r))
        if rc != 0:
            try:
                check(rc)
            except ExgError as e:
                e.result = r
                raise
        return r

    if entries_capacity is None:
        entries_capacity = int(call().total_entries)
    cap = int(entries_capacity)
    entries = torch.zeros((max(n_rows, 1), 2), dtype=torch.int64, device=dev)
    keys = torch.zeros((max(cap, 1), 2), dtype=torch.int64, device=dev)
    values = torch.zeros((max(cap, 1), 2), dtype=torch.int64, device=dev)
    bases = torch.zeros(((n_rows + chunk_rows - 1) // chunk_rows + 1,), dtype=torch.int64, device=dev) if chunk_rows else None
    a.d_out_entries, a.d_out_keys, a.d_out_values, a.entries_capacity = entries.data_ptr(), keys.data_ptr(), values.data_ptr(), cap
    a.chunk_rows, a.d_out_chunk_base = chunk_rows, bases.data_ptr() if chunk_rows else None
    r = call()
    k = min(int(r.total_entries), cap) if not (r.flags & abi.EXG_RF_CAPACITY) else 0
    return entries[:n_rows], keys[:k], values[:k], bases, r


class BcfToVcf:
    """exg_bcf_to_vcf on decoded BCF records resident in HBM (d_input[0] is a record start): the two dictionaries as lists indexed
    by dictionary index (bytes, or None where no ID has that index), the header's sample count, an output buffer of
    `output_capacity` bytes.  run() returns (result block, the text written)."""

    def __init__(self, n_bytes, strings, contigs, n_samples=0, output_capacity=None, device="cuda"):
        torch = _torch()
        self.lib = load_library()
        self.n_bytes, self.n_samples = n_bytes, n_samples
        self.gt_index = strings.index(b"GT") if b"GT" in strings else 0xFFFFFFFF
        self.dicts = []
        for names in (contigs, strings):
            table, data = [], b""
            for name in names:
                table += [len(data), 0xFFFFFFFF if name is None else len(name)]
                data += name or b""
            d_table = torch.from_numpy(np.array(table + [0, 0], dtype=np.uint32).view(np.int32)).to(device)
            self.dicts.append((upload(data + b"\0"), d_table, len(names)))
        self.output_capacity = int(output_capacity if output_capacity is not None else 8 * n_bytes + 4096)
        self.out = torch.empty(max(self.output_capacity, 1) + 64, dtype=torch.uint8, device=device)
        self.ws_bytes = int(self.lib.exg_bcf_workspace_bytes(n_bytes, n_samples))
        self.ws = torch.empty((self.ws_bytes + 255) // 8, dtype=torch.int64, device=device)
        self.result = torch.zeros(8, dtype=torch.int64, device=device)
        self.args = abi.BcfToVcfArgs()

    def launch(self, d_input, n_bytes=None, flags=abi.EXG_F_EOF, output_capacity=None):
        """one call (it synchronises) -> the result block"""
        a = self.args
        cap = self.output_capacity if output_capacity is None else output_capacity
        assert cap <= self.output_capacity
        a.d_input = d_input.data_ptr() if hasattr(d_input, "data_ptr") else d_input
        a.n_bytes = self.n_bytes if n_bytes is None else n_bytes
        a.flags, a.n_samples = flags, self.n_samples
        (cb, ct, cn), (sb, st, sn) = self.dicts
        a.d_contig_bytes, a.d_contig_table, a.n_contigs = cb.data_ptr(), ct.data_ptr(), cn
        a.d_string_bytes, a.d_string_table, a.n_strings = sb.data_ptr(), st.data_ptr(), sn
        a.gt_index = self.gt_index
        a.d_output, a.output_capacity = self.out.data_ptr(), cap
        a.d_workspace, a.workspace_bytes = self.ws.data_ptr(), self.ws_bytes
        a.d_result = self.result.data_ptr()
        a.stream = stream_ptr().value
        check(self.lib.exg_bcf_to_vcf(C.byref(a)))
        r = abi.BcfToVcfResult()
        check(self.lib.exg_bcf_result(C.c_void_p(self.result.data_ptr()), stream_ptr(), C.byref(r)))
        return r

    def run(self, d_input, n_bytes=None, flags=abi.EXG_F_EOF, output_capacity=None, guard=0xA5):
        """launch() with the output buffer filled with `guard` first, so that a test sees what was not written -> (result, buffer)"""
        self.out.fill_(guard)
        r = self.launch(d_input, n_bytes, flags, output_capacity)
        return r, self.out.cpu().numpy().tobytes()


def read_bcf_file_records(path, columns=None, where=None, filters=None):
    """the rows of a BCF file through the table function (the VCF schema of the file's own header): a convenience for scripts
    and tests.  columns / where / filters are Relation.fetchall's."""
    from . import table_function
    return table_function.connect().table_function("read_bcf_file_records", path).fetchall(columns=columns, where=where, filters=filters)


def tabix_query(index_bytes, region):
    """exg_tabix_query (host only): the inflated bytes of a .tbi and a region -> ([(virtual begin, virtual end)], resolved region as
    (ref_id, name, start, end)), by the two-call capacity protocol"""
    lib = load_library()
    enc = region.encode() if isinstance(region, str) else region
    n = C.c_uint64(0)
    resolved = abi.Region()
    check(lib.exg_tabix_query(index_bytes, len(index_bytes), enc, None, 0, C.byref(n), C.byref(resolved)))
    chunks = (abi.VirtualChunk * max(1, n.value))()
    check(lib.exg_tabix_query(index_bytes, len(index_bytes), enc, chunks, n.value, C.byref(n), C.byref(resolved)))
    return ([(int(chunks[i].begin), int(chunks[i].end)) for i in range(n.value)],
            (int(resolved.ref_id), resolved.name[:resolved.name_len], int(resolved.start), int(resolved.end)))


def vcf_region_keep(scan, n_rows, d_input, payload_base, name, start, end=abi.REGION_UNBOUNDED, guard=-1):
    """exg_vcf_region_keep on the columns a VcfScan left in HBM -> the keep words (uint64 numpy array of (n_rows + 63) // 64 words;
    the buffer behind them is filled with `guard` first and one word longer, so that a test sees a store out of place)"""
    torch = _torch()
    lib = load_library()
    words = (n_rows + 63) // 64
    keep = torch.full((words + 1,), guard, dtype=torch.int64, device=scan.pos.device)
    d_name = upload(name)
    a = abi.VcfRegionArgs()
    a.d_chrom, a.d_ref, a.d_info = scan.cols[0].data_ptr(), scan.cols[3].data_ptr(), scan.cols[7].data_ptr()
    a.d_pos = scan.pos.data_ptr()
    a.d_payload = d_input.data_ptr()
    a.payload_base = payload_base
    a.n_rows = n_rows
    a.d_name, a.name_len = d_name.data_ptr(), len(name)
    a.start, a.end = start, end
    a.d_keep = keep.data_ptr()
    a.stream = stream_ptr().value
    check(lib.exg_vcf_region_keep(C.byref(a)))
    torch.cuda.synchronize()
    host = keep.cpu().numpy().view(np.uint64)
    assert host[words] == np.uint64(guard & 0xFFFFFFFFFFFFFFFF), "exg_vcf_region_keep wrote behind its last word"
    return host[:words]


def vcf_query(path, region, columns=None, where=None, filters=None):
    """the rows of vcf_query(path, region) through the table function — a BGZF VCF with its tabix index beside it (path + ".tbi").
    columns / where / filters are Relation.fetchall's."""
    from . import table_function
    return table_function.connect().table_function("vcf_query", path, region=region).fetchall(columns=columns, where=where, filters=filters)


def vcf_query_reader(path, region, batch_size=abi.EXG_VECTOR_SIZE):
    """vcf_query_reader — the reference's FFI entry behind vcf_query (exon/include/rust.hpp:60-63) — as a pyarrow.RecordBatchReader"""
    import pyarrow as pa
    lib = load_library()
    stream = (C.c_uint64 * 8)()
    enc = lambda s: s if isinstance(s, bytes) else s.encode()  # noqa: E731
    err = lib.exg_vcf_query_reader(C.addressof(stream), enc(path), enc(region), batch_size)
    if err:
        msg = C.string_at(err).decode("utf-8", "replace")
        C.CDLL(None).free(C.c_void_p(err))
        raise ExgError(abi.EXG_E_INVALID_ARG, msg)
    return pa.RecordBatchReader._import_from_c(C.addressof(stream))
