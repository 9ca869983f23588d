"""exg_sequence_op on the GPU: the six sequence scalars on duckdb::string_t columns in HBM against tests/seqfn_ref.py (an
independent restatement of the reference's module.cpp:30-370).  The output strings are compared after resolving pointers AND as
raw bytes against the output contract of include/exon_gpu.h: the string_t array byte for byte, the out-of-line rows packed in
row order without gaps, total_bytes, the result block and the raised text on an error."""
import ctypes as C
import os

import numpy as np
import pytest

import seqfn_ref as ref

pytestmark = pytest.mark.gpu

BASE = 1 << 40
OUT_BASE = 1 << 46
SENTINEL = 0xA5
STRING_OPS = list(ref.STRING_OPS)
ALL_OPS = list(ref.ALL_OPS)
op_ids = lambda op: ref.OP_NAMES[op]      # noqa: E731


def seq(n, op, rng):
    """n valid letters for op"""
    alphabet = np.frombuffer(b"ACGU" if op == ref.REVERSE_TRANSCRIBE else b"ACGT", np.uint8)
    return alphabet[rng.integers(0, 4, n)].tobytes()


def scale(op):
    return 3 if op == ref.TRANSLATE else 1


class Launch:
    """one exg_sequence_op call on buffers of the test's own: sentinel-filled outputs of exactly the capacity asked for"""

    def __init__(self, op, d_col, n, d_payload, payload_base, out_capacity, workspace_bytes=None):
        import torch
        from exon_duckdb_amd import abi, device, load_library
        lib = load_library()
        self.op, self.n, self.cap = op, n, out_capacity
        self.out_col = torch.full((max(n, 1), 16), SENTINEL, dtype=torch.uint8, device="cuda")
        self.out_payload = torch.full((out_capacity + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.out_float = torch.full((max(n, 1),), -7.0, dtype=torch.float32, device="cuda")
        ws_bytes = int(lib.exg_sequence_workspace_bytes(op, n)) if workspace_bytes is None else workspace_bytes
        self.ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device="cuda")
        self.d_result = torch.full((8,), -1, dtype=torch.int64, device="cuda")
        a = self.args = abi.SequenceOpArgs()
        a.op, a.n_rows = op, n
        a.d_strings = d_col.data_ptr() if d_col is not None else None
        a.d_payload = d_payload.data_ptr() if d_payload is not None else None
        a.payload_base = payload_base
        a.d_out_strings, a.d_out_payload = self.out_col.data_ptr(), self.out_payload.data_ptr()
        a.out_capacity, a.out_base = out_capacity, OUT_BASE
        a.d_out_float = self.out_float.data_ptr()
        a.d_workspace, a.workspace_bytes = self.ws.data_ptr(), ws_bytes
        a.d_result = self.d_result.data_ptr()
        a.stream = device.stream_ptr().value
        self.keep = (d_col, d_payload)
        self.rc = lib.exg_sequence_op(C.byref(a))
        self.message = lib.exg_last_error_message() if self.rc else b""
        self.result = abi.SeqResult()
        if self.rc == 0:
            self.result_rc = lib.exg_sequence_result(C.c_void_p(self.d_result.data_ptr()), device.stream_ptr(), C.byref(self.result))
            self.message = lib.exg_last_error_message() if self.result_rc else b""

    def host(self):
        return self.out_col[:self.n].cpu().numpy(), self.out_payload.cpu().numpy(), self.out_float[:self.n].cpu().numpy()


def upload_column(rows, **kw):
    import torch
    from exon_duckdb_amd import device
    col, payload = ref.build_column(rows, payload_base=BASE, **kw)
    d_col = torch.from_numpy(col).cuda() if len(rows) else None
    return d_col, device.upload(payload.tobytes())


def total_bytes(op, rows):
    if op == ref.GC_CONTENT:
        return 0
    lens = [0 if s is None else (len(s) // 3 if op == ref.TRANSLATE else len(s)) for s in rows]
    return sum(n for n in lens if n > 12)


def check_launch(op, rows, run):
    """everything exg_sequence_op owes for `rows`, on success or on an error"""
    from exon_duckdb_amd import abi
    assert run.rc == 0, run.message
    r = run.result
    assert r.total_bytes == total_bytes(op, rows) and bytes(r.pad) == bytes(20)
    err = ref.first_error(op, rows)
    if err is not None:
        row, e = err
        assert run.result_rc == abi.EXG_E_PARSE
        want_bytes = e.text[-3:] if e.code == ref.PE_CODON else e.text[-1:] if e.code == ref.PE_INVALID_CHARACTER else b""
        assert (r.error_code, r.error_row, r.error_offset, r.error_length, r.flags) == (e.code, row, e.offset, e.length, 0)
        assert bytes(r.error_bytes) == want_bytes.ljust(4, b"\0")
        assert run.message == e.text + b" in row %d" % row
        return
    assert run.result_rc == 0, run.message
    assert (r.error_code, r.error_row, r.error_offset, r.error_length, r.flags, bytes(r.error_bytes)) == (0, 0, 0, 0, 0, bytes(4))
    col, payload, floats = run.host()
    if op == ref.GC_CONTENT:
        want = np.array([np.float32(0) if s is None else ref.apply_fast(op, s) for s in rows], np.float32)
        assert np.array_equal(floats.view(np.uint32), want.view(np.uint32)), np.flatnonzero(floats.view(np.uint32) != want.view(np.uint32))[:8]
        return
    outputs = [ref.apply_fast(op, s) for s in rows]
    want_col, want_payload = ref.expected_column(outputs, OUT_BASE)
    total = int(r.total_bytes)
    assert total == len(want_payload)
    assert ref.decode_column(col, payload[:total], OUT_BASE) == [o or b"" for o in outputs]
    bad = np.flatnonzero((col != want_col).any(axis=1)) if len(rows) else []
    assert len(bad) == 0, (bad[:8], col[bad[0]], want_col[bad[0]])
    assert np.array_equal(payload[:total], want_payload)
    assert (payload[total:] == SENTINEL).all(), "bytes written behind total_bytes"


def run_rows(op, rows, out_capacity=None, **kw):
    d_col, d_payload = upload_column(rows, **kw)
    cap = total_bytes(op, rows) if out_capacity is None else out_capacity
    run = Launch(op, d_col, len(rows), d_payload, BASE, cap)
    check_launch(op, rows, run)
    return run


LADDER = [0, 1, 2, 3, 11, 12, 13, 15, 16, 17, 63, 64, 65] + [(1 << k) + d for k in range(8, 17) for d in (-1, 0, 1)]


@pytest.mark.parametrize("op", ALL_OPS, ids=op_ids)
def test_length_ladder(gpu, op):
    """every length around the inline, group, wave and tile boundaries, at every source alignment 0..15, NULL rows between;
    the bytes between the rows ('#') are invalid for every op: no row may be seen to read them"""
    rng = np.random.default_rng(op)
    rows = []
    for rep in range(16):       # 35 (translate: 37) out-of-line rows a repetition, coprime with 16: every length meets every alignment
        for k, n in enumerate(LADDER):
            rows.append(seq(n * scale(op), op, rng))
            if k % 4 == 3:
                rows.append(None)
        rows.append(seq(40 * scale(op), op, rng))
    run_rows(op, rows, alignments=list(range(16)))
    if op == ref.TRANSLATE:     # 36 -> 12 is inlined, 39 -> 13 is not
        run = run_rows(op, [seq(36, op, rng), seq(39, op, rng), seq(36, op, rng)], alignments=[5])
        assert run.result.total_bytes == 13


@pytest.mark.parametrize("op", ALL_OPS, ids=op_ids)
def test_one_long_row_among_many_short_ones(gpu, op):
    """300 rows of 150 bytes and one of 1 MiB + 3 (translate_dna_to_aa: three times that, so that it is a whole number of
    codons) first, in the middle, last"""
    rng = np.random.default_rng(10 + op)
    short = [seq(150, op, rng) for _ in range(300)]
    long_row = seq(((1 << 20) + 3) * scale(op), op, rng)
    for at in (0, 150, 300):
        run_rows(op, short[:at] + [long_row] + short[at:], lead=at % 16)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257, 100000])
@pytest.mark.parametrize("op", ALL_OPS, ids=op_ids)
def test_row_counts(gpu, op, n):
    rng = np.random.default_rng(20 + op)
    distinct = [seq(150, op, rng) for _ in range(257)]
    run_rows(op, [distinct[i % 257] for i in range(n)])


@pytest.mark.parametrize("op", ALL_OPS, ids=op_ids)
def test_all_rows_empty_and_all_rows_null(gpu, op):
    for rows in ([b""] * 1000, [None] * 1000, [None, b"", None, b"ACG", b""] * 100):
        run = run_rows(op, rows)
        assert run.result.total_bytes == 0


def test_gc_content_is_bit_exact(gpu):
    rows = []
    for n in (3, 7, 150):
        for k in range(n + 1):
            rows.append(b"G" * (k // 2) + b"A" * (n - k) + b"C" * (k - k // 2))
    rows += [b"gcgc", b"gcGC\xc7\xc3", b"g" * 150, b"\xc7\xc3" * 75 + b"G", b"GCgc" * 5000]     # lower case and bytes >= 0x80 never count
    run_rows(ref.GC_CONTENT, rows, alignments=[3, 8, 0, 15])
    # (float)size rounds: 2^24 + 1 bytes with an odd count
    n = (1 << 24) + 1
    big = np.full(n, ord("A"), np.uint8)
    big[::3] = ord("G")
    big[1::7] = ord("c")
    big[-1] = ord("C")
    count = int(np.count_nonzero((big == ord("G")) | (big == ord("C"))))
    if count % 2 == 0:
        big[1] = ord("C") if big[1] != ord("C") else ord("A")
        count = int(np.count_nonzero((big == ord("G")) | (big == ord("C"))))
    assert count % 2 == 1 and int(np.float32(n)) == n - 1
    run = run_rows(ref.GC_CONTENT, [b"ACGT" * 40, big.tobytes(), b"GG"], lead=7)
    assert run.host()[2][1].tobytes() == (np.float32(count) / np.float32(n)).tobytes()


def bad_byte(op):
    return {ref.REVERSE_TRANSCRIBE: b"T", ref.TRANSCRIBE: b"U"}.get(op, b"N")


def spoil(op, s, unit):
    """s with its unit-th byte (translate_dna_to_aa: the middle letter of its unit-th codon) made invalid"""
    at = 3 * unit + 1 if op == ref.TRANSLATE else unit
    return s[:at] + bad_byte(op) + s[at + 1:]


@pytest.mark.parametrize("op", STRING_OPS, ids=op_ids)
def test_errors(gpu, op):
    """the bad byte / codon on the first, a middle and the last row; at the first, the last and the 2^14-th byte (codon) of a
    row of 2^15 + 1; the result block and the message are exact (check_launch)"""
    rng = np.random.default_rng(30 + op)
    k = scale(op)
    short = [seq(150, op, rng) for _ in range(300)]
    long_row = seq(((1 << 15) + 1) * k, op, rng)
    units = len(long_row) // k
    for row_at in (0, 150, 300):
        for unit in (0, units - 1, 1 << 14):
            rows = short[:row_at] + [spoil(op, long_row, unit)] + short[row_at:]
            run = run_rows(op, rows, lead=unit % 16)
            assert run.result.error_row == row_at and run.result.error_offset == unit * k
    # short rows: inlined outputs and the byte-by-byte path around row ends
    for row_at, n, unit in ((0, 1, 0), (7, 12, 11), (299, 13, 12), (150, 150, 149), (151, 150, 0)):
        rows = list(short)
        rows[row_at] = spoil(op, seq(n * k, op, rng), unit)
        run = run_rows(op, rows)
        assert run.result.error_row == row_at
    # two bad rows: the lower one wins, wherever in the row its byte is
    rows = list(short)
    rows[200], rows[17], rows[18] = spoil(op, short[200], 0), spoil(op, short[17], 49), spoil(op, short[18], 0)
    assert run_rows(op, rows).result.error_row == 17
    rows = [spoil(op, long_row, units - 1), spoil(op, long_row, 0)] + short
    assert run_rows(op, rows).result.error_offset == (units - 1) * k
    # two bad bytes in one row: the leftmost
    assert run_rows(op, short + [spoil(op, spoil(op, long_row, 20000), 999)]).result.error_offset == 999 * k


def test_translate_length_errors(gpu):
    from exon_duckdb_amd import abi
    op = ref.TRANSLATE
    rng = np.random.default_rng(40)
    short = [seq(150, op, rng) for _ in range(300)]
    for row_at in (0, 150, 300):
        for n in (1, 4, 37, 40, 151, (1 << 15) + 2):
            run = run_rows(op, short[:row_at] + [seq(n, op, rng)] + short[row_at:])
            assert (run.result.error_code, run.result.error_row, run.result.error_length) == (abi.EXG_PE_SEQ_LENGTH, row_at, n)
            assert run.message == b"Invalid sequence length: %d in row %d" % (n, row_at)
    # a bad length and a bad codon in one row: the length wins; a bad codon in a lower row wins over both
    for n in (40, 152, 3 * (1 << 14) + 2):
        both = spoil(op, seq(n, op, rng), 0)
        assert run_rows(op, short + [both]).result.error_code == abi.EXG_PE_SEQ_LENGTH
        run = run_rows(op, [spoil(op, short[0], 3)] + short + [both])
        assert (run.result.error_code, run.result.error_row, run.result.error_offset) == (abi.EXG_PE_SEQ_CODON, 0, 9)
    assert run_rows(op, [b"NNNN"]).message == b"Invalid sequence length: 4 in row 0"
    assert run_rows(op, [b"ATGNNN"]).message == b"Invalid codon: NNN in row 0"


@pytest.mark.parametrize("op", ALL_OPS, ids=op_ids)
def test_a_bad_byte_in_the_slack_between_two_rows_is_not_an_error(gpu, op):
    rng = np.random.default_rng(50 + op)
    rows = [seq(n * scale(op), op, rng) for n in (13, 150, 16, 4097, 31, 150, 150, 48, 1025)]
    for slack in (b"N", b"#Q\xff", b"acgtn" * 7):
        run = run_rows(op, rows, slack=slack, lead=len(slack))
        assert run.result.error_code == 0


def test_sequence_op_raises_the_references_text(gpu):
    import torch
    from exon_duckdb_amd import ExgError, abi, device
    rows = [b"ATCG" * 40, b"ATCGQ", b"ATNN"]
    col, payload = ref.build_column(rows, payload_base=BASE)
    d_col, d_payload = torch.from_numpy(col).cuda().view(torch.int64), device.upload(payload.tobytes())
    with pytest.raises(ExgError) as e:
        device.sequence_op(abi.EXG_SEQ_COMPLEMENT, d_col, 3, d_payload, BASE)
    assert e.value.code == abi.EXG_E_PARSE and str(e.value).endswith("Invalid character in sequence: Q in row 1")
    out, out_payload, r = device.sequence_op(abi.EXG_SEQ_COMPLEMENT, d_col, 1, d_payload, BASE)
    got = ref.decode_column(out.cpu().numpy().view(np.uint8).reshape(1, 16), out_payload.cpu().numpy(), device.SEQ_OUT_BASE)
    assert got == [ref.apply(ref.COMPLEMENT, rows[0])] and r.total_bytes == 160 and device.SEQ_OUT_BASE == OUT_BASE
    floats, r = device.sequence_op(abi.EXG_SEQ_GC_CONTENT, d_col, 3, d_payload, BASE)
    assert floats.cpu().numpy().tolist() == [0.5, 0.4000000059604645, 0.0] and r.total_bytes == 0


@pytest.mark.parametrize("op", STRING_OPS, ids=op_ids)
def test_capacity(gpu, op):
    from exon_duckdb_amd import abi
    rng = np.random.default_rng(60 + op)
    rows = [seq(n * scale(op), op, rng) for n in (150, 5, 13, 20000, 0, 150, 12)] + [None]
    total = total_bytes(op, rows)
    assert total == 150 + 13 + 20000 + 150
    d_col, d_payload = upload_column(rows)
    for cap in (total - 1, 0):
        run = Launch(op, d_col, len(rows), d_payload, BASE, cap)
        assert run.rc == 0 and run.result_rc == 0
        assert (run.result.flags, run.result.total_bytes, run.result.error_code) == (abi.EXG_RF_CAPACITY, total, 0)
        col, payload, _ = run.host()
        assert (col == SENTINEL).all() and (payload == SENTINEL).all(), "an output buffer was touched"
    run = Launch(op, d_col, len(rows), d_payload, BASE, total)
    check_launch(op, rows, run)
    assert run.result.flags == 0


@pytest.fixture(scope="module")
def scanned_columns(gpu, oracle, golden_dir):
    """the sequence columns three scans leave in HBM, with the oracle's rows: (name, d_col, n, d_payload, payload_base, rows)"""
    from exon_duckdb_amd import abi, device
    out = []
    with open(os.path.join(golden_dir, "test.fastq"), "rb") as f:
        golden = f.read()
    for name, data in (("test.fastq", golden), ("synth_fastq", bytes(oracle.synth_fastq(332 * 1000)))):
        exp = oracle.fastq_parse(data, want_string_t=False)
        d_in = device.upload(data)
        scan = device.FastqScan(len(data))
        scan.launch(d_in, payload_base=BASE)
        res = scan.fetch()
        assert res.error_code == 0 and res.n_records == exp.n_rows
        out.append((name, scan.cols[2], exp.n_rows, d_in, BASE, exp.columns["sequence"].to_list(), scan))
    data = bytes(oracle.synth_fasta(620))
    exp = oracle.fasta_parse(data)
    d_in = device.upload(data)
    scan = device.FastaScan(len(data))
    scan.launch(d_in, payload_base=BASE, seq_payload_base=BASE << 1)
    res = scan.fetch()
    assert res.error_code == 0 and res.n_records == exp.n_rows == 620
    out.append(("synth_fasta", scan.cols[2], exp.n_rows, scan.payload, BASE << 1, exp.columns["sequence"].to_list(), scan))
    return out


@pytest.mark.parametrize("op", [ref.COMPLEMENT, ref.TRANSCRIBE, ref.GC_CONTENT, ref.TRANSLATE], ids=op_ids)
def test_behind_the_scans(scanned_columns, op):
    """the op straight on the column a scan wrote (FASTQ: pointers into the input; FASTA: into d_seq_payload), against
    seqfn_ref over the oracle's rows — whatever they hold: reads with an N must report it"""
    for name, d_col, n, d_payload, base, rows, _ in scanned_columns:
        run = Launch(op, d_col, n, d_payload, base, max(total_bytes(op, rows), 16))
        check_launch(op, rows, run)


def test_translate_behind_the_fastq_scan_reports_the_codon_with_an_n(gpu):
    from exon_duckdb_amd import abi, device
    rng = np.random.default_rng(70)
    reads = [seq(150, ref.TRANSLATE, rng) for _ in range(500)]
    reads[321] = reads[321][:100] + b"N" + reads[321][101:]
    for spoiled in (False, True):
        rows = reads if spoiled else reads[:321]
        data = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * 150) for i, s in enumerate(rows))
        d_in = device.upload(data)
        scan = device.FastqScan(len(data))
        scan.launch(d_in, payload_base=BASE)
        assert scan.fetch().n_records == len(rows)
        run = Launch(ref.TRANSLATE, scan.cols[2], len(rows), d_in, BASE, 50 * len(rows))
        check_launch(ref.TRANSLATE, rows, run)      # 150 % 3 == 0: ACGT reads translate
        assert run.result.error_code == (abi.EXG_PE_SEQ_CODON if spoiled else 0)
        if spoiled:
            assert run.message == b"Invalid codon: " + reads[321][99:102] + b" in row 321"


@pytest.mark.parametrize("op", ALL_OPS, ids=op_ids)
def test_two_launches_are_byte_identical(gpu, op):
    rng = np.random.default_rng(80 + op)
    rows = [seq(n * scale(op), op, rng) for n in [150] * 200 + [70000, 9, 13, 0, 33000] + [150] * 100] + [None]
    d_col, d_payload = upload_column(rows, alignments=[1, 6, 11])
    a, b = (Launch(op, d_col, len(rows), d_payload, BASE, total_bytes(op, rows)) for _ in range(2))
    check_launch(op, rows, a)
    for x, y in zip(a.host(), b.host()):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert bytes(a.result) == bytes(b.result)


def test_argument_errors(gpu):
    from exon_duckdb_amd import abi
    rows = [b"ACGT" * 10, b"AC"]
    d_col, d_payload = upload_column(rows)
    ok = Launch(ref.COMPLEMENT, d_col, 2, d_payload, BASE, 64)
    assert ok.rc == 0 and ok.result_rc == 0
    for run in (Launch(ref.COMPLEMENT, None, 2, d_payload, BASE, 64),            # null d_strings
                Launch(0, d_col, 2, d_payload, BASE, 64), Launch(7, d_col, 2, d_payload, BASE, 64),      # unknown op
                Launch(ref.COMPLEMENT, d_col, 2, d_payload, BASE, 64, workspace_bytes=ok.args.workspace_bytes - 8),
                Launch(ref.GC_CONTENT, d_col, 2, d_payload, BASE, 64, workspace_bytes=ok.args.workspace_bytes)):   # short workspace
        assert run.rc == abi.EXG_E_INVALID_ARG and run.message.startswith(b"exg_sequence_op: ")
        assert (run.out_col.cpu().numpy() == SENTINEL).all() and (run.d_result.cpu().numpy() == -1).all()
