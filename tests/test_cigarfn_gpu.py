"""exg_cigar_op on the GPU: parse_cigar and extract_from_cigar on duckdb::string_t columns in HBM against tests/cigar_ref.py (a
regular expression and a left-to-right loop).  Every case compares element for element — the list entries, the one-letter
string_t of every operation byte for byte, the lengths, the slices as raw string_t — and checks that nothing behind n_rows /
total_ops was written: the outputs are sentinel-filled buffers of exactly the size asked for.

The kernels cut the rows longer than 12 bytes into tiles of 4 KiB of "tile space" (the concatenation of those rows), not the
16 KiB of the sequence scalars: the long-row cases below place their boundaries by TILE = 4096."""
import ctypes as C
import struct

import numpy as np
import pytest

import cigar_ref as ref
import seqfn_ref

pytestmark = pytest.mark.gpu

BASE, SEQ_BASE = 1 << 40, 1 << 41
SENTINEL = 0xA5
TILE = 4096
PARSE, EXTRACT = 1, 2


def upload_column(rows, base, **kw):
    import torch
    from exon_duckdb_amd import device
    col, payload = seqfn_ref.build_column(rows, payload_base=base, **kw)
    return (torch.from_numpy(col).cuda() if len(rows) else None), device.upload(payload.tobytes())


def long_bytes(rows):
    return sum(len(s) for s in rows if s is not None and len(s) > 12)


class Launch:
    """one exg_cigar_op call on buffers of the test's own: sentinel-filled outputs of exactly the capacity asked for"""

    def __init__(self, op, cigar, n, cap=0, sequence=(None, None), payload_bytes=0, children=True):
        import torch
        from exon_duckdb_amd import abi, device, load_library
        lib = load_library()
        self.op, self.n, self.cap = op, n, cap
        full = lambda shape, dt: torch.full(shape, SENTINEL, dtype=dt, device="cuda")      # noqa: E731
        self.entries = full((n + 4, 16), torch.uint8)
        self.out_op = full((cap + 4, 16), torch.uint8)
        self.out_len = full((cap + 4, 4), torch.uint8)
        self.start, self.end = full((n + 4, 4), torch.uint8), full((n + 4, 4), torch.uint8)
        self.slices = full((n + 4, 16), torch.uint8)
        ws_bytes = int(lib.exg_cigar_workspace_bytes(op, n, payload_bytes))
        self.ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device="cuda")
        self.d_result = torch.full((8,), -1, dtype=torch.int64, device="cuda")
        a = self.args = abi.CigarOpArgs()
        a.op, a.n_rows = op, n
        a.d_cigar = cigar[0].data_ptr() if cigar[0] is not None else None
        a.d_cigar_payload, a.cigar_payload_base = cigar[1].data_ptr(), BASE
        if op == PARSE:
            a.ops_capacity = cap
            if children:
                a.d_out_entries, a.d_out_op, a.d_out_len = self.entries.data_ptr(), self.out_op.data_ptr(), self.out_len.data_ptr()
        else:
            a.d_sequence = sequence[0].data_ptr() if sequence[0] is not None else None
            a.d_sequence_payload, a.sequence_payload_base = sequence[1].data_ptr(), SEQ_BASE
            a.d_out_start, a.d_out_end, a.d_out_sequence = self.start.data_ptr(), self.end.data_ptr(), self.slices.data_ptr()
        a.d_workspace, a.workspace_bytes = self.ws.data_ptr(), ws_bytes
        a.d_result = self.d_result.data_ptr()
        a.stream = device.stream_ptr().value
        self.keep = (cigar, sequence)
        self.rc = lib.exg_cigar_op(C.byref(a))
        self.message = lib.exg_last_error_message() if self.rc else b""
        self.result = abi.CigarResult()
        if self.rc == 0:
            self.result_rc = lib.exg_cigar_result(C.c_void_p(self.d_result.data_ptr()), device.stream_ptr(), C.byref(self.result))
            self.message = lib.exg_last_error_message() if self.result_rc else b""

    def parse_host(self):
        return self.entries.cpu().numpy(), self.out_op.cpu().numpy(), self.out_len.cpu().numpy()

    def extract_host(self):
        return self.start.cpu().numpy(), self.end.cpu().numpy(), self.slices.cpu().numpy()


def check_error(run, rows, err, total):
    from exon_duckdb_amd import abi
    r = run.result
    assert run.rc == 0, run.message
    assert r.n_rows == len(rows) and r.total_ops == total and bytes(r.pad) == bytes(23)
    if err is None:
        assert run.result_rc == 0, run.message
        assert (r.error_code, r.error_row, r.error_offset, r.error_byte) == (0, 0, 0, 0)
        return False
    row, e = err
    s = rows[row] or b""
    assert run.result_rc == abi.EXG_E_PARSE
    assert (r.error_code, r.error_row, r.error_offset) == (e.code, row, e.offset), (r.error_code, r.error_row, r.error_offset, row, e.code, e.offset)
    assert r.error_byte == (s[e.offset] if e.code == ref.PE_INVALID and e.offset < len(s) else 0)
    assert run.message == ref.error_message(row, e), run.message
    return True


def check_parse(rows, run, cap, children=True):
    """everything a parse_cigar call owes for `rows`, on success, on an error or with too small a capacity"""
    from exon_duckdb_amd import abi
    cigars = [s or b"" for s in rows]
    total = sum(ref.letters(s) for s in cigars)
    failed = check_error(run, rows, ref.first_error(cigars), total)
    assert run.result.flags == (abi.EXG_RF_CAPACITY if total > cap else 0)
    entries, out_op, out_len = run.parse_host()
    n = len(rows)
    assert (entries[n if children else 0:] == SENTINEL).all(), "entries written behind n_rows"
    if total > cap:
        assert (out_op == SENTINEL).all() and (out_len == SENTINEL).all(), "a child was written although the capacity is too small"
    assert (out_op[min(total, cap):] == SENTINEL).all() and (out_len[min(total, cap):] == SENTINEL).all(), "written behind total_ops"
    if failed or not children:
        return
    ops = [ref.parse(s) for s in cigars]
    counts = np.array([len(o) for o in ops], np.uint64)
    want_entries = np.zeros((n, 2), np.uint64)
    want_entries[:, 1] = counts
    want_entries[:, 0] = np.cumsum(counts) - counts
    got_entries = entries[:n].copy().view(np.uint64).reshape(n, 2)
    bad = np.flatnonzero((got_entries != want_entries).any(axis=1))
    assert len(bad) == 0, (bad[:8], got_entries[bad[0]], want_entries[bad[0]])
    if total > cap:
        return
    flat = [x for o in ops for x in o]
    want_op = np.zeros((total, 16), np.uint8)
    want_op[:, 0] = 1
    want_op[:, 4] = np.frombuffer("".join(o for o, _ in flat).encode(), np.uint8) if total else 0
    want_len = np.array([v for _, v in flat], np.int32)
    bad = np.flatnonzero((out_op[:total] != want_op).any(axis=1))
    assert len(bad) == 0, (bad[:8], out_op[bad[0]], want_op[bad[0]])
    got_len = out_len[:total].copy().view(np.int32).reshape(total)
    bad = np.flatnonzero(got_len != want_len)
    assert len(bad) == 0, (bad[:8], got_len[bad[:8]], want_len[bad[:8]])


def run_parse(rows, cap=None, children=True, **kw):
    cigar = upload_column(rows, BASE, **kw)
    total = sum(ref.letters(s or b"") for s in rows)
    cap = total if cap is None else cap
    run = Launch(PARSE, cigar, len(rows), cap, payload_bytes=long_bytes(rows), children=children)
    check_parse(rows, run, cap, children)
    return run


def check_extract(seqs, rows, run, seq_col):
    cigars, sequences = [s or b"" for s in rows], [s or b"" for s in seqs]
    failed = check_error(run, rows, ref.first_error(cigars, sequences), 0)
    assert run.result.flags == 0
    start, end, slices = run.extract_host()
    n = len(rows)
    assert (start[n:] == SENTINEL).all() and (end[n:] == SENTINEL).all() and (slices[n:] == SENTINEL).all(), "written behind n_rows"
    if failed:
        return
    got_start, got_end = start[:n].copy().view(np.int32).reshape(n), end[:n].copy().view(np.int32).reshape(n)
    want = bytearray(16 * n)
    for r in range(n):
        a, b, s = ref.extract(sequences[r], cigars[r])
        assert (got_start[r], got_end[r]) == (a, b), (r, got_start[r], got_end[r], a, b)
        if len(s) <= 12:
            struct.pack_into("<I12s", want, 16 * r, len(s), s)            # inlined and zero padded
        else:                                                             # the input's pointer + start, the slice's own prefix
            ptr, = struct.unpack_from("<Q", seq_col[r].tobytes(), 8)
            struct.pack_into("<I4sQ", want, 16 * r, len(s), s[:4], ptr + a)
    want = np.frombuffer(bytes(want), np.uint8).reshape(n, 16)
    bad = np.flatnonzero((slices[:n] != want).any(axis=1))
    assert len(bad) == 0, (bad[:8], slices[bad[0]], want[bad[0]])


def run_extract(seqs, rows, **kw):
    cigar = upload_column(rows, BASE, **kw)
    sequence = upload_column(seqs, SEQ_BASE, alignments=list(range(16)))
    run = Launch(EXTRACT, cigar, len(rows), sequence=sequence, payload_bytes=long_bytes(rows))
    check_extract(seqs, rows, run, sequence[0].cpu().numpy() if len(rows) else None)
    return run


def cigar_of(rng, n_ops, lo=1, hi=400):
    return b"".join(b"%d%c" % (int(rng.integers(lo, hi)), ref.OPS[int(rng.integers(0, 9))]) for _ in range(n_ops))


def mixed_rows(rng, n):
    """the shapes of a cigar column side by side: NULL, empty, `*`, one operation, exactly 12 bytes (inlined), exactly 13 (out of
    line), short-read shapes and a few dozen operations"""
    shapes = [lambda: None, lambda: b"", lambda: b"*", lambda: b"150M", lambda: b"75M2I73M", lambda: b"100M20I30M2D",
              lambda: b"100M20I30M12D", lambda: cigar_of(rng, int(rng.integers(1, 5))), lambda: cigar_of(rng, int(rng.integers(5, 40))),
              lambda: b"0" * int(rng.integers(0, 30)) + b"7S", lambda: b"1M2I3D4N5S6H7P8=9X"]
    rows = [shapes[int(rng.integers(0, len(shapes)))]() for _ in range(n)]
    for k, s in enumerate((b"100M20I30M2D", b"100M20I30M12D")[:n]):
        rows[k] = s
        assert len(s) == 12 + k
    return rows


def sequences_for(rng, rows, short=False):
    """a sequence per row that the row's leading and trailing insertions fit into; a third of them inlined"""
    out = []
    for s in rows:
        ops = ref.parse(s or b"")
        need = (ops[0][1] if ops and ops[0][0] == "I" else 0) + (ops[-1][1] if ops and ops[-1][0] == "I" else 0)
        extra = int(rng.integers(0, 13)) if short or rng.integers(0, 3) == 0 else int(rng.integers(13, 200))
        out.append(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, need + extra)].tobytes() if need + extra or rng.integers(0, 2) else None)
    return out


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5000])
def test_row_counts_and_shapes(gpu, n):
    """every row shape in one column, the out-of-line rows at every payload alignment 0..15 with digits in front of each (a
    walker that left its row would read them)"""
    rng = np.random.default_rng(n)
    rows = mixed_rows(rng, n)
    run_parse(rows, alignments=list(range(16)), slack=b"9")
    run_extract(sequences_for(rng, rows), rows, alignments=list(range(16)), slack=b"9")


def boundary_row(prefix, n_ops=10000):
    """`prefix` and then 123M 456I 789D ... of four bytes each: every tile boundary of a row that starts tile space falls at
    the same place of an operation, (TILE - len(prefix)) % 4 bytes into it"""
    return prefix + b"".join(b"%d%c" % (100 + k % 900, ref.OPS[k % 9]) for k in range(n_ops))


@pytest.mark.parametrize("prefix", [b"1M", b"12M", b"123M", b"1234M"], ids=["in_run_2", "in_run_1", "at_run_start", "run_then_letter"])
def test_a_row_over_many_tiles(gpu, prefix):
    """one row of about 40 KB (10 000 operations, ten tiles).  The boundary falls inside a digit run (two digits before it, or
    one), in front of a run, and — `1234M` — between a run and its letter: the letter is the first byte of a tile and walks its
    whole run in the tile before"""
    row = boundary_row(prefix)
    assert len(row) > 9 * TILE and (TILE - len(prefix)) % 4 == {2: 2, 3: 1, 4: 0, 5: 3}[len(prefix)]
    run_parse([row])
    run_parse([b"5M", row, b"150M"], alignments=[7])
    seq = b"ACGT" * 5
    run_extract([seq, seq, seq], [b"3I5M", b"2I" + row + b"4I", b"*"], alignments=[3])       # a long CIGAR, a short sequence
    run_extract([b"ACGTACGTACGTACGTA"], [b"2I" + row + b"2I"])                               # a slice of 13 bytes


def test_a_long_row_between_inlined_rows(gpu):
    """a row of about 70 KB between two runs of a thousand inlined rows: its operations sit between theirs"""
    rng = np.random.default_rng(70)
    short = [cigar_of(rng, int(rng.integers(1, 4)), hi=99)[:12] for _ in range(2000)]
    short = [s if ref.error_offset(s) is None else b"150M" for s in short]
    long_row = cigar_of(rng, 20000)
    assert all(len(s) <= 12 for s in short) and len(long_row) > 68000
    rows = short[:1000] + [long_row] + short[1000:]
    run_parse(rows)
    run_extract(sequences_for(rng, rows, short=True), rows)


def test_a_run_of_twenty_thousand_zeros(gpu):
    """leading zeros do not count: 20 000 of them, then 1M — one walker (the M), one linear walk over five tiles; again with
    the run ending the row (an error at the row's length) and with a value above the bound behind the zeros"""
    zeros = b"0" * 20000
    run_parse([b"3S", zeros + b"1M" + b"22I" * 700, b"4H"])
    run_extract([b"ACGTACGT"], [zeros + b"2I5M00000001I"])
    run_parse([b"3S", b"5M" + zeros, b"4H"])
    run_parse([b"3S", b"5M" + zeros + b"268435456M" + b"3I" * 2000, b"4H"])
    run_parse([b"3S", b"5M" + zeros + b"268435455M" + b"3I" * 2000, b"4H"])


def pad_long(s, front=True):
    """`s` made a long row by valid operations in front of it (or behind it)"""
    return b"10M2I30M2D40M" + s if front else s + b"10M2I30M2D40M"


ERRORS = [b"5M?3I", b"5M*", b"5m", b"5M 3I", b"5M\x003I", b"5M\xff",          # a byte that is neither
          b"MMM", b"5MM", b"5M=",                                             # a letter without digits
          b"12", b"5M12",                                                     # digits up to the end
          b"268435456M", b"5M999999999I", b"0000268435456M", b"99999999999999999999999M", b"5M268435456",      # above the bound
          b"5?7?", b"5M300000000I?"]                                          # the leftmost wins


@pytest.mark.parametrize("bad", ERRORS, ids=lambda s: repr(s[:20]))
def test_every_error_kind_with_its_offset(gpu, bad):
    """inlined, out of line, and deep in a row of several tiles; both ops"""
    good = [b"150M", b"*", b"75M2I73M10S2H", None]
    deep = boundary_row(b"12M", 3000) + bad
    for s in (bad, pad_long(bad), deep):
        assert ref.error_offset(s) is not None
        rows = good + [s] + good
        run_parse(rows, alignments=[5, 11])
        run_extract([b"ACGT"] * len(rows), rows, alignments=[5, 11])
    if ref.error_offset(pad_long(bad, front=False)) is not None:
        run_parse(good + [pad_long(bad, front=False)], alignments=[9])


def test_which_error_wins(gpu):
    long_ok = boundary_row(b"12M", 5000)
    assert len(long_ok) > 4 * TILE
    # a bad byte in the last tile of a long row 0 against a bad short row 1: row 0 wins
    run = run_parse([long_ok + b"?", b"MMM"])
    assert (run.result.error_row, run.result.error_offset) == (0, len(long_ok))
    # two bad bytes in one row, tiles apart: the leftmost wins
    two = long_ok[:5000] + b"?" + long_ok[5001:] + b"?"
    run = run_parse([b"150M", two])
    assert (run.result.error_row, run.result.error_offset) == (1, 5000)
    # a bad long row behind a bad short row: the short row wins
    run = run_parse([b"150M", b"5MM", two])
    assert (run.result.error_row, run.result.error_offset) == (1, 2)
    # extract_from_cigar: a syntax error comes before the range error, in the row and between rows
    run_extract([b"ACGT"], [b"9I1M9I5"])
    run_extract([b"ACGT"], [b"9I" + long_ok + b"9I5"])
    run = run_extract([b"ACGT", b"ACGT"], [b"9I", b"MMM"])
    assert (run.result.error_row, run.result.error_code) == (0, ref.PE_RANGE)
    run = run_extract([b"ACGT", b"ACGT"], [b"MMM", b"9I"])
    assert (run.result.error_row, run.result.error_code) == (0, ref.PE_INVALID)


@pytest.mark.parametrize("shift", [0, 1, 2, 5, 9, 10])
def test_an_error_whose_run_straddles_a_tile_boundary(gpu, shift):
    """ten digits above the bound, `shift` of them in front of the first tile boundary: the offset is the ninth digit's,
    whichever tile holds it"""
    prefix = next(p for p in (b"12M", b"123M", b"1234M", b"12345M") if (TILE - shift - len(p)) % 4 == 0)
    head = boundary_row(prefix, (TILE - shift - len(prefix)) // 4)
    assert len(head) == TILE - shift and ref.error_offset(head) is None
    row = head + b"3000000000M" + b"5I" * 100
    assert ref.error_offset(row) == len(head) + 8
    run_parse([row])
    run_parse([b"4M", row], alignments=[13])
    run_extract([b"ACGT"], [row])
    run_parse([head + b"0000000000" + b"77M" + b"5I" * 100])               # the same run, valid: ten zeros astride


def test_capacity_and_the_counting_call(gpu):
    from exon_duckdb_amd import abi
    rng = np.random.default_rng(11)
    rows = mixed_rows(rng, 300) + [cigar_of(rng, 3000)]
    total = sum(ref.letters(s or b"") for s in rows)
    run = run_parse(rows, cap=0, children=False)                            # the counting call: NULL children
    assert run.result.total_ops == total and run.result.flags == abi.EXG_RF_CAPACITY
    run = run_parse(rows, cap=total - 1)                                    # one short: the sentinels stay
    assert run.result.total_ops == total and run.result.flags == abi.EXG_RF_CAPACITY
    run = run_parse(rows, cap=total)
    assert run.result.total_ops == total and run.result.flags == 0
    run = run_parse([None, b"", b"*"], cap=0, children=False)               # nothing to write is no capacity error
    assert run.result.total_ops == 0 and run.result.flags == 0
    run = run_parse(rows[:100] + [b"5MM"], cap=0, children=False)           # the counting call validates all the same
    assert run.result.error_row == 100


def test_extract_from_cigar(gpu):
    seq = b"AACCAAC"
    pins = ([b"AACCAA", seq], [b"2I2M2I", b"2I2M2I1M"])                     # test_scalar_functions.test:105-116
    run_extract(*pins)
    long_seq = bytes(b"ACGT"[k % 4] for k in range(40))
    cases = [(long_seq, b"40M"), (long_seq, b"5I35M"), (long_seq, b"35M5I"), (long_seq, b"5I30M5I"),       # neither, first, last, both
             (long_seq, b"20I"), (long_seq, b""), (long_seq, b"*"), (None, b"*"), (b"", b"3M"), (None, None),
             (long_seq[:24], b"6I12M6I"), (long_seq[:25], b"6I13M6I"),                                   # slices of 12 and of 13 bytes
             (long_seq[:12], b"12M"), (long_seq[:13], b"13M"), (long_seq[:13], b"1I12M"), (long_seq[:14], b"1I13M"),
             (b"ACGTACGTACGT", b"2I8M2I"), (b"ACG", b"1I1M1I"), (b"AC", b"1I"),                           # inlined sequences
             (long_seq, b"0000000000005I30M000005I")]
    run_extract([s for s, _ in cases], [c for _, c in cases])
    for bad in ((long_seq, b"41I"), (long_seq, b"21I"), (long_seq, b"21I1M20I"), (b"", b"1I"), (b"ACGT", b"3I2I")):             # start > end
        run = run_extract([long_seq, bad[0]], [b"40M", bad[1]])
        assert (run.result.error_code, run.result.error_row) == (ref.PE_RANGE, 1)


def string_rows(col, n):
    return col[:n].cpu().numpy().view(np.uint8).reshape(n, 16)


def test_on_the_columns_of_a_sam_and_a_bam_scan(gpu):
    """the cigar and sequence columns of exg_sam_scan and of exg_bam_scan, fed to both ops without leaving the device: every
    operation letter, unmapped reads (the scans hand `*` over as the empty string)"""
    import sam_files as S
    import bam_files as BAM
    import test_sam_host as H
    from exon_duckdb_amd import abi, device
    text = S.mixed(S.rng(31), 48)
    d_text = device.upload(text)
    sam = device.SamScan(len(text))
    sam.launch(d_text)
    res = sam.fetch()
    assert res.error_code == 0 and res.n_records == 48
    recs = H.cross_format_records()
    stream = b"".join(BAM.record(**r) for r in recs)
    d_stream = device.upload(stream)
    bam = device.BamScan(len(stream), S.REFS)
    bam.launch(d_stream, flags=abi.EXG_F_EOF)
    bres = bam.fetch()
    assert bres.error_code == 0 and bres.n_records == len(recs)
    for scan, n, rows, payload, base in ((sam, 48, sam.rows(48, text), d_text, sam.PAYLOAD_BASE),
                                         (bam, len(recs), bam.rows(len(recs), bres.side_bytes), bam.side, bam.SIDE_BASE)):
        cigars, seqs = [r[6] or b"" for r in rows], [r[8] or b"" for r in rows]
        assert set(b"".join(cigars)) >= set(ref.OPS) and b"" in cigars
        entries, op, length, r = device.parse_cigar(scan.cols[6], n, payload, base)
        want = [ref.parse(s) for s in cigars]
        assert r.total_ops == sum(len(o) for o in want) and r.error_code == 0
        assert entries.cpu().numpy().astype(np.uint64).tolist() == [[sum(len(o) for o in want[:k]), len(want[k])] for k in range(n)]
        got_op = string_rows(op, int(r.total_ops))
        assert (got_op[:, :4].copy().view(np.uint32) == 1).all() and not got_op[:, 5:].any()
        assert list(zip(got_op[:, 4].tobytes().decode(), length.cpu().numpy().tolist())) == [x for o in want for x in o]
        start, end, slices, r = device.extract_from_cigar(scan.cols[8], payload, base, scan.cols[6], payload, base, n)
        assert r.error_code == 0
        raw, seq_raw = string_rows(slices, n), string_rows(scan.cols[8], n)
        for k in range(n):
            a, b, s = ref.extract(seqs[k], cigars[k])
            assert (int(start[k]), int(end[k])) == (a, b)
            if len(s) <= 12:
                assert raw[k].tobytes() == struct.pack("<I12s", len(s), s)
            else:
                assert raw[k].tobytes() == struct.pack("<I4sQ", len(s), s[:4], struct.unpack_from("<Q", seq_raw[k].tobytes(), 8)[0] + a)


def test_two_runs_are_byte_identical(gpu):
    rng = np.random.default_rng(3)
    rows = mixed_rows(rng, 700) + [cigar_of(rng, 6000)] + mixed_rows(rng, 300)
    seqs = sequences_for(rng, rows)
    a, b = run_parse(rows), run_parse(rows)
    for x, y in zip(a.parse_host(), b.parse_host()):
        assert np.array_equal(x, y)
    assert bytes(a.result) == bytes(b.result)
    a, b = run_extract(seqs, rows), run_extract(seqs, rows)
    for x, y in zip(a.extract_host(), b.extract_host()):
        assert np.array_equal(x, y)
    assert bytes(a.result) == bytes(b.result)


def test_host_and_device_agree(gpu):
    """a few hundred random rows, valid and broken in one byte, with a fixed seed: table_function.* and the device op give the
    same rows, and the same first error"""
    from exon_duckdb_amd import ExgError, device, table_function as tf
    rng = np.random.default_rng(17)
    rows = []
    for it in range(400):
        s = cigar_of(rng, int(rng.integers(1, 12)), lo=0, hi=1 << int(rng.integers(1, 29)))
        rows.append(s)
    seqs = sequences_for(rng, [s if ref.error_offset(s) is None else b"" for s in rows])
    broken = list(rows)
    for k in (391, 120, 333):                                               # the first error is row 120's
        s = broken[k]
        at = int(rng.integers(0, len(s)))
        broken[k] = s[:at] + b"?" + s[at + 1:]
    for cigars in (rows, broken):
        host, host_err = [], None
        for k, s in enumerate(cigars):
            try:
                host.append((tf.parse_cigar(s), tf.extract_from_cigar(seqs[k] or b"", s)))
            except ExgError as e:
                host_err = (k, e.parse_code, e.offset)
                break
        cigar, sequence = upload_column(cigars, BASE), upload_column(seqs, SEQ_BASE)
        try:
            entries, op, length, r = device.parse_cigar(cigar[0], len(cigars), cigar[1], BASE)
            start, end, slices, _ = device.extract_from_cigar(sequence[0], sequence[1], SEQ_BASE, cigar[0], cigar[1], BASE, len(cigars))
            dev_err = None
        except ExgError as e:
            dev_err = str(e)
        if host_err is None:
            assert dev_err is None and len(host) == len(cigars)
            letters, lens = string_rows(op, int(r.total_ops))[:, 4].tobytes().decode(), length.cpu().numpy().tolist()
            ent, st, en = entries.cpu().numpy().tolist(), start.cpu().numpy().tolist(), end.cpu().numpy().tolist()
            for k, (p, x) in enumerate(host):
                o, m = ent[k]
                assert [{"op": letters[j], "len": lens[j]} for j in range(o, o + m)] == p
                assert (st[k], en[k]) == (x["sequence_start"], x["sequence_end"])
        else:
            assert host_err[0] == 120 and dev_err is not None
            assert dev_err.endswith("Invalid CIGAR string in row %d at byte %d" % (host_err[0], host_err[2])), dev_err
