"""read_sam_file_records on the device against the Python reader of tests/sam_files.py: every input through the general path
(EXG_ALGO_MULTIPASS) AND the single-pass scan (EXG_ALGO_FUSED_FULL), with and without EXG_F_NO_STORE, every comparison
exact — rows as tuples (NULL as None, strings resolved out of the input bytes), the row count, and for a failing input the
error's code, record ordinal and byte offset with the rows in front of it intact.  Then the same records through
exg_bam_scan, the reader (batches, a long header, decoders, shards, fan-out, projection, COUNT(*), the memory cap) and the
pushed-down filters on all ten columns.

Scan inputs are 100-200 KiB: at least three super-tiles of 32 KiB and a ragged tail."""
import bz2
import gzip
import json
import os

import pytest

import bam_files as BAM
import sam_files as S
import test_filters_gpu as TF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXPECTED = json.load(open(os.path.join(GOLDEN, "sam", "expected_sam.json")))
HALF, SUPER, WIN = 16384, 32768, 1024    # the single-pass scan's staging unit, its super-tile (two halves), the window in front of a half
FN = "read_sam_file_records"
LINE = b"q1\t99\tchr1\t100\t60\t10M\t=\t300\t210\tACGTACGTAC\tIIIIIIIIII"


def as_row(values):
    return tuple(v.encode() if isinstance(v, str) else v for v in values)


def launch(data, algo, flags=None, capacity=None, project=None):
    from exon_duckdb_amd import abi, device
    d_in = device.upload(data)
    scan = device.SamScan(len(data), capacity_records=capacity)
    scan.launch(d_in, flags=(abi.EXG_F_BOF | abi.EXG_F_EOF) if flags is None else flags, algo=algo, project=project)
    return scan, scan.fetch()


def check(data, want_error=None):
    """alignment lines (no header) through both drivers, stored and EXG_F_NO_STORE, against the oracle; -> the oracle's (rows, error)"""
    from exon_duckdb_amd import abi
    rows, err = S.read(data)
    if want_error is not None:
        assert err is not None and err[:2] == want_error, (err, want_error)
    for algo in (abi.EXG_ALGO_MULTIPASS, abi.EXG_ALGO_FUSED_FULL):
        scan, res = launch(data, algo)
        assert not res.flags & (abi.EXG_RF_CAPACITY | abi.EXG_RF_HEAD_UNRESOLVED | abi.EXG_RF_INDEX_OVERFLOW), (algo, res.flags)
        assert bool(res.flags & abi.EXG_RF_NON_ASCII) == any(b >= 0x80 for b in data), algo
        assert res.n_records == len(rows), (algo, res.n_records, len(rows), res.error_code, res.error_record)
        if err is None:
            assert res.error_code == 0 and res.consumed_bytes == len(data), (algo, res.error_code, res.error_record, res.error_offset)
        else:
            assert (res.error_record, res.error_code, res.error_offset) == err, (algo, res.error_record, res.error_code, res.error_offset, err)
        got = scan.rows(len(rows), data)
        if got != rows:
            k = next(i for i, (g, w) in enumerate(zip(got, rows)) if g != w)
            raise AssertionError((algo, k, got[k], rows[k]))
        _, res2 = launch(data, algo, flags=abi.EXG_F_BOF | abi.EXG_F_EOF | abi.EXG_F_NO_STORE, capacity=0)
        assert (res2.n_records, res2.error_code) == (res.n_records, res.error_code), algo
        if err is not None:
            assert (res2.error_record, res2.error_offset) == err[::2], algo
    return rows, err


def reader_rows(path, **kw):
    from exon_duckdb_amd.reader import ShardReader
    r = ShardReader(str(path), "sam", **kw)
    try:
        return r.rows()
    finally:
        r.close()


# ---------------------------------------------------------------- inputs (built once, never changed)
def mix_bytes():
    """every shape of the writer, 45-470-byte lines, a CRLF on every 97th line, no final newline, 515 rows (8 * 64 + 3)"""
    data = S.mixed(S.rng(11), 515, crlf_every=97, final_newline=False)
    lens = [len(ln) for _, ln in S.lines_of(data)]
    assert 100 << 10 <= len(data) <= 140 << 10 and min(lens) < 70 and max(lens) > 350 and len(lens) % 64 == 3, (len(data), min(lens), max(lens))
    return data


def place(rng, data, at, ln, anchor):
    """data + filler lines + ln, with byte `anchor` of ln at offset `at` of the result"""
    data = S.fill_to(rng, data, at - anchor - 900)
    gap = at - anchor - len(data)
    probe = S.line(S.rng(99), read_len=36, name=b"F", aux=False) + b"\n"
    assert len(probe) < 200 < gap, (gap, len(probe))
    filler = S.line(S.rng(99), read_len=36, name=b"F" * (1 + gap - len(probe)), aux=False) + b"\n"
    assert len(filler) == gap
    data += filler + ln
    assert data[at - anchor:at - anchor + len(ln)] == ln
    return data


def seam_bytes():
    """lines whose first byte, whose SEQ-ending tab and whose QUAL-ending byte (a tab in front of aux fields, else the line feed)
    are the first byte of a half / a super-tile and the last byte of the one in front: twelve placements at twelve seams"""
    rng = S.rng(12)
    data, marks = b"", []
    for i, (part, delta) in enumerate((p, d) for p in ("head", "seq_tab", "qual_end") for d in (0, -1)):
        for seam in ((4 * i + 1) * HALF, (2 * i + 1) * SUPER):                    # a half seam inside a super-tile, then a super-tile seam
            f = S.line(rng, read_len=150, aux=seam % SUPER != 0).split(b"\t")
            f[0], f[10] = b"seam_%d" % len(marks), b"J" * 150
            ln = b"\t".join(f) + b"\n"
            seq_tab = len(b"\t".join(f[:10]))
            anchor = {"head": 0, "seq_tab": seq_tab, "qual_end": seq_tab + 151}[part]
            assert ln[anchor:anchor + 1] == (b"s" if part == "head" else b"\t" if part == "seq_tab" or len(f) > 11 else b"\n")
            data = place(rng, data, seam + delta, ln, anchor)
            marks.append((seam + delta, part))
    return S.fill_to(rng, data, len(data) + 3000)[:-1], marks


def far_bytes():
    """lines for k_line_far: a 5 kB read that begins in front of a half's window and ends inside the half, a 5 kB name the same way,
    a 40 kB read over two whole halves and a super-tile seam — all with aux fields behind QUAL or without"""
    rng = S.rng(13)
    data = S.fill_to(rng, b"", 3 * HALF - 2600)
    a0 = len(data)
    data += S.line(rng, read_len=2500, aux=True) + b"\n"
    assert a0 < 3 * HALF - WIN - 900 and 3 * HALF < len(data) < 4 * HALF
    data = S.fill_to(rng, data, 5 * HALF - 1500)
    b0 = len(data)
    data += S.line(rng, read_len=100, name=b"N" * 5000) + b"\r\n"
    assert b0 < 5 * HALF - WIN and 5 * HALF < len(data) < 6 * HALF
    data = S.fill_to(rng, data, 7 * HALF - 3100)
    c0 = len(data)
    data += S.line(rng, read_len=20000, aux=False) + b"\n"
    assert c0 < 7 * HALF and len(data) > 9 * HALF and c0 // SUPER != len(data) // SUPER
    data = S.fill_to(rng, data, 190 << 10)
    return data[:-1]                      # (a ragged tail: no final newline)


@pytest.fixture(scope="module")
def mix():
    return mix_bytes()


@pytest.fixture(scope="module")
def far():
    return far_bytes()


# ---------------------------------------------------------------- 1. the golden files
def test_golden_files(gpu):
    from exon_duckdb_amd import table_function
    pinned = [as_row(r) for r in EXPECTED["example1.sam"]["rows"]]
    assert pinned == [(b"ref1_grp1_p001", 99, b"ref1", 1, 10, b"0", b"10M", b"ref1", b"CGAGCTCGGT", b"!!!!!!!!!!")]
    con = table_function.connect()
    for f in EXPECTED["example1.sam"]["files"]:
        path = os.path.join(GOLDEN, f)
        kw = {"compression": "bzip2"} if f.endswith(".bz2") else {}
        assert reader_rows(path, **kw) == pinned, f
        rel = con.table_function(FN, path, **kw)
        assert rel.names == S.NAMES and rel.fetchall() == pinned and rel.count() == 1, f
        assert list(rel.types) == [4 if c in S.INT_COLS else 1 for c in range(10)]      # INTEGER / VARCHAR
    for name in ("example1.sam", "little.sam", "comment1.sam"):
        raw = open(os.path.join(GOLDEN, "sam", name), "rb").read()
        want = [as_row(r) for r in EXPECTED[name]["rows"]]
        assert check(raw[S.header_end(raw):])[0] == want and reader_rows(os.path.join(GOLDEN, "sam", name)) == want, name
    path = os.path.join(GOLDEN, "sam", "comment1.sam")
    assert con.table_function(FN, path).fetchall(columns=["sequence", "name"]) == [(r[8], r[0]) for r in want]


# ---------------------------------------------------------------- 2. - 5. shapes
def test_mix_crlf_and_unterminated_tail(gpu, mix):
    rows, err = check(mix)
    assert err is None and len(rows) == 515
    assert {r[2] is None for r in rows} == {True, False} and {r[8] == b"" for r in rows} == {True, False}


def test_densest_lines_fill_a_half(gpu):
    """the shortest valid line — eleven one-byte fields, 22 bytes with its LF — 1 600 times: 744 lines a half, then ordinary lines"""
    data = S.fill_to(S.rng(14), b"q\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*\n" * 1600, 110 << 10)[:-1]
    rows, err = check(data)
    assert err is None and rows[:1600] == [(b"q", 0, None, None, None, b"0", b"", None, b"", b"")] * 1600 and len(rows) % 64 != 0


def test_line_heads_seq_tabs_and_qual_ends_on_the_seams(gpu):
    data, marks = seam_bytes()
    assert len(marks) == 12 and len({m[0] // HALF for m in marks}) == 12 and len(data) > 11 * SUPER + 2000
    rows, err = check(data)
    assert err is None and sum(r[0].startswith(b"seam_") for r in rows) == 12


def test_far_lines_and_a_read_over_two_halves(gpu, far):
    rows, err = check(far)
    assert err is None
    assert sorted(len(r[8]) for r in rows)[-2:] == [2500, 20000] and max(len(r[0]) for r in rows) == 5000
    assert max(len(r[9]) for r in rows) == 20000


def probe_lines():
    f = LINE.split(b"\t")

    def ln(seq, qual, aux=()):
        return b"\t".join(f[:9] + [seq, qual] + list(aux))
    aux = [b"NM:i:0", b"XX:Z:" + b"x" * 80]
    return [ln(b"ACGTACGTAC", b"*"), ln(b"ACGTACGTAC", b"*", aux), ln(b"*", b"IIIIIIIIII"), ln(b"*", b"IIIIIIIIII", aux), ln(b"*", b"I"), ln(b"*", b"I", aux),
            ln(b"*", b"II", aux), ln(b"*", b"*"), ln(b"*", b"*", aux), ln(b"A", b"*"), ln(b"A", b"*", aux), ln(b"A", b"I"), ln(b"A", b"I", aux),
            ln(b"ACGTACGTAC", b"IIIIIIIIII"), ln(b"ACGTACGTAC", b"IIIIIIIIII", aux), ln(b"*", b"J" * 300, aux), ln(b"G" * 300, b"*", aux),
            ln(b"G" * 300, b"J" * 300, [b"", b""]), ln(b"*", b"**"), ln(b"**", b"II")] + star_lines()


STAR_AUX = [b"NM:i:0", b"MD:Z:10", b"RG:Z:g1"]        # behind QUAL `*`: tabs 1, 8 and 16 bytes behind QUAL's first byte, the line's end 24


def star_lines():
    """QUAL `*` with SEQ present, SEQ's length equal to the offset (from QUAL's first byte) of each aux tab and of the line's
    end, with one, two and three aux fields and with none — where a probe by SEQ's length lands on a tab or on the end"""
    f = LINE.split(b"\t")
    out = []
    for n_aux in (0, 1, 2, 3):
        ends = [1]
        for a in STAR_AUX[:n_aux]:
            ends.append(ends[-1] + 1 + len(a))
        for L in ends:
            out.append(b"\t".join(f[:9] + [(b"ACGT" * 6)[:L], b"*"] + STAR_AUX[:n_aux]))
    assert [len(x.split(b"\t")[9]) for x in out] == [1, 1, 8, 1, 8, 16, 1, 8, 16, 24]
    return out


def test_the_qual_probe(gpu):
    """QUAL `*` with SEQ present, SEQ `*` with QUAL present (of one byte, of SEQ's length, of another), both `*`; nothing or aux
    fields behind QUAL"""
    rng = S.rng(15)
    data = S.fill_to(rng, b"", 40 << 10) + b"".join(ln + b"\n" for ln in probe_lines()) + S.fill_to(rng, b"", 70 << 10)
    k = len(S.lines_of(S.fill_to(S.rng(15), b"", 40 << 10)))
    rows, err = check(data)
    assert err is None
    got = [r[8:] for r in rows[k:k + 20]]
    assert got[:4] == [(b"ACGTACGTAC", b"")] * 2 + [(b"", b"IIIIIIIIII")] * 2 and got[7:11] == [(b"", b"")] * 2 + [(b"A", b"")] * 2
    assert got[15:] == [(b"", b"J" * 300), (b"G" * 300, b""), (b"G" * 300, b"J" * 300), (b"", b"**"), (b"**", b"II")]
    assert [r[8:] for r in rows[k + 20:k + 30]] == [((b"ACGT" * 6)[:L], b"") for L in (1, 1, 8, 1, 8, 16, 1, 8, 16, 24)]
    # a miss of the probe that is no `*`: the lengths differ
    f = LINE.split(b"\t")
    for qual in (b"IIIIIIIII", b"IIIIIIIIIII", b"I", b"**"):
        for aux in ((), (b"NM:i:0",)):
            bad = b"\t".join(f[:10] + [qual] + list(aux))
            check(S.mixed(S.rng(16), 20) + bad + b"\n" + S.mixed(S.rng(17), 5), want_error=(20, S.E_LENGTHS))


# ---------------------------------------------------------------- 6. integer edges
def with_field(k, value):
    f = LINE.split(b"\t")
    f[k] = value
    return b"\t".join(f)


BIG = b"268435455M" * 8                                                        # a span of 2^31 - 8
EDGE_ROWS = [with_field(1, b"65535"), with_field(1, b"0000000000000000000000007"), with_field(3, b"0"), with_field(3, b"2147483647"),
             with_field(4, b"000"), with_field(4, b"007"), with_field(4, b"255"), with_field(4, b"0255"), with_field(5, b"268435455M"),
             with_field(5, BIG).replace(b"\t100\t", b"\t8\t"), with_field(5, BIG).replace(b"\t100\t", b"\t9\t"), with_field(5, b"268435455N" * 40),
             with_field(5, b"*").replace(b"\t100\t", b"\t1\t"), with_field(5, b"3S4M1I2D1N1=1X5H6P")]
EDGE_ERRORS = [(with_field(1, b"65536"), S.E_FLAG), (with_field(1, b"+1"), S.E_FLAG), (with_field(1, b"-1"), S.E_FLAG), (with_field(1, b"9" * 30), S.E_FLAG),
               (with_field(3, b"2147483648"), S.E_POSITION), (with_field(3, b"+1"), S.E_POSITION), (with_field(3, b"4294967297"), S.E_POSITION),
               (with_field(3, b"1 "), S.E_POSITION), (with_field(4, b"256"), S.E_MAPQ), (with_field(4, b"+1"), S.E_MAPQ), (with_field(4, b"6O"), S.E_MAPQ),
               (with_field(5, b"268435456M"), S.E_CIGAR), (with_field(5, b"4294967306M"), S.E_CIGAR), (with_field(5, b"+1M"), S.E_CIGAR),
               (with_field(5, b"10"), S.E_CIGAR), (with_field(5, b"M"), S.E_CIGAR), (with_field(5, b"10M*"), S.E_CIGAR), (with_field(5, b"10B"), S.E_CIGAR)]


def test_integer_edges_as_rows(gpu):
    rng = S.rng(18)
    data = S.fill_to(rng, b"", 50 << 10) + b"".join(ln + b"\n" for ln in EDGE_ROWS) + S.fill_to(rng, b"", 60 << 10)
    k = len(S.lines_of(S.fill_to(S.rng(18), b"", 50 << 10)))
    rows, err = check(data)
    assert err is None
    e = rows[k:k + len(EDGE_ROWS)]
    assert [e[0][1], e[1][1]] == [65535, 7] and e[2][3:5] == (None, None) and e[3][3:5] == (2147483647, None)
    assert [r[5] for r in e[4:8]] == [b"0", b"7", None, None] and e[8][4] == 100 + 268435455 - 1
    assert e[9][3:5] == (8, 2147483647) and e[10][3:5] == (9, None) and e[11][4] is None and e[12][3:5] == (1, None) and e[13][4] == 108


@pytest.mark.parametrize("case", range(len(EDGE_ERRORS)))
def test_integer_edges_as_errors(gpu, case):
    bad, code = EDGE_ERRORS[case]
    front = S.mixed(S.rng(19), 70)
    rows, err = check(front + bad + b"\n" + S.mixed(S.rng(20), 30), want_error=(70, code))
    assert len(rows) == 70 and err[2] == len(front)


# ---------------------------------------------------------------- 7. errors
BAD_LINES = {S.E_FIELD_COUNT: b"\t".join(LINE.split(b"\t")[:10]), S.E_EMPTY_FIELD: with_field(6, b""), S.E_HEADER_LINE: with_field(0, b"@q1"),
             S.E_FLAG: with_field(1, b"x"), S.E_POSITION: with_field(3, b"1e3"), S.E_MAPQ: with_field(4, b"-"), S.E_CIGAR: with_field(5, b"10Q"),
             S.E_LENGTHS: with_field(10, b"IIII")}


@pytest.fixture(scope="module")
def base_lines():
    data = S.mixed(S.rng(21), 520)
    assert len(data) > 3 * SUPER + 5000
    return [ln for _, ln in S.lines_of(data)]


def with_lines(base_lines, repl, final_newline=True):
    lines = list(base_lines)
    for k, ln in repl.items():
        lines[k] = ln
    data = b"\n".join(lines) + b"\n"
    return data if final_newline else data[:-1]


def line_in_second_super_tile(base_lines):
    off = 0
    for k, ln in enumerate(base_lines):
        if off > SUPER + 100:
            return k
        off += len(ln) + 1


@pytest.mark.parametrize("code", sorted(BAD_LINES))
def test_each_error_on_the_first_a_middle_and_the_last_line(gpu, base_lines, code):
    mid, last = line_in_second_super_tile(base_lines), len(base_lines) - 1
    for k in (0, mid, last):
        rows, _ = check(with_lines(base_lines, {k: BAD_LINES[code]}, final_newline=k != last), want_error=(k, code))
        assert len(rows) == k


def test_empty_fields_empty_lines_and_late_header_lines(gpu, base_lines):
    mid = line_in_second_super_tile(base_lines)
    for k in range(11):
        check(with_lines(base_lines, {mid: with_field(k, b"")}), want_error=(mid, S.E_EMPTY_FIELD))
    check(with_lines(base_lines, {mid: LINE[:-len(b"IIIIIIIIII")]}), want_error=(mid, S.E_EMPTY_FIELD))        # "...SEQ\t" at the line's end
    for bad in (b"", b"\r", b"@CO\tlate", b"@SQ\tSN:x\tLN:1"):
        check(with_lines(base_lines, {mid: bad}), want_error=(mid, S.E_FIELD_COUNT))


def test_the_earlier_of_two_bad_lines_wins_and_the_leftmost_field(gpu, base_lines):
    mid = line_in_second_super_tile(base_lines)
    later = mid + 250                                                      # two super-tiles further on
    assert sum(len(ln) + 1 for ln in base_lines[mid:later]) > SUPER and later < len(base_lines)
    check(with_lines(base_lines, {mid: BAD_LINES[S.E_CIGAR], later: BAD_LINES[S.E_FIELD_COUNT]}), want_error=(mid, S.E_CIGAR))
    check(with_lines(base_lines, {mid: BAD_LINES[S.E_FIELD_COUNT], later: BAD_LINES[S.E_POSITION], 5: BAD_LINES[S.E_MAPQ]}), want_error=(5, S.E_MAPQ))
    # within a line: the field count first, then the leftmost field
    check(with_lines(base_lines, {mid: b"\t".join([b"", b"x", b"", b"y"])}), want_error=(mid, S.E_FIELD_COUNT))
    check(with_lines(base_lines, {mid: with_field(1, b"x").replace(b"\t100\t", b"\ty\t")}), want_error=(mid, S.E_FLAG))
    check(with_lines(base_lines, {mid: with_field(4, b"999").replace(b"\t10M\t", b"\t10Q\t")}), want_error=(mid, S.E_MAPQ))
    check(with_lines(base_lines, {mid: with_field(5, b"1Q").replace(b"IIIIIIIIII", b"II")}), want_error=(mid, S.E_CIGAR))
    check(with_lines(base_lines, {mid: with_field(0, b"@q").replace(b"\t99\t", b"\t-\t")}), want_error=(mid, S.E_HEADER_LINE))


def test_utf8_is_validated_behind_the_fields(gpu, base_lines):
    mid = line_in_second_super_tile(base_lines)
    rows, err = check(with_lines(base_lines, {mid: with_field(0, b"n\xc3\xa9m"), mid + 3: LINE + b"\tCO:Z:caf\xc3\xa9"}))
    assert err is None and rows[mid][0] == b"n\xc3\xa9m"
    check(with_lines(base_lines, {mid: with_field(0, b"n\xc3\xa9m"), mid + 3: LINE + b"\tCO:Z:caf\xe9"}), want_error=(mid + 3, S.E_INVALID_UTF8))
    check(with_lines(base_lines, {mid: with_field(3, b"x").replace(b"q1", b"q\xff")}), want_error=(mid, S.E_POSITION))      # the field's error comes first
    # a line that begins in front of its half's window: validated by the kernel behind the scan
    long_bad = with_field(9, b"A" * 3000).replace(b"IIIIIIIIII", b"J" * 1500 + b"\xe9" + b"J" * 1499)
    check(with_lines(base_lines, {mid: long_bad}), want_error=(mid, S.E_INVALID_UTF8))


# ---------------------------------------------------------------- 8. capacity, projection, selectors
def test_capacity_one_short_and_null_column_pointers(gpu, mix):
    from exon_duckdb_amd import ExgError, abi
    rows, _ = S.read(mix)
    for algo in (abi.EXG_ALGO_MULTIPASS, abi.EXG_ALGO_FUSED_FULL):
        scan, res = launch(mix, algo, capacity=len(rows) - 1)
        assert res.flags & abi.EXG_RF_CAPACITY and res.n_records == len(rows) - 1 and res.error_code == 0, algo
        assert scan.rows(len(rows) - 1, mix) == rows[:-1], algo
        scan, res = launch(mix, algo, capacity=len(rows))
        assert not res.flags & abi.EXG_RF_CAPACITY and res.n_records == len(rows), algo
        for keep in ([0, 1, 3], [4, 7], [2, 5, 9]):
            scan, res = launch(mix, algo, project=keep)
            assert res.n_records == len(rows) and res.error_code == 0, algo
            assert scan.rows(len(rows), mix, columns=keep) == [tuple(r[c] for c in keep) for r in rows], (algo, keep)
        # a column that is not produced is still validated
        cut = mix.rfind(b"\n", 0, 40000) + 1
        bad = mix[:cut] + with_field(5, b"10Q") + b"\n" + mix[cut:]
        want = S.read(bad)[1]
        _, res = launch(bad, algo, project=[1])
        assert want[1] == S.E_CIGAR and (res.error_record, res.error_code, res.error_offset) == want, algo
    with pytest.raises(ExgError):
        launch(mix, abi.EXG_ALGO_FUSED_INDEX)


def test_auto_and_fused_are_the_single_pass_scan(gpu, far):
    from exon_duckdb_amd import abi
    rows, _ = S.read(far)
    for algo in (abi.EXG_ALGO_AUTO, abi.EXG_ALGO_FUSED):
        scan, res = launch(far, algo)
        assert res.n_records == len(rows) and res.error_code == 0 and not res.flags & (abi.EXG_RF_FALLBACK | abi.EXG_RF_REDO)
        assert scan.rows(len(rows), far) == rows


def test_mate_reference_equals_points_at_rname(gpu):
    """`=` gives a string_t on RNAME's own bytes: with a reference name of more than 12 bytes both columns hold the same pointer"""
    from exon_duckdb_amd import abi
    lines = [with_field(2, b"chrUn_KI270742v1"), with_field(2, b"chrUn_KI270742v1").replace(b"\t=\t", b"\tchrUn_KI270742v1\t"),
             with_field(2, b"*"), with_field(2, b"chr1")]
    data = S.mixed(S.rng(22), 40) + b"".join(ln + b"\n" for ln in lines)
    for algo in (abi.EXG_ALGO_MULTIPASS, abi.EXG_ALGO_FUSED_FULL):
        scan, res = launch(data, algo)
        assert res.n_records == 44 and res.error_code == 0
        cols, _ = scan.host(44)
        assert cols[2][40].tobytes() == cols[7][40].tobytes() and cols[2][40, :4].tobytes() == (16).to_bytes(4, "little")
        assert cols[2][41].tobytes() != cols[7][41].tobytes()                                   # its own bytes
        rows = scan.rows(44, data)
        assert [r[7] for r in rows[40:]] == [b"chrUn_KI270742v1", b"chrUn_KI270742v1", None, b"chr1"]


# ---------------------------------------------------------------- 9. the same records through exg_bam_scan
def test_cross_format_on_the_device(gpu):
    from exon_duckdb_amd import abi, device
    import test_sam_host as H
    recs = H.cross_format_records()
    stream = b"".join(BAM.record(**r) for r in recs)
    scan = device.BamScan(len(stream), S.REFS)
    scan.launch(device.upload(stream), flags=abi.EXG_F_EOF)
    res = scan.fetch()
    assert res.error_code == 0 and res.n_records == len(recs)
    bam_rows = scan.rows(res.n_records, res.side_bytes)
    text = b"".join(S.from_bam_fields(S.REFS, **r) + b"\n" for r in recs)
    for algo in (abi.EXG_ALGO_MULTIPASS, abi.EXG_ALGO_FUSED_FULL):
        sam, sres = launch(text, algo)
        assert sres.error_code == 0 and sres.n_records == len(recs)
        assert sam.rows(len(recs), text) == bam_rows, algo


# ---------------------------------------------------------------- 10. the reader
@pytest.fixture(scope="module")
def files(gpu, mix, far, tmp_path_factory):
    d = tmp_path_factory.mktemp("sam_reader")
    out = {}
    for name, data in (("mix", mix), ("far", far)):
        p = d / (name + ".sam")
        p.write_bytes(S.header() + data)
        out[name] = (str(p), S.header() + data, S.read(data)[0])
    return d, out


def test_reader_default_and_4096_byte_batches(files, monkeypatch):
    from exon_duckdb_amd import table_function
    from exon_duckdb_amd.reader import ShardReader
    _, f = files
    for name, (path, _, rows) in f.items():
        monkeypatch.delenv("EXG_DEVICE_BATCH_BYTES", raising=False)
        assert reader_rows(path) == rows, name
        assert table_function.connect().table_function(FN, path).fetchall() == rows, name
        monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", "4096")
        r = ShardReader(path, "sam")
        assert r.rows() == rows, name
        st = r.stats()
        r.close()
        assert st["device_batches"] >= 10 and st["scan_algo"] == 3, (name, st)       # EXG_ALGO_FUSED_FULL throughout
        r = ShardReader(path, "SAM")                                                  # (any case)
        assert r.count() == len(rows) and r.stats()["host_vector_bytes"] == 0, name
        r.close()


def test_reader_header_longer_than_a_batch_header_only_and_empty(files, tmp_path, monkeypatch):
    _, f = files
    _, _, rows = f["mix"]
    body = f["mix"][1][len(S.header()):]
    long_header = S.header(extra=[b"@CO\t%d %s\r\n" % (i, b"c" * 90) for i in range(120)])
    assert len(long_header) > 12000
    monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", "4096")
    cases = {"long.sam": (long_header + body, rows), "only.sam": (long_header, []), "empty.sam": (b"", []), "none.sam": (body, rows),
             "open.sam": (b"@HD\tVN:1.6", [])}
    for name, (data, want) in cases.items():
        p = tmp_path / name
        p.write_bytes(data)
        assert reader_rows(p) == want, name
    (tmp_path / "long.sam.gz").write_bytes(gzip.compress(long_header + body, 6, mtime=0))
    (tmp_path / "only.sam.gz").write_bytes(gzip.compress(long_header, 6, mtime=0))
    assert reader_rows(tmp_path / "long.sam.gz") == rows and reader_rows(tmp_path / "only.sam.gz") == []


def test_reader_errors_name_the_byte_and_keep_the_rows_in_front(files, base_lines, tmp_path):
    from exon_duckdb_amd import ExgError
    from exon_duckdb_amd.reader import ShardReader
    mid = line_in_second_super_tile(base_lines)
    data = S.header() + with_lines(base_lines, {mid: BAD_LINES[S.E_MAPQ]})
    rows, err = S.read_file(data)
    assert len(rows) == mid and err[1] == S.E_MAPQ
    p = tmp_path / "bad.sam"
    p.write_bytes(data)
    r = ShardReader(str(p), "sam")
    with pytest.raises(ExgError) as e:
        r.rows()
    r.close()
    assert f"at byte {err[2]} of" in str(e.value) and "mapping quality" in str(e.value)      # (a byte of the file: the header counts)
    with pytest.raises(ExgError):
        ShardReader(str(p), "sam").count()


def test_reader_decoders(files, monkeypatch):
    from exon_duckdb_amd import table_function
    from exon_duckdb_amd.testing import bgzf
    from zstd_util import compress
    d, f = files
    path, data, rows = f["mix"]
    bgzf.bgzip(path, str(d / "mix.bgz.sam.gz"))
    (d / "mix.one.sam.gz").write_bytes(gzip.compress(data, 6, mtime=0))
    (d / "mix.sam.bz2").write_bytes(bz2.compress(data))
    (d / "mix.sam.zst").write_bytes(compress(data, 3, True))
    for batch in (None, "4096"):
        if batch:
            monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", batch)
        assert reader_rows(d / "mix.bgz.sam.gz") == rows
        assert reader_rows(d / "mix.one.sam.gz") == rows
        assert reader_rows(d / "mix.sam.bz2", compression="bzip2") == rows
        assert reader_rows(d / "mix.sam.zst") == rows
    con = table_function.connect()
    assert con.table_function(FN, str(d / "mix.bgz.sam.gz")).fetchall(columns=["name", "start"]) == [(r[0], r[3]) for r in rows]
    assert con.table_function(FN, str(d / "mix.sam.bz2"), compression="bzip2").count() == len(rows)


@pytest.mark.parametrize("name", ["mix", "far"])
def test_reader_shards_and_fan_out(files, monkeypatch, name):
    from exon_duckdb_amd.reader import ShardReader
    from exon_duckdb_amd.testing import bgzf
    d, f = files
    path, data, rows = f[name]
    monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", str(16 << 10))
    monkeypatch.setenv("EXG_SHARD_HALO", "512")                 # (the halo grows until it holds the line across the cut)
    for n in (2, 3, 7):
        got, counts = [], 0
        for i in range(n):
            got += reader_rows(path, shard_index=i, shard_count=n)      # (a shard that is not the first never sees the header)
            r = ShardReader(path, "sam", shard_index=i, shard_count=n)
            counts += r.count()
            r.close()
        assert got == rows and counts == len(rows), (name, n)
    monkeypatch.setenv("EXON_GPU_SHARDS", "5")
    monkeypatch.setenv("EXG_FANOUT_WORKERS", "3")
    assert reader_rows(path, shard_count=0) == rows, name
    r = ShardReader(path, "sam", shard_count=0)
    assert r.count() == len(rows)
    r.close()
    if name == "mix":
        gz = str(d / "shards.sam.gz")
        bgzf.bgzip(path, gz)
        assert sum((reader_rows(gz, shard_index=i, shard_count=3) for i in range(3)), []) == rows
        assert reader_rows(gz, shard_count=0) == rows


def test_reader_projection_and_count_bytes(files):
    from exon_duckdb_amd.reader import ShardReader
    _, f = files
    path, _, rows = f["mix"]
    r = ShardReader(path, "sam", columns=[3])
    assert r.rows() == [(x[3],) for x in rows]
    r.close()
    r = ShardReader(path, "sam", columns=[1])
    assert r.rows() == [(x[1],) for x in rows] and r.stats()["host_vector_bytes"] == 4 * len(rows)
    r.close()
    r = ShardReader(path, "sam", columns=[0, 9, 4])
    assert r.rows() == [(x[0], x[4], x[9]) for x in rows]
    r.close()
    r = ShardReader(path, "sam")
    assert r.count() == len(rows) and r.stats()["host_vector_bytes"] == 0
    r.close()


def test_reader_memory_cap(gpu, tmp_path, monkeypatch):
    """a file of 64 MiB built by repeating one block, under EXG_DEVICE_MEM_CAP_MB=16: the digest of the uncapped read, and the
    peak under the cap"""
    from exon_duckdb_amd.reader import ShardReader
    cap_mb = 16
    block = S.mixed(S.rng(23), 3000)
    times = (64 << 20) // len(block) + 1
    path = tmp_path / "big.sam"
    with open(path, "wb") as f:
        f.write(S.header())
        for _ in range(times):
            f.write(block)
    n_rows = 3000 * times
    cols = [0, 1, 3, 5, 8]
    monkeypatch.delenv("EXG_DEVICE_MEM_CAP_MB", raising=False)
    r = ShardReader(str(path), "sam", columns=cols)
    free = r.digest(per_column=True)
    r.close()
    monkeypatch.setenv("EXG_DEVICE_MEM_CAP_MB", str(cap_mb))
    r = ShardReader(str(path), "sam", columns=cols)
    capped = r.digest(per_column=True)
    st = r.stats()
    r.close()
    print(f"cap {cap_mb} MiB: peak {st['device_bytes_peak'] / 1048576:.2f} MiB, {st['device_batches']} batches of {st['device_batch_bytes']} bytes")
    assert os.path.getsize(path) >= 64 << 20 and free == capped and capped[0] == n_rows
    assert st["device_bytes_peak"] <= cap_mb << 20 and st["device_batches"] >= 8, st
    r = ShardReader(str(path), "sam")
    assert r.count() == n_rows
    r.close()


# ---------------------------------------------------------------- 11. filters: the records of the BAM filter tests, as text
def filter_bytes():
    recs = [dict(name=TF.BAM_NAMES[r % 5] + (b"" if r % 3 else b"/%d" % r), flag=TF.BAM_FLAGS[r % 5], ref=TF.BAM_REF_IDS[r % 9], pos=TF.BAM_POS[r % 7],
                 mapq=TF.BAM_MAPQ[r % 6], cigar=TF.BAM_CIGARS[r % 4], next_ref=TF.BAM_MATE_IDS[r % 7], seq=TF.BAM_SEQS[r % 8], qual=TF.bam_qual(r))
            for r in range(TF.N_ROWS)]
    return S.header(TF.BAM_REFS) + b"".join(S.from_bam_fields(TF.BAM_REFS, **r) + b"\n" for r in recs)


@pytest.fixture(scope="module")
def sam_site(gpu, tmp_path_factory):
    data = filter_bytes()
    rows, err = S.read_file(data)
    want = BAM.parse_decoded(TF.bam_raw())
    assert err is None and len(rows) == TF.N_ROWS and rows == want.rows           # the BAM filter tests' rows, value for value
    p = tmp_path_factory.mktemp("filters_sam") / "edge.sam"
    p.write_bytes(data)
    return TF.Site(p, "sam", FN, S.NAMES, list(S.NAMES), TF.BAM_SCHEMA, [dict(zip(S.NAMES, r)) for r in rows], TF.BAM_LITERALS)


@pytest.fixture(params=["default", "small"])
def batch(request, monkeypatch):
    if request.param == "small":
        monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", "4096")
    else:
        monkeypatch.delenv("EXG_DEVICE_BATCH_BYTES", raising=False)
    return request.param


@pytest.mark.parametrize("col", S.NAMES)
def test_filters_every_leaf(sam_site, batch, col):
    TF.check_leaves(sam_site, col, sam_site.shard_rows)


def test_filters_random_trees(sam_site, batch):
    TF.check_trees(sam_site, TF.trees_for(sam_site, 80, 4), sam_site.shard_rows)
