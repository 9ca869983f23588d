"""read_gtf on the device against the Python reader of tests/gtf_files.py: every scan input through the general path
(EXG_ALGO_MULTIPASS) AND the single-pass scan (EXG_ALGO_FUSED_FULL), stored and with EXG_F_NO_STORE, every comparison exact —
rows as tuples (NULL as None, strings resolved out of the input bytes, score as the float32's bits), the keep words, the line
count, and for a failing input the error's code, row and byte offset with the rows in front of it intact.  exg_gtf_attributes
against the same reader's attribute grammar: entries, keys, values, the lowest failing row with the leftmost offset and its
byte, the two-call capacity protocol.  Then the reader: the reference's fixture in four encodings, projection, pushed-down
filters beside skipped comment lines, shards cut inside quoted values, stripes, the memory cap, determinism, and a fuzz.

Scan inputs are 50-200 KiB: several super-tiles of 32 KiB and a ragged tail."""
import json
import os

import numpy as np
import pytest

import fuzz_gtf as FZ
import gtf_files as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gtf")
EXPECTED = json.load(open(os.path.join(GOLDEN, "expected_gtf.json")))
HALF, SUPER, WIN = 16384, 32768, 1024    # the single-pass scan's staging unit, its super-tile (two halves), the window in front of a half
FN = "read_gtf"
LINE = b'chr1\thavana\texon\t11869\t12227\t.\t+\t.\tgene_id "ENSG00000223972"; exon_number 1;'
BASE = 1 << 44


def with_field(k, value, line=LINE):
    f = line.split(b"\t")
    f[k] = value
    return b"\t".join(f)


def launch(data, algo, flags=None, capacity=None, project=None, dense=False):
    from exon_duckdb_amd import abi, device
    d_in = device.upload(data)
    ws = len(data) * 8 + (1 << 20) if dense else None       # the general path's line index for a line per 2 bytes
    scan = device.GtfScan(len(data), capacity_records=capacity, workspace_bytes=ws)
    scan.launch(d_in, flags=(abi.EXG_F_BOF | abi.EXG_F_EOF) if flags is None else flags, algo=algo, project=project)
    return scan, scan.fetch()


def check(data, want_error=None, dense=False):
    """lines through both drivers, stored and EXG_F_NO_STORE, against the oracle (column 8: the raw ninth field); -> (rows, keep, error)"""
    from exon_duckdb_amd import abi
    rows, keep, err = G.read(data, attributes=False)
    if want_error is not None:
        assert err is not None and err[:2] == want_error, (err, want_error)
    for algo in (abi.EXG_ALGO_MULTIPASS, abi.EXG_ALGO_FUSED_FULL):
        scan, res = launch(data, algo, dense=dense)
        assert not res.flags & (abi.EXG_RF_CAPACITY | abi.EXG_RF_HEAD_UNRESOLVED | abi.EXG_RF_INDEX_OVERFLOW), (algo, res.flags)
        assert bool(res.flags & abi.EXG_RF_NON_ASCII) == any(b >= 0x80 for b in data), algo
        assert res.n_records == len(keep), (algo, res.n_records, len(keep), res.error_code, res.error_record)      # n_records counts LINES
        if err is None:
            assert res.error_code == 0 and res.consumed_bytes == len(data), (algo, res.error_code, res.error_record, res.error_offset)
            assert bool(res.flags & abi.EXG_RF_ROWS_SKIPPED) == (not all(keep)), algo
        else:
            assert (res.error_record, res.error_code, res.error_offset) == err[:3], (algo, res.error_record, res.error_code, res.error_offset, err)
        assert scan.kept(len(keep)).tolist() == keep, algo
        got = scan.rows(len(keep), data)
        if got != rows:
            k = next((i for i, (g, w) in enumerate(zip(got, rows)) if g != w), min(len(got), len(rows)))
            raise AssertionError((algo, k, len(got), len(rows), got[k:k + 1], rows[k:k + 1]))
        _, res2 = launch(data, algo, flags=abi.EXG_F_BOF | abi.EXG_F_EOF | abi.EXG_F_NO_STORE, capacity=0, dense=dense)
        assert (res2.n_records, res2.error_code) == (res.n_records, res.error_code), algo
        assert (res2.flags & abi.EXG_RF_ROWS_SKIPPED) == (res.flags & abi.EXG_RF_ROWS_SKIPPED), algo
        if err is not None:
            assert (res2.error_record, res2.error_offset) == (err[0], err[2]), algo
    return rows, keep, err


# ---------------------------------------------------------------- inputs (built once, never changed)
@pytest.fixture(scope="module")
def mix():
    """every shape of the writer, a `#!` line every 41st line, a CRLF every 97th, no final newline, 515 lines (8 * 64 + 3)"""
    data = G.mixed(G.rng(11), 515, crlf_every=97, comment_every=41, final_newline=False)
    assert 60 << 10 <= len(data) <= 200 << 10, len(data)
    return data


@pytest.fixture(scope="module")
def base_lines():
    return [G.line(G.rng(300 + i)) for i in range(420)]


def with_lines(lines, repl, final_newline=True):
    lines = list(lines)
    for k, ln in repl.items():
        lines[k] = ln
    data = b"\n".join(lines) + b"\n"
    return data if final_newline else data[:-1]


def line_in_second_super_tile(lines):
    off = 0
    for k, ln in enumerate(lines):
        if off > SUPER + 100:
            return k
        off += len(ln) + 1


# ---------------------------------------------------------------- 1. the scan: shapes
def test_fixture_bytes_through_the_scan(gpu):
    data = open(os.path.join(GOLDEN, "test.gtf"), "rb").read()
    rows, keep, err = check(data)
    assert err is None and len(rows) == 77 and rows[0][:8] == (b"chr1", b"processed_transcript", b"exon", 11869, 12227, None, b"+", None)


def test_mixed_lines_comments_crlf_and_no_final_newline(gpu, mix):
    rows, keep, err = check(mix)
    assert err is None and keep.count(False) == 12 and len(rows) == 503
    assert {r[5] for r in rows} >= {None, 0, 0x3F000000}                                 # NULL, "0" and "0.5"
    check(mix + b"\n")


def pad_line(n):
    """a valid line of exactly n bytes with its LF (n >= 80)"""
    empty = G.line(G.rng(1), attrs=b'pad ""')
    ln = G.line(G.rng(1), attrs=b'pad "' + b"p" * (n - 1 - len(empty)) + b'"') + b"\n"
    assert len(ln) == n
    return ln


def test_lines_across_the_half_and_super_tile_seams(gpu):
    """a line whose head, whose leading fields and whose attributes lie on a half seam and on a super-tile seam"""
    rng = G.rng(12)
    data, at = b"", []
    for i, anchor in enumerate((0, 1, 30, 60, 200, 300)):
        seam = (2 * i + 1) * HALF if i % 2 else (i + 1) * SUPER
        data = G.fill_to(rng, data, seam - anchor - 700)
        data += pad_line(seam - anchor - len(data))
        assert len(data) == seam - anchor
        at.append(len(data))
        data += G.line(rng, attrs=G.attributes(rng, n_entries=8, tags=12)) + b"\n"
        assert len(data) > seam + 20
    data = G.fill_to(rng, data, len(data) + 900)
    rows, keep, err = check(data[:-1])
    assert err is None and all(keep)


def test_lines_that_begin_in_front_of_the_window_and_lines_longer_than_a_half(gpu):
    rng = G.rng(13)
    data = G.fill_to(rng, b"", 3 * HALF - 2600)
    a0 = len(data)
    data += G.line(rng, attrs=b'note "' + b"; x" * 1000 + b'"; tag "a"') + b"\n"                    # begins > 1 KiB in front of its half
    assert a0 < 3 * HALF - WIN - 900 and 3 * HALF < len(data) < 4 * HALF
    data = G.fill_to(rng, data, 5 * HALF - 1500)
    b0 = len(data)
    data += G.line(rng, seqname=b"N" * 5000) + b"\r\n"                                               # a 5 kB seqname the same way
    assert b0 < 5 * HALF - WIN and 5 * HALF < len(data) < 6 * HALF
    data = G.fill_to(rng, data, 7 * HALF - 3100)
    c0 = len(data)
    data += G.line(rng, attrs=b'seq "' + b"ACGT" * 10000 + b'"') + b"\n"                             # 40 kB: over two whole halves (k_line_far)
    assert c0 < 7 * HALF and len(data) > 9 * HALF and c0 // SUPER != len(data) // SUPER
    data += b"#" + b"c" * 20000 + b"\n"                                                              # a far line that is a comment
    data = G.fill_to(rng, data, 200 << 10)
    rows, keep, err = check(data[:-1])
    assert err is None and keep.count(False) == 1 and max(len(r[8]) for r in rows) == 40006


def test_a_half_of_hash_lines_goes_in_passes(gpu):
    """`#` + LF: 8 192 lines a half, eight times what the scan's line list holds"""
    rng = G.rng(14)
    head = G.fill_to(rng, b"", 2000)
    data = head + b"#\n" * (HALF + 3000) + G.fill_to(rng, b"", 3000)
    rows, keep, err = check(data, dense=True)
    assert err is None and keep.count(False) == HALF + 3000 and len(rows) > 10


def test_comment_lines_at_rows_63_64_65_cross_the_keep_word_seam(gpu, base_lines):
    repl = {63: b"#sixty-three", 64: b"#", 65: b"#!sixty-five", 127: b"#", 128: b"#", 0: b"#first", len(base_lines) - 1: b"#last"}
    rows, keep, err = check(with_lines(base_lines, repl))
    assert err is None and [i for i, k in enumerate(keep) if not k] == sorted(repl)
    check(with_lines(base_lines, repl, final_newline=False))


def test_a_buffer_that_is_all_comments(gpu):
    data = b"".join(b"#!directive %d with some text behind it\n" % i for i in range(1500))
    rows, keep, err = check(data)
    assert err is None and rows == [] and len(keep) == 1500 and len(data) > SUPER
    check(b"#\n")
    check(b"#")


def test_score_literals_for_the_exact_parser(gpu, base_lines):
    """more than 19 digits astride a rounding boundary: decided by the fix-up kernel behind the scan, with the bits strtof gives"""
    lits = [b"16777217.0000000000000000001", b"16777216.9999999999999999999", b"0.50000002980232238769531250000000001", b"8388609.50000000000000000001"]
    repl = {10 + 70 * i: with_field(5, lit) for i, lit in enumerate(lits)}
    rows, keep, err = check(with_lines(base_lines, repl))
    assert err is None and [rows[k][5] for k in sorted(repl)] == [G.f32_bits(lit) for lit in lits]


# ---------------------------------------------------------------- 2. the scan: every error
BAD_LINES = {
    G.E_FIELD_COUNT: LINE.rsplit(b"\t", 1)[0],
    G.E_EMPTY_FIELD: with_field(2, b""),
    G.E_POSITION: with_field(3, b"0"),
    G.E_SCORE: with_field(5, b"1e"),
    G.E_STRAND: with_field(6, b"*"),
    G.E_FRAME: with_field(7, b"3"),
    G.E_INVALID_UTF8: with_field(0, b"chr\xe9"),
}


@pytest.mark.parametrize("code", sorted(BAD_LINES))
def test_each_error_on_the_first_a_middle_and_the_last_line(gpu, base_lines, code):
    mid, last = line_in_second_super_tile(base_lines), len(base_lines) - 1
    for k in (0, mid, last):
        rows, keep, _ = check(with_lines(base_lines, {k: BAD_LINES[code], 3: b"#c"} if k else {k: BAD_LINES[code]}, final_newline=k != last), want_error=(k, code))
        assert len(keep) == k


def test_empty_lines_bad_fields_and_the_order_of_errors(gpu, base_lines):
    mid = line_in_second_super_tile(base_lines)
    later = mid + 200
    assert sum(len(ln) + 1 for ln in base_lines[mid:later]) > SUPER and later < len(base_lines)
    for bad in (b"", b"\r", b" #x", with_field(0, b""), with_field(3, b"+5"), with_field(4, b"9223372036854775808"), with_field(5, b""),
                with_field(6, b""), with_field(6, b"+-"), with_field(7, b"00")):
        check(with_lines(base_lines, {mid: bad}))
    check(with_lines(base_lines, {mid: BAD_LINES[G.E_SCORE], later: BAD_LINES[G.E_FIELD_COUNT]}), want_error=(mid, G.E_SCORE))
    check(with_lines(base_lines, {mid: BAD_LINES[G.E_FIELD_COUNT], later: BAD_LINES[G.E_POSITION], 5: BAD_LINES[G.E_FRAME]}), want_error=(5, G.E_FRAME))
    check(with_lines(base_lines, {mid: with_field(4, b"x", with_field(5, b"y"))}), want_error=(mid, G.E_POSITION))
    check(with_lines(base_lines, {mid: with_field(3, b"x", with_field(0, b"chr\xe9"))}), want_error=(mid, G.E_POSITION))
    check(with_lines(base_lines, {mid: b"#caf\xe9"}), want_error=(mid, G.E_INVALID_UTF8))
    check(with_lines(base_lines, {mid: with_field(8, b'n "' + b"J" * 3000 + b"\xe9" + b'"')}), want_error=(mid, G.E_INVALID_UTF8))     # a far line
    rows, _, err = check(with_lines(base_lines, {mid: with_field(0, b"chr\xc3\xa9")}))
    assert err is None and rows[mid][0] == b"chr\xc3\xa9"


def test_capacity_projection_and_selectors(gpu, mix):
    from exon_duckdb_amd import ExgError, abi
    rows, keep, _ = G.read(mix, attributes=False)
    n = len(keep)
    for algo in (abi.EXG_ALGO_MULTIPASS, abi.EXG_ALGO_FUSED_FULL, abi.EXG_ALGO_AUTO, abi.EXG_ALGO_FUSED):
        scan, res = launch(mix, algo, capacity=n - 1)
        assert res.flags & abi.EXG_RF_CAPACITY and res.n_records == n - 1 and res.error_code == 0, algo
        assert scan.rows(n - 1, mix) == rows[:-1], algo
        for cols in ([0, 3], [8], [5, 6, 7], [1, 2, 4]):
            scan, res = launch(mix, algo, project=cols)
            assert res.n_records == n and res.error_code == 0, algo
            assert scan.rows(n, mix, columns=cols) == [tuple(r[c] for c in cols) for r in rows], (algo, cols)
        # a column that is not produced is still validated
        cut = mix.rfind(b"\n", 0, 40000) + 1
        bad = mix[:cut] + with_field(5, b"1e") + b"\n" + mix[cut:]
        want = G.read(bad)[2]
        _, res = launch(bad, algo, project=[0])
        assert want[1] == G.E_SCORE and (res.error_record, res.error_code, res.error_offset) == want[:3], algo
    with pytest.raises(ExgError):
        launch(mix, abi.EXG_ALGO_FUSED_INDEX)


# ---------------------------------------------------------------- 3. exg_gtf_attributes
def string_column(fields, base=BASE):
    """ninth fields -> ([n, 16] uint8 string_t rows, payload bytes): up to 12 bytes inlined, longer ones at base + offset"""
    rows = np.zeros((max(len(fields), 1), 16), np.uint8)
    payload = bytearray(b"front-pad")                       # (offsets that are no multiple of anything)
    for i, f in enumerate(fields):
        rows[i, :4] = np.frombuffer(len(f).to_bytes(4, "little"), np.uint8)
        if len(f) <= 12:
            rows[i, 4:4 + len(f)] = np.frombuffer(f, np.uint8)
        else:
            rows[i, 4:8] = np.frombuffer(f[:4], np.uint8)
            rows[i, 8:16] = np.frombuffer((base + len(payload)).to_bytes(8, "little"), np.uint8)
            payload += f
    return rows, bytes(payload) + b"\0" * 16


def strings_of(t, payload, base=BASE):
    raw = t.cpu().numpy().view(np.uint8).reshape(-1, 16)
    out = []
    for r in raw:
        ln = int.from_bytes(r[:4].tobytes(), "little")
        if ln <= 12:
            assert not r[4 + ln:].any(), "inlined string_t is not zero padded"
            out.append(r[4:4 + ln].tobytes())
        else:
            o = int.from_bytes(r[8:16].tobytes(), "little") - base
            assert 0 <= o and o + ln <= len(payload) and payload[o:o + 4] == r[4:8].tobytes(), "string_t outside the payload, or a wrong prefix"
            out.append(payload[o:o + ln])
    return out


def run_attributes(fields, row_map=None, chunk_rows=0, capacity=None):
    import torch
    from exon_duckdb_amd import device
    rows, payload = string_column(fields)
    col = torch.from_numpy(rows).cuda().view(torch.int64)
    pay = device.upload(payload)
    rm = torch.tensor(row_map, dtype=torch.int32).cuda() if row_map is not None else None
    n = len(fields) if row_map is None else len(row_map)
    ent, keys, vals, bases, r = device.gtf_attributes(col, n, pay, BASE, entries_capacity=capacity, row_map=rm, chunk_rows=chunk_rows)
    return ent.cpu().numpy().astype(np.uint64), strings_of(keys, payload) if len(keys) else [], strings_of(vals, payload) if len(vals) else [], bases, r


def check_attributes(fields):
    """a column of ninth fields against the oracle's grammar: the lowest failing row, or every entry"""
    from exon_duckdb_amd import ExgError
    want, first_bad = [], None
    for i, f in enumerate(fields):
        try:
            want.append(G.parse_attributes(f))
        except G.GtfError as e:
            want.append(None)
            if first_bad is None:
                first_bad = (i, e.offset, f[e.offset] if e.offset < len(f) else 0)
    if first_bad is not None:
        with pytest.raises(ExgError) as e:
            run_attributes(fields)
        r = e.value.result
        assert (r.error_row, r.error_offset, r.error_byte, r.error_code) == first_bad + (G.E_ATTRIBUTES,), (first_bad, r.error_row, r.error_offset, r.error_byte)
        assert f"row {first_bad[0]} at byte {first_bad[1]}" in str(e.value)
    good = [i for i, w in enumerate(want) if w is not None]
    ent, keys, vals, _, r = run_attributes(fields, row_map=good if first_bad is not None else None)
    flat = [kv for i in good for kv in want[i]]
    assert r.error_code == 0 and r.total_entries == len(flat) == len(keys) and r.n_rows == len(good)
    assert list(zip(keys, vals)) == flat
    off = 0
    for j, i in enumerate(good):
        assert (int(ent[j, 0]), int(ent[j, 1])) == (off, len(want[i])), (j, i)
        off += len(want[i])
    return want


def test_attribute_fields_of_0_1_63_64_65_and_200_bytes(gpu):
    def field(n):                       # `k "vvv...";` of exactly n bytes (n >= 6), else what fits
        return b";" * n if n < 6 else b'k "' + b"v" * (n - 5) + b'";'
    fields = [field(n) for n in (0, 1, 63, 64, 65, 200, 12, 13, 127, 128, 129)]
    assert [len(f) for f in fields] == [0, 1, 63, 64, 65, 200, 12, 13, 127, 128, 129]
    want = check_attributes(fields)
    assert want[0] == want[1] == [] and want[5] == [(b"k", b"v" * 195)]
    # unquoted, with the value's last byte the field's last: the end of the field closes the entry
    check_attributes([b"k " + b"v" * n for n in (1, 61, 62, 63, 125, 126, 127)])


def test_a_quote_that_opens_in_one_word_and_closes_in_the_next(gpu):
    fields = []
    for open_at in (60, 62, 63, 64, 127):
        fields.append(b"k" * (open_at - 1) + b' "' + b"; " * 40 + b'" ; z 9')       # the quote opens at byte open_at, closes two words on
        assert fields[-1][open_at] == 0x22
    want = check_attributes(fields)
    assert all(w[0][1] == b"; " * 40 and w[1] == (b"z", b"9") for w in want)
    check_attributes([b'k "' + b"x" * n + b'"' for n in range(56, 70)])          # the closing quote at every lane around the seam


def test_semicolons_and_spaces_inside_quotes_unquoted_values_and_repeated_keys(gpu):
    fields = [b'note "5; prime end; see x"; empty ""; exon_number 1;level 2 ;', b'tag "basic"; tag "CCDS"; tag "basic";',
              b'gene_id "ENSG00000223972"; transcript_id "ENST00000456328"; exon_number "1"; gene_name "DDX11L1";', b" ;; a 1;; ;b 2; ;",
              b'k\tv w', b"k v\tw"]
    want = check_attributes(fields)
    assert want[1] == [(b"tag", b"basic"), (b"tag", b"CCDS"), (b"tag", b"basic")] and want[3] == [(b"a", b"1"), (b"b", b"2")]
    assert want[4] == [(b"k\tv", b"w")] and want[5] == [(b"k", b"v\tw")]                  # a tab is a byte like any other


def test_no_entries_more_than_64_entries_in_a_row_and_n_rows_0(gpu):
    many = b"".join(b'k%d "v%d"; ' % (i, i) for i in range(150))
    dense = b"a b;" * 500                                                        # sixteen entries a word
    want = check_attributes([b"", many, b"   ", dense, b";;;", many + b"tag x"])
    assert [len(w) for w in want] == [0, 150, 0, 500, 0, 151]
    ent, keys, vals, _, r = run_attributes([])
    assert r.total_entries == 0 and r.error_code == 0 and r.n_rows == 0 and len(ent) == 0


def test_the_two_call_capacity_protocol_and_chunk_relative_entries(gpu):
    from exon_duckdb_amd import abi
    rng = G.rng(31)
    fields = [G.attributes(rng) for _ in range(300)]
    want = [G.parse_attributes(f) for f in fields]
    total = sum(len(w) for w in want)
    ent, keys, vals, _, r = run_attributes(fields, capacity=total - 1)
    assert r.flags & abi.EXG_RF_CAPACITY and r.total_entries == total and len(keys) == 0 and r.error_code == 0
    ent, keys, vals, _, r = run_attributes(fields, capacity=total)
    assert not r.flags and list(zip(keys, vals)) == [kv for w in want for kv in w]
    ent, keys, vals, bases, r = run_attributes(fields, chunk_rows=64)
    bases = bases.cpu().numpy().tolist()
    counts = [len(w) for w in want]
    assert bases == [sum(counts[:c]) for c in range(0, 300, 64)] + [total]
    for j in range(300):
        assert (int(ent[j, 0]), int(ent[j, 1])) == (sum(counts[j // 64 * 64:j]), counts[j]), j


ATTR_ERRORS = [b"gene_id", b'a "1"; gene_id ; b 2', b"k   ", b'a "1"; note "never closed; b 2', b'a "1"x; b 2', b'a "1" x', b'a "1""2"', b'"k" v',
               b'k"e"y v', b'k v"x"', b"k v w", b"k" * 70 + b' "' + b"v" * 70, b"k" * 130, b'a 1; b "' + b";" * 200, b"a 1;" * 40 + b"k"]


@pytest.mark.parametrize("k", range(len(ATTR_ERRORS)))
def test_every_attribute_error_names_the_lowest_row_and_the_leftmost_offset(gpu, k):
    rng = G.rng(40 + k)
    fields = [G.attributes(rng) for _ in range(130)]
    fields[70] = ATTR_ERRORS[k]
    fields[100] = ATTR_ERRORS[(k + 1) % len(ATTR_ERRORS)]          # a later failing row does not win
    want = check_attributes(fields)
    assert want[70] is None and want[100] is None


# ---------------------------------------------------------------- 4. the reader
def reader_rows(path, **kw):
    from exon_duckdb_amd.reader import ShardReader
    r = ShardReader(str(path), "gtf", **kw)
    try:
        return r.rows()
    finally:
        r.close()


def user_rows(data):
    rows, _, err = G.read(data)
    assert err is None
    return [G.user_row(r) for r in rows]


@pytest.mark.parametrize("name,compression", [("test.gtf", None), ("test.gtf.gz", None), ("test.gtf.zst", None), ("test.gtf.bz2", "bzip2")])
def test_fixture_in_four_encodings_through_read_gtf(gpu, name, compression):
    """test_gtf_scan.test:5-22: the first row with attributes['gene_id'][1], and count(*)"""
    from exon_duckdb_amd import table_function
    con = table_function.connect()
    rel = con.table_function(FN, os.path.join(GOLDEN, name), compression=compression)
    assert rel.names == G.NAMES and [table_function.type_sql(t) for t in rel.trees] == G.TYPES
    first = rel.fetchall(limit=1)[0]
    want = EXPECTED["first_row"]
    assert [v.decode() if isinstance(v, bytes) else v for v in first[:8]] == want[:8]
    assert [v for k, v in first[8] if k == b"gene_id"][0].decode() == want[8]
    assert rel.count() == EXPECTED["count"] == 77
    rows = rel.fetchall()
    assert rows == user_rows(open(os.path.join(GOLDEN, "test.gtf"), "rb").read())
    if compression is None and name == "test.gtf":
        assert con.from_path(os.path.join(GOLDEN, name)).count() == 77                   # the replacement scan


@pytest.fixture(scope="module")
def files(gpu, mix, tmp_path_factory):
    d = tmp_path_factory.mktemp("gtf_reader")
    rng = G.rng(21)
    big = G.mixed(rng, 2600, crlf_every=97, comment_every=37) + G.line(rng, attrs=b'seq "' + b"ACGT" * 10000 + b'"') + b"\n" + G.mixed(rng, 400, comment_every=5)
    out = {}
    for name, data in (("mix", mix), ("big", big)):
        p = d / (name + ".gtf")
        p.write_bytes(data)
        out[name] = (str(p), data, user_rows(data))
    return d, out


def test_reader_default_and_4096_byte_batches(files, monkeypatch):
    from exon_duckdb_amd import table_function
    from exon_duckdb_amd.reader import ShardReader
    _, f = files
    for name, (path, data, rows) in f.items():
        monkeypatch.delenv("EXG_DEVICE_BATCH_BYTES", raising=False)
        assert reader_rows(path) == rows, name
        assert table_function.connect().table_function(FN, path).fetchall() == rows, name
        monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", "4096")
        r = ShardReader(path, "gtf")
        assert r.rows() == rows, name
        st = r.stats()
        r.close()
        assert st["device_batches"] >= 10 and st["scan_algo"] == 3, (name, st)       # EXG_ALGO_FUSED_FULL throughout
        r = ShardReader(path, "GTF")
        assert r.count() == len(rows) and r.stats()["host_vector_bytes"] == 0, name
        r.close()


def test_reader_all_comment_batches_empty_and_header_only_files(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", "4096")
    comments = b"".join(b"#!directive %d with some text behind it\n" % i for i in range(400))       # four batches without a row
    body = G.mixed(G.rng(22), 60)
    for name, data in (("lead.gtf", comments + body), ("only.gtf", comments), ("empty.gtf", b""), ("tail.gtf", body + comments)):
        p = tmp_path / name
        p.write_bytes(data)
        assert reader_rows(p) == user_rows(data), name
        from exon_duckdb_amd.reader import ShardReader
        r = ShardReader(str(p), "gtf")
        assert r.count() == len(user_rows(data)), name
        r.close()


def test_reader_errors_scan_and_attributes(gpu, base_lines, tmp_path):
    from exon_duckdb_amd import ExgError
    from exon_duckdb_amd.reader import ShardReader
    mid = line_in_second_super_tile(base_lines)
    data = with_lines(base_lines, {mid: BAD_LINES[G.E_FRAME], 2: b"#c"})
    _, keep, err = G.read(data)
    p = tmp_path / "bad.gtf"
    p.write_bytes(data)
    r = ShardReader(str(p), "gtf")
    with pytest.raises(ExgError) as e:
        r.rows()
    r.close()
    assert f"at byte {err[2]} of" in str(e.value) and "frame" in str(e.value)
    with pytest.raises(ExgError):
        ShardReader(str(p), "gtf").count()
    # a malformed ninth field is the attributes kernel's to find: an error when the column is selected, not otherwise
    data = with_lines(base_lines, {mid: with_field(8, b'gene_id "g"; lonely')})
    p = tmp_path / "bad_attr.gtf"
    p.write_bytes(data)
    with pytest.raises(ExgError) as e:
        reader_rows(p)
    assert "invalid GTF attributes at byte 19 " in str(e.value)
    assert len(reader_rows(p, columns=[0, 3])) == len(base_lines)


def test_reader_decoders(files, monkeypatch):
    import bz2
    import gzip
    from exon_duckdb_amd import table_function
    from exon_duckdb_amd.testing import bgzf
    from zstd_util import compress
    d, f = files
    path, data, rows = f["mix"]
    bgzf.bgzip(path, str(d / "mix.bgz.gtf.gz"))
    (d / "mix.one.gtf.gz").write_bytes(gzip.compress(data, 6, mtime=0))
    (d / "mix.gtf.bz2").write_bytes(bz2.compress(data))
    (d / "mix.gtf.zst").write_bytes(compress(data, 3, True))
    for batch in (None, "4096"):
        if batch:
            monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", batch)
        assert reader_rows(d / "mix.bgz.gtf.gz") == rows
        assert reader_rows(d / "mix.one.gtf.gz") == rows
        assert reader_rows(d / "mix.gtf.bz2", compression="bzip2") == rows
        assert reader_rows(d / "mix.gtf.zst") == rows
    con = table_function.connect()
    assert con.table_function(FN, str(d / "mix.bgz.gtf.gz")).fetchall(columns=["seqname", "start"]) == [(r[0], r[3]) for r in rows]
    assert con.table_function(FN, str(d / "mix.gtf.zst")).fetchall(columns=["attributes"]) == [(r[8],) for r in rows]
    assert con.table_function(FN, str(d / "mix.gtf.bz2"), compression="bzip2").count() == len(rows)


def test_reader_projection_seqname_start_and_attributes_alone(files):
    from exon_duckdb_amd.reader import ShardReader
    _, f = files
    for name in ("mix", "big"):
        path, _, rows = f[name]
        r = ShardReader(path, "gtf", columns=[0, 3])
        assert r.rows() == [(x[0], x[3]) for x in rows]
        assert r.stats()["host_vector_bytes"] == 24 * len(rows) if name == "mix" else True
        r.close()
        assert reader_rows(path, columns=[8]) == [(x[8],) for x in rows]
        assert reader_rows(path, columns=[5, 6, 7]) == [x[5:8] for x in rows]
        assert reader_rows(path, columns=[4, 8, 1]) == [(x[1], x[4], x[8]) for x in rows]


def test_reader_filter_beside_skipped_comment_lines(files, monkeypatch):
    from exon_duckdb_amd import table_function
    from exon_duckdb_amd.table_function import F
    _, f = files
    path, _, rows = f["big"]
    for batch in (None, "4096"):
        if batch:
            monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", batch)
        rel = table_function.connect().table_function(FN, path)
        want = [r for r in rows if r[2] == b"exon" and r[3] > 100_000_000]
        assert 0 < len(want) < len(rows)
        got = rel.fetchall(filters={"type": F.cmp("=", b"exon"), "start": F.cmp(">", 100_000_000)})
        assert got == want
        assert rel.count(filters={"type": F.cmp("=", b"exon"), "start": F.cmp(">", 100_000_000)}) == len(want)
        want = [(r[0], r[8]) for r in rows if r[5] is not None and r[5] >= 0.5 and r[6] is None]
        assert want
        got = rel.fetchall(columns=["seqname", "attributes"], filters={"score": F.cmp(">=", 0.5), "strand": F.isnull()})
        assert got == want
    from exon_duckdb_amd import ExgError
    from exon_duckdb_amd.reader import ShardReader
    with pytest.raises(ExgError):
        ShardReader(path, "gtf", filters="attributes = 'x'")


def shard_file(n_cuts):
    """blocks of lines with a line between them whose 3 kB quoted value (`;` and spaces inside) straddles each of the cuts of
    n_cuts + 1 equal byte ranges"""
    rng = G.rng(50 + n_cuts)
    block = G.mixed(rng, 120, comment_every=11)
    long_line = b'chr1\thavana\tgene\t1\t2\t.\t+\t.\tgene_id "g"; note "' + b";  " * 1000 + b'"; tag "t";\n'
    data = (block + long_line) * n_cuts + block
    n = len(data)
    for c in range(1, n_cuts + 1):
        cut = n * c // (n_cuts + 1)
        line_start = data.rfind(b"\n", 0, cut) + 1
        assert data[line_start:line_start + len(long_line)] == long_line and 60 < cut - line_start < len(long_line) - 20, (c, cut - line_start)
    return data


@pytest.mark.parametrize("n", [2, 3])
def test_reader_shards_with_cuts_inside_a_quoted_value(gpu, tmp_path, monkeypatch, n):
    from exon_duckdb_amd.reader import ShardReader
    data = shard_file(n - 1)
    rows = user_rows(data)
    p = tmp_path / "cut.gtf"
    p.write_bytes(data)
    monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", str(16 << 10))
    monkeypatch.setenv("EXG_SHARD_HALO", "512")                 # (the halo grows until it holds the line across the cut)
    got, counts = [], 0
    for i in range(n):
        got += reader_rows(p, shard_index=i, shard_count=n)
        r = ShardReader(str(p), "gtf", shard_index=i, shard_count=n)
        counts += r.count()
        r.close()
    assert got == rows and counts == len(rows)


def test_reader_forced_stripes(files, monkeypatch):
    from exon_duckdb_amd.reader import ShardReader
    _, f = files
    path, _, rows = f["big"]
    monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", str(16 << 10))
    monkeypatch.setenv("EXON_GPU_SHARDS", "5")
    monkeypatch.setenv("EXG_FANOUT_WORKERS", "3")
    assert reader_rows(path, shard_count=0) == rows
    r = ShardReader(path, "gtf", shard_count=0)
    assert r.count() == len(rows)
    r.close()


def test_reader_memory_cap(gpu, tmp_path, monkeypatch):
    """a file of 48 MiB built by repeating one block, under EXG_DEVICE_MEM_CAP_MB=16: the digest of the uncapped read, and the
    peak under the cap"""
    from exon_duckdb_amd.reader import ShardReader
    cap_mb = 16
    block = G.mixed(G.rng(23), 3000, comment_every=50)
    n_block = len(user_rows(block))
    times = (48 << 20) // len(block) + 1
    path = tmp_path / "big.gtf"
    with open(path, "wb") as f:
        for _ in range(times):
            f.write(block)
    cols = [0, 2, 3, 5, 6]
    monkeypatch.delenv("EXG_DEVICE_MEM_CAP_MB", raising=False)
    r = ShardReader(str(path), "gtf", columns=cols)
    free = r.digest(per_column=True)
    r.close()
    monkeypatch.setenv("EXG_DEVICE_MEM_CAP_MB", str(cap_mb))
    r = ShardReader(str(path), "gtf", columns=cols)
    capped = r.digest(per_column=True)
    st = r.stats()
    r.close()
    print(f"cap {cap_mb} MiB: peak {st['device_bytes_peak'] / 1048576:.2f} MiB, {st['device_batches']} batches of {st['device_batch_bytes']} bytes")
    assert free == capped and capped[0] == n_block * times
    assert st["device_bytes_peak"] <= cap_mb << 20 and st["device_batches"] >= 8, st
    # with the attributes: their children are the batch's own scratch on top
    r = ShardReader(str(path), "gtf", columns=[0, 8])
    with_attrs = r.digest(nested=True)
    st = r.stats()
    r.close()
    print(f"cap {cap_mb} MiB with attributes: peak {st['device_bytes_peak'] / 1048576:.2f} MiB")
    assert with_attrs[0] == n_block * times and st["device_bytes_peak"] <= cap_mb << 20, st


def test_the_same_input_twice_gives_byte_identical_outputs(gpu, mix):
    import torch
    from exon_duckdb_amd import abi, device
    _, keep, _ = G.read(mix, attributes=False)
    n = len(keep)
    kept_rows = [i for i, k in enumerate(keep) if k]
    outs = []
    for _ in range(2):
        d_in = device.upload(mix)
        scan = device.GtfScan(len(mix), capacity_records=n)
        for t in scan.cols + list(scan.validity.values()) + [scan.keep]:
            t.zero_()                                           # (a comment line's slots are not written: zeros in both runs)
        scan.launch(d_in, algo=abi.EXG_ALGO_FUSED_FULL)
        assert scan.fetch().n_records == n
        row_map = torch.tensor(kept_rows, dtype=torch.int32).cuda()
        ent, keys, vals, _, r = device.gtf_attributes(scan.cols[8], len(kept_rows), d_in, scan.PAYLOAD_BASE, row_map=row_map)
        assert r.error_code == 0
        outs.append([c[:n].cpu().numpy().tobytes() for c in scan.cols] + [v.cpu().numpy().tobytes() for v in scan.validity.values()] +
                    [scan.keep.cpu().numpy().tobytes(), ent.cpu().numpy().tobytes(), keys.cpu().numpy().tobytes(), vals.cpu().numpy().tobytes()])
    assert outs[0] == outs[1]


# ---------------------------------------------------------------- 5. fuzz
@pytest.mark.parametrize("seed", range(6))
def test_fuzz_scan(gpu, seed):
    check(FZ.scan_input(seed))


@pytest.mark.parametrize("seed", range(4))
def test_fuzz_attributes(gpu, seed):
    check_attributes(FZ.attribute_fields(seed))


@pytest.mark.parametrize("seed", range(3))
def test_fuzz_reader(gpu, tmp_path, monkeypatch, seed):
    data = FZ.scan_input(2 * seed, n_lines=400)                 # (even seeds: no mutated line)
    p = tmp_path / "fuzz.gtf"
    p.write_bytes(data)
    monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", "8192")
    assert reader_rows(p) == user_rows(data)
