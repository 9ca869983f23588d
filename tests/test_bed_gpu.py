"""read_bed_file on the device against the Python reader of tests/bed_files.py: every input through the general path
(EXG_ALGO_MULTIPASS) AND the single-pass scan (EXG_ALGO_FUSED_FULL), with and without EXG_F_NO_STORE, every comparison
exact — rows as tuples (NULL as None, strings resolved out of the input bytes), the row count, and for a failing input the
error's code, record ordinal and byte offset with the rows in front of it intact.  Then the reader (batches, decoders,
shards, fan-out, projection, COUNT(*), the memory cap) and the pushed-down filters on all twelve columns.

Inputs are 150-200 KiB: at least three super-tiles of 32 KiB and a ragged tail."""
import bz2
import gzip
import json
import os

import pytest

import bed_files as B
import filter_oracle as fo
import test_filters_gpu as TF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXPECTED = json.load(open(os.path.join(GOLDEN, "expected_bed.json")))
HALF, SUPER = 16384, 32768           # the single-pass scan's staging unit and its super-tile (two halves)


def as_row(values):
    return tuple(v.encode() if isinstance(v, str) else v for v in values)


def launch(data, algo, flags=None, capacity=None, project=None):
    from exon_duckdb_amd import abi, device
    d_in = device.upload(data)
    scan = device.BedScan(len(data), capacity_records=capacity)
    scan.launch(d_in, flags=(abi.EXG_F_BOF | abi.EXG_F_EOF) if flags is None else flags, algo=algo, project=project)
    return scan, scan.fetch()


def check(data, want_error=None):
    """both algorithms, stored and EXG_F_NO_STORE, against the oracle; -> the oracle's (rows, error)"""
    from exon_duckdb_amd import abi
    rows, err = B.read(data)
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
    r = ShardReader(str(path), "bed", **kw)
    try:
        return r.rows()
    finally:
        r.close()


# ---------------------------------------------------------------- inputs (built once, never changed)
def mix_bytes():
    """all eight field counts, 25-90-byte lines, a CRLF on every 97th line, no final newline, 3 651 rows (57 * 64 + 3)"""
    data = B.mixed(B.rng(11), 3651, crlf_every=97, final_newline=False)
    lens = [len(ln) for _, ln in B.lines_of(data)]
    assert 150 << 10 <= len(data) <= 200 << 10 and 25 <= min(lens) < 30 and 85 <= max(lens) <= 90 and len(lens) % 64 == 3, (len(data), min(lens), max(lens))
    return data


def far_bytes():
    """a 3 KiB name that begins in front of a half's window and ends inside the half, a 2 000-block line across a super-tile
    seam, a 40 KiB line across two whole halves"""
    rng = B.rng(12)
    data = B.fill_to(rng, b"", 3 * HALF - 2100)
    a0 = len(data)
    data += B.line(rng, 12, name=b"N" * 3072) + b"\n"
    assert a0 < 3 * HALF - 1024 - 900 and 3 * HALF < len(data) < 4 * HALF
    data = B.fill_to(rng, data, 2 * SUPER - 8100)
    b0 = len(data)
    data += B.line(rng, 12, n_blocks=2000, trailing_comma=True) + b"\n"
    assert b0 < 2 * SUPER - 7000 and len(data) > 2 * SUPER + 4000
    data = B.fill_to(rng, data, 7 * HALF - 3100)
    c0 = len(data)
    data += B.line(rng, 6, name=b"L" * (40 << 10)) + b"\r\n"
    assert c0 < 7 * HALF and len(data) > 9 * HALF
    data = B.fill_to(rng, data, 185 << 10)
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
    pinned = [as_row(r) for r in EXPECTED["test3.bed"]["rows"]]
    rows, err = check(open(os.path.join(GOLDEN, "bed/test3.bed"), "rb").read())
    assert err is None and rows == pinned
    con = table_function.connect()
    for f in EXPECTED["test3.bed"]["files"]:
        path = os.path.join(GOLDEN, f)
        assert reader_rows(path) == pinned, f
        rel = con.table_function("read_bed_file", path)
        assert rel.names == B.NAMES and rel.fetchall() == pinned and rel.count() == 1, f
        assert list(rel.types) == [2 if c in B.INT_COLS else 1 for c in range(12)]      # BIGINT / VARCHAR
        assert con.from_path(path).fetchall(limit=1) == pinned, f        # test_bed_io.test:4-18 through the replacement scan
    hg = [as_row(r) for r in EXPECTED["hg38.head.bed"]["rows"]]
    path = os.path.join(GOLDEN, "bed/hg38.head.bed")
    assert check(open(path, "rb").read())[0] == hg and reader_rows(path) == hg
    assert con.table_function("read_bed_file", path).fetchall(columns=["end", "reference_sequence_name"]) == [(r[2], r[0]) for r in hg]


# ---------------------------------------------------------------- 2. - 4. shapes
def test_field_count_mix_crlf_and_unterminated_tail(gpu, mix):
    rows, err = check(mix)
    assert err is None and len(rows) == 3651 and {sum(v is not None for v in r[:9]) for r in rows} >= {3}


def test_dense_half_is_emitted_in_passes(gpu):
    """more lines in a half than its list holds (2 730 six-byte lines against 1 024), then ordinary lines"""
    data = B.fill_to(B.rng(13), b"c\t1\t2\n" * 3200, 160 << 10)[:-1]
    rows, err = check(data)
    assert err is None and rows[:3200] == [(b"c", 2, 2) + (None,) * 9] * 3200 and len(rows) % 64 != 0


def test_window_far_lines_and_a_line_over_two_halves(gpu, far):
    rows, err = check(far)
    assert err is None
    assert sorted(len(r[3]) for r in rows if r[3] is not None)[-2:] == [3072, 40 << 10]
    assert max(r[9] or 0 for r in rows) == 2000 and max(len(r[10] or b"") for r in rows) > 5000


# ---------------------------------------------------------------- 5. integer edges
EDGE_ROWS = [b"c\t0\t1", b"c\t+7\t13", b"c\t%d\t%d" % (2 ** 63 - 2, 2 ** 63 - 1), b"c\t1\t+0009223372036854775807",
             b"c\t1\t2\tn\t1000", b"c\t1\t2\tn\t1", b"c\t1\t2\tn\t5\t+\t0\t1\t255,0,0", b"c\t1\t2\tn\t5\t-\t%d\t%d\t0,0,255" % (2 ** 63 - 2, 2 ** 63 - 1),
             b"c\t00000000000000000000000007\t13"]
EDGE_ERRORS = [(b"c\t%d\t13" % (2 ** 63 - 1), B.E_POSITION), (b"c\t1\t%d" % 2 ** 63, B.E_POSITION), (b"c\t1\t" + b"9" * 20, B.E_POSITION),
               (b"c\t12345678901234567890\t13", B.E_POSITION), (b"c\t\t13", B.E_POSITION), (b"c\t-1\t13", B.E_POSITION),
               (b"c\t 5\t13", B.E_POSITION), (b"c\t5 \t13", B.E_POSITION), (b"c\t1\t0", B.E_POSITION),
               (b"c\t1\t2\tn\t1001", B.E_SCORE), (b"c\t1\t2\tn\t5\t+\t1\t2\t256,0,0", B.E_COLOR), (b"c\t1\t2\tn\t5\t+\t1\t2\t1,2", B.E_COLOR),
               (b"c\t1\t2\tn\t5\t+\t%d\t2" % (2 ** 63 - 1), B.E_POSITION), (b"c\t1\t2\tn\t5\t+\t1\t0", B.E_POSITION)]


def test_integer_edges_as_rows(gpu):
    rng = B.rng(14)
    data = B.fill_to(rng, b"", 70 << 10) + b"".join(ln + b"\n" for ln in EDGE_ROWS) + B.fill_to(rng, b"", 80 << 10)
    k = len(B.lines_of(B.fill_to(B.rng(14), b"", 70 << 10)))
    rows, err = check(data)
    assert err is None
    assert [r[1:3] for r in rows[k:k + 4]] == [(1, 1), (8, 13), (2 ** 63 - 1, 2 ** 63 - 1), (2, 2 ** 63 - 1)]
    assert [r[4] for r in rows[k + 4:k + 6]] == [1000, 1] and rows[k + 6][6:9] == (1, 1, b"255,0,0")
    assert rows[k + 7][6:9] == (2 ** 63 - 1, 2 ** 63 - 1, b"0,0,255") and rows[k + 8][1] == 8


@pytest.mark.parametrize("case", range(len(EDGE_ERRORS)))
def test_integer_edges_as_errors(gpu, case):
    bad, code = EDGE_ERRORS[case]
    front = B.mixed(B.rng(15), 70)
    rows, err = check(front + bad + b"\n" + B.mixed(B.rng(16), 30), want_error=(70, code))
    assert len(rows) == 70 and err[2] == len(front)


# ---------------------------------------------------------------- 6. errors
BAD_LINES = {B.E_FIELD_COUNT: b"c\t1\t2\tn\t5\t+\t1\t2\t0\t1", B.E_REFERENCE_NAME: b"\t1\t2", B.E_POSITION: b"c\tx\t2", B.E_SCORE: b"c\t1\t2\tn\t.",
             B.E_STRAND: b"c\t1\t2\tn\t5\t*", B.E_COLOR: b"c\t1\t2\tn\t5\t+\t1\t2\tred", B.E_BLOCKS: b"c\t1\t2\tn\t5\t+\t1\t2\t0\t3\t1,2\t1,2,3"}


@pytest.fixture(scope="module")
def base_lines():
    data = B.mixed(B.rng(17), 2600)
    assert len(data) > 3 * SUPER + 5000
    return [ln for _, ln in B.lines_of(data)]


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


def test_the_earlier_of_two_bad_lines_wins(gpu, base_lines):
    mid = line_in_second_super_tile(base_lines)
    later = mid + 1200                                                     # two super-tiles further on
    assert sum(len(ln) + 1 for ln in base_lines[mid:later]) > SUPER
    check(with_lines(base_lines, {mid: BAD_LINES[B.E_STRAND], later: BAD_LINES[B.E_FIELD_COUNT]}), want_error=(mid, B.E_STRAND))
    check(with_lines(base_lines, {mid: BAD_LINES[B.E_FIELD_COUNT], later: BAD_LINES[B.E_POSITION], 5: BAD_LINES[B.E_COLOR]}), want_error=(5, B.E_COLOR))


def test_utf8_is_validated_behind_the_fields(gpu, base_lines):
    mid = line_in_second_super_tile(base_lines)
    rows, err = check(with_lines(base_lines, {mid: b"c\t1\t2\tn\xc3\xa9m\t7", mid + 3: b"chr\xc3\xa9\t1\t2"}))
    assert err is None and rows[mid][3] == b"n\xc3\xa9m" and rows[mid + 3][0] == b"chr\xc3\xa9"
    check(with_lines(base_lines, {mid: b"c\t1\t2\tn\xc3\xa9", mid + 3: b"c\t1\t2\tn\xffm\t7"}), want_error=(mid + 3, B.E_INVALID_UTF8))
    check(with_lines(base_lines, {mid: b"c\t1\tx\tn\xff"}), want_error=(mid, B.E_POSITION))      # the field's error comes first
    # a line that begins in front of its half's window: validated by the kernel behind the scan
    long_bad = b"c\t1\t2\t" + b"L" * 3000 + b"\xe9" + b"L" * 3000
    check(with_lines(base_lines, {mid: long_bad}), want_error=(mid, B.E_INVALID_UTF8))


# ---------------------------------------------------------------- 7. capacity and projection
def test_capacity_one_short_and_null_column_pointers(gpu, mix):
    from exon_duckdb_amd import abi
    rows, _ = B.read(mix)
    for algo in (abi.EXG_ALGO_MULTIPASS, abi.EXG_ALGO_FUSED_FULL):
        scan, res = launch(mix, algo, capacity=len(rows) - 1)
        assert res.flags & abi.EXG_RF_CAPACITY and res.n_records == len(rows) - 1 and res.error_code == 0, algo
        assert scan.rows(len(rows) - 1, mix) == rows[:-1], algo
        scan, res = launch(mix, algo, capacity=len(rows))
        assert not res.flags & abi.EXG_RF_CAPACITY and res.n_records == len(rows), algo
        keep = [0, 2, 5, 10]
        scan, res = launch(mix, algo, project=keep)
        assert res.n_records == len(rows) and res.error_code == 0, algo
        assert scan.rows(len(rows), mix, columns=keep) == [tuple(r[c] for c in keep) for r in rows], algo
        # a column that is not produced is still validated
        cut = mix.rfind(b"\n", 0, 40000) + 1
        bad = mix[:cut] + b"c\t1\t2\tn\t5\t?\n" + mix[cut:]
        want = B.read(bad)[1]
        _, res = launch(bad, algo, project=[1])
        assert want[1] == B.E_STRAND and (res.error_record, res.error_code, res.error_offset) == want, algo
    from exon_duckdb_amd import ExgError
    with pytest.raises(ExgError):
        launch(mix, abi.EXG_ALGO_FUSED_INDEX)


def test_auto_and_fused_are_the_single_pass_scan(gpu, far):
    from exon_duckdb_amd import abi
    rows, _ = B.read(far)
    for algo in (abi.EXG_ALGO_AUTO, abi.EXG_ALGO_FUSED):
        scan, res = launch(far, algo)
        assert res.n_records == len(rows) and res.error_code == 0 and not res.flags & (abi.EXG_RF_FALLBACK | abi.EXG_RF_REDO)
        assert scan.rows(len(rows), far) == rows


# ---------------------------------------------------------------- 8. the reader
@pytest.fixture(scope="module")
def files(gpu, mix, far, tmp_path_factory):
    d = tmp_path_factory.mktemp("bed_reader")
    out = {}
    for name, data in (("mix", mix), ("far", far)):
        p = d / (name + ".bed")
        p.write_bytes(data)
        out[name] = (str(p), data, B.read(data)[0])
    return d, out


def test_reader_default_and_4096_byte_batches(files, monkeypatch):
    from exon_duckdb_amd import table_function
    from exon_duckdb_amd.reader import ShardReader
    _, f = files
    for name, (path, _, rows) in f.items():
        monkeypatch.delenv("EXG_DEVICE_BATCH_BYTES", raising=False)
        assert reader_rows(path) == rows, name
        assert table_function.connect().table_function("read_bed_file", path).fetchall() == rows, name
        monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", "4096")
        r = ShardReader(path, "bed")
        assert r.rows() == rows, name
        st = r.stats()
        r.close()
        assert st["device_batches"] >= 20 and st["scan_algo"] == 3, (name, st)      # EXG_ALGO_FUSED_FULL throughout
        r = ShardReader(path, "BED")                                                  # (any case)
        assert r.count() == len(rows) and r.stats()["host_vector_bytes"] == 0, name
        r.close()


def test_reader_errors_name_the_byte_and_keep_the_rows_in_front(files, base_lines, tmp_path):
    from exon_duckdb_amd import ExgError
    mid = line_in_second_super_tile(base_lines)
    data = with_lines(base_lines, {mid: BAD_LINES[B.E_SCORE]})
    rows, err = B.read(data)
    p = tmp_path / "bad.bed"
    p.write_bytes(data)
    from exon_duckdb_amd.reader import ShardReader
    r = ShardReader(str(p), "bed")
    with pytest.raises(ExgError) as e:
        r.rows()
    r.close()
    assert f"at byte {err[2]} of" in str(e.value) and "score" in str(e.value)
    with pytest.raises(ExgError):
        ShardReader(str(p), "bed").count()


def test_reader_decoders(files, monkeypatch):
    from exon_duckdb_amd.testing import bgzf
    d, f = files
    path, data, rows = f["mix"]
    bgzf.bgzip(path, str(d / "mix.bgz.bed.gz"))
    (d / "mix.one.bed.gz").write_bytes(gzip.compress(data, 6, mtime=0))
    (d / "mix.bed.bz2").write_bytes(bz2.compress(data))
    for batch in (None, "4096"):
        if batch:
            monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", batch)
        assert reader_rows(d / "mix.bgz.bed.gz") == rows
        assert reader_rows(d / "mix.one.bed.gz") == rows
        assert reader_rows(d / "mix.bed.bz2", compression="bzip2") == rows
    from exon_duckdb_amd import table_function
    con = table_function.connect()
    assert con.from_path(str(d / "mix.bgz.bed.gz")).fetchall(columns=["name", "start"]) == [(r[3], r[1]) for r in rows]
    assert con.table_function("read_bed_file", str(d / "mix.bed.bz2"), compression="bzip2").count() == len(rows)


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
            got += reader_rows(path, shard_index=i, shard_count=n)
            r = ShardReader(path, "bed", shard_index=i, shard_count=n)
            counts += r.count()
            r.close()
        assert got == rows and counts == len(rows), (name, n)
    monkeypatch.setenv("EXON_GPU_SHARDS", "5")
    monkeypatch.setenv("EXG_FANOUT_WORKERS", "3")
    assert reader_rows(path, shard_count=0) == rows, name
    r = ShardReader(path, "bed", shard_count=0)
    assert r.count() == len(rows)
    r.close()
    if name == "mix":
        gz = str(d / "shards.bed.gz")
        bgzf.bgzip(path, gz)
        assert sum((reader_rows(gz, shard_index=i, shard_count=3) for i in range(3)), []) == rows
        assert reader_rows(gz, shard_count=0) == rows


def test_reader_projection_and_count_bytes(files):
    from exon_duckdb_amd.reader import ShardReader
    _, f = files
    path, _, rows = f["mix"]
    r = ShardReader(path, "bed", columns=[1])
    assert r.rows() == [(x[1],) for x in rows] and r.stats()["host_vector_bytes"] == 8 * len(rows)
    r.close()
    r = ShardReader(path, "bed", columns=[0, 9, 4])
    assert r.rows() == [(x[0], x[4], x[9]) for x in rows]
    r.close()
    r = ShardReader(path, "bed")
    assert r.count() == len(rows) and r.stats()["host_vector_bytes"] == 0
    r.close()


def test_reader_memory_cap(gpu, tmp_path, monkeypatch):
    """a file of 128 MiB built by repeating one block, under EXG_DEVICE_MEM_CAP_MB=16: the digest of the uncapped read, and the
    peak under the cap"""
    from exon_duckdb_amd.reader import ShardReader
    cap_mb = 16
    block = B.mixed(B.rng(18), 12000, counts=(12, 9, 12))
    times = (128 << 20) // len(block) + 1
    path = tmp_path / "big.bed"
    with open(path, "wb") as f:
        for _ in range(times):
            f.write(block)
    n_rows = 12000 * times
    cols = [1, 2, 3, 9]
    monkeypatch.delenv("EXG_DEVICE_MEM_CAP_MB", raising=False)
    r = ShardReader(str(path), "bed", columns=cols)
    free = r.digest(per_column=True)
    r.close()
    monkeypatch.setenv("EXG_DEVICE_MEM_CAP_MB", str(cap_mb))
    r = ShardReader(str(path), "bed", columns=cols)
    capped = r.digest(per_column=True)
    st = r.stats()
    r.close()
    print(f"cap {cap_mb} MiB: peak {st['device_bytes_peak'] / 1048576:.2f} MiB, {st['device_batches']} batches of {st['device_batch_bytes']} bytes")
    assert os.path.getsize(path) >= 128 << 20 and free == capped and capped[0] == n_rows
    assert st["device_bytes_peak"] <= cap_mb << 20 and st["device_batches"] >= 8, st
    r = ShardReader(str(path), "bed")
    assert r.count() == n_rows
    r.close()


# ---------------------------------------------------------------- 9. filters
N_ROWS = 333
F_CHROMS = [b"1", b"chr1", b"chr1_random", b"chr1_randomA", b"chr1_randomAB", b"chr1_randomAC", b"chr1Xrandom", b"chr\xc3\xa9", b"\xc3\xa9",
            b"L" * 300, b"L" * 299 + b"M"]
F_STARTS = [0, 2147483646, 2147483647, 9007199254740991, 9007199254740992, 2 ** 63 - 2, 4]
F_ENDS = [1, 2147483647, 2 ** 63 - 1, 5, 9007199254740993]
F_NAMES = [b".", b"n", b"name_prefix_A", b"name_prefix_B", b"name_prefix_AB", b"N" * 300, b"it's"]
F_SCORES = [b"0", b"1", b"1000", b"500"]
F_STRANDS = [b"+", b"-", b"."]
F_COLORS = [b"0", b"255,0,0", b"0,0,0", b"12,34,56", b"255,255,255"]
F_BLOCKS = [(0, b"", b""), (1, b"5", b"0"), (2, b"2,1", b"0,3"), (3, b"10,20,30,", b"0,100,2000"), (2, b"123456,7890123", b"0,1234567890123")]
F_COUNTS = [12, 3, 4, 5, 12, 6, 7, 8, 9, 12, 12, 6, 12]
SCHEMA = {n: "l" if k in B.INT_COLS else "u" for k, n in enumerate(B.NAMES)}


def filter_bytes():
    lines = []
    for r in range(N_ROWS):
        bc, bs, bt = F_BLOCKS[r % 5]
        f = [F_CHROMS[r % 11], b"%d" % F_STARTS[r % 7], b"%d" % F_ENDS[r % 5], F_NAMES[r % 7], F_SCORES[r % 4], F_STRANDS[r % 3],
             b"%d" % F_STARTS[(r + 3) % 7], b"%d" % F_ENDS[(r + 2) % 5], F_COLORS[r % 5], b"%d" % bc, bs, bt]
        lines.append(b"\t".join(f[:F_COUNTS[r % 13]]) + b"\n")
    return b"".join(lines)


def int_literals(values):
    out = []
    for v in values:
        out += [str(v), str(v + 1), str(v - 1)]
    return sorted(set(out), key=int) + ["4.5", "9007199254740992.0", "1e10", "-1"]


@pytest.fixture(scope="module")
def bed_site(gpu, tmp_path_factory):
    data = filter_bytes()
    rows, err = B.read(data)
    assert err is None and len(rows) == N_ROWS
    p = tmp_path_factory.mktemp("filters_bed") / "edge.bed"
    p.write_bytes(data)
    dict_rows = [dict(zip(B.NAMES, r)) for r in rows]
    lit = {"reference_sequence_name": TF.string_literals(F_CHROMS), "name": TF.string_literals([n for n in F_NAMES if n != b"."]),
           "strand": [b"+", b"-", b"", b"+ ", b"."], "color": TF.string_literals([c for c in F_COLORS if c != b"0"]),
           "block_sizes": TF.string_literals(sorted({b",".join(bs.split(b",")[:bc]) for bc, bs, _ in F_BLOCKS})),
           "block_starts": TF.string_literals(sorted({bt for _, _, bt in F_BLOCKS})),
           "start": int_literals([v + 1 for v in F_STARTS if v + 2 < 2 ** 63]) + [str(2 ** 63 - 1)],
           "end": int_literals([v for v in F_ENDS if v + 1 < 2 ** 63]) + [str(2 ** 63 - 1)],
           "score": ["0", "1", "2", "500", "999", "1000", "1001", "499.5"],
           "thick_start": int_literals([v + 1 for v in F_STARTS if v + 2 < 2 ** 63]), "thick_end": int_literals([v for v in F_ENDS if v + 1 < 2 ** 63]),
           "block_count": ["0", "1", "2", "3", "4", "-1", "1.5"]}
    return TF.Site(p, "bed", "read_bed_file", B.NAMES, list(B.NAMES), SCHEMA, dict_rows, lit)


@pytest.fixture(params=["default", "small"])
def batch(request, monkeypatch):
    if request.param == "small":
        monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", "4096")
    else:
        monkeypatch.delenv("EXG_DEVICE_BATCH_BYTES", raising=False)
    return request.param


@pytest.mark.parametrize("col", B.NAMES)
def test_filters_every_leaf(bed_site, batch, col):
    TF.check_leaves(bed_site, col, bed_site.shard_rows)


def test_filters_random_trees(bed_site, batch):
    TF.check_trees(bed_site, TF.trees_for(bed_site, 80, 4), bed_site.shard_rows)
