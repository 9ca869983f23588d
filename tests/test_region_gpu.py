"""vcf_query on the device: the reference's pins on its own indexed file (tests/golden/vcf-index/), rows against a brute-force
filter of the full read_vcf rows at the chunk boundary and through vcf_query_reader, the region predicate alone on scanned
columns, generated files whose members cut lines (tests/tabix_files.py is the oracle: writer, index, planner, row rule), the
proof that the index is used (region_members), and projection / filters / COUNT(*) / the memory cap / a stale index."""
import os
import random

import numpy as np
import pytest

import tabix_files as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "vcf-index", "index.vcf.gz")


@pytest.fixture(scope="module")
def con(gpu):
    from exon_duckdb_amd.table_function import connect
    return connect()


@pytest.fixture(scope="module")
def fixture_rows(con):
    """the full read_vcf rows of the indexed file (computed once), and the text's own view of them for the brute force"""
    full = con.table_function("read_vcf", FIXTURE).fetchall()
    text = T.rows_of(T.bgunzip(open(FIXTURE, "rb").read()))
    assert len(full) == len(text) == 621
    return full, text


def kept_indices(text_rows, region):
    return [i for i, r in enumerate(text_rows) if T.keeps(r[0], r[1], r[2], r[3], *region)]


# ---- the reference's pins ------------------------------------------------------------------------------------------------------
def test_fixture_counts_and_first_row(con, fixture_rows):
    # SELECT COUNT(*) FROM vcf_query('vcf-index/index.vcf.gz', '1') -> 191                       (test_vcf_record_scan.test:43-46)
    rel = con.table_function("vcf_query", FIXTURE, region="1")
    assert rel.count() == 191 and rel.last_max_threads == 1
    # SELECT chrom, pos, ref, alt, qual, info.indel, info.dp FROM vcf_query(..., '1') LIMIT 1 -> 1, 9999919, G, [<*>], 0.0, NULL, 1  (:48-57)
    chrom, pos, ref, alt, qual, info = rel.fetchall(columns=["chrom", "pos", "ref", "alt", "qual", "info"], limit=1)[0]
    assert (chrom, pos, ref, alt, qual, info["INDEL"], info["DP"]) == (b"1", 9999919, b"G", [b"<*>"], 0.0, None, 1)
    full, text = fixture_rows
    counts = {name: con.table_function("vcf_query", FIXTURE, region=name).count() for name in ("1", "2", "10")}
    assert counts == {n: len(kept_indices(text, (n.encode(), 1, T.UNBOUNDED))) for n in counts} and sum(counts.values()) == 621
    assert rel.names == con.table_function("read_vcf", FIXTURE).names


def fixture_regions(text):
    pos = {c: [r[1] for r in text if r[0] == c] for c in (b"1", b"2", b"10")}
    return [(b"1", pos[b"1"][10], pos[b"1"][50]), (b"1", 1, pos[b"1"][0]), (b"1", pos[b"1"][-1], T.UNBOUNDED),     # the first and the last row of a chunk
            (b"2", 1, pos[b"2"][0]), (b"2", pos[b"2"][-1], pos[b"2"][-1]), (b"10", pos[b"10"][5], pos[b"10"][5]),
            (b"2", pos[b"2"][3] + 1, pos[b"2"][4] - 1) if pos[b"2"][4] - pos[b"2"][3] > 1 else (b"2", 1, 1),       # between two rows: nothing
            (b"10", 1, T.UNBOUNDED), (b"1", pos[b"1"][-1] + 1, T.UNBOUNDED), (b"2", 1, 5)]


def test_fixture_rows_equal_brute_force_at_both_boundaries(con, fixture_rows):
    import pyarrow as pa
    from exon_duckdb_amd import arrow, device
    full, text = fixture_rows
    whole = arrow.new_reader(FIXTURE, "vcf").read_all()
    sizes = []
    for reg in fixture_regions(text):
        want = kept_indices(text, reg)
        got = con.table_function("vcf_query", FIXTURE, region=T.region_text(reg)).fetchall()
        assert got == [full[i] for i in want], reg
        table = device.vcf_query_reader(FIXTURE, T.region_text(reg)).read_all()
        assert table.schema == whole.schema and table.equals(whole.take(pa.array(want, type=pa.int64()))), reg
        sizes.append(len(want))
    assert 0 in sizes and 1 in sizes and max(sizes) > 40


# ---- the predicate alone -------------------------------------------------------------------------------------------------------
INFO_FORMS = [b"END=1500", b"X=1;END=1500", b"SVEND=9000;END=1200", b"END", b"END=.", b"DP=4;END=1001", b".", b"SVEND=1500", b"END=999;DP=1",
              b"DP=1", b"END=5x", b"END=2500"]


def predicate_text(n_rows):
    rng = random.Random(n_rows)
    lines, rows = [], []
    for k in range(n_rows):
        chrom = (b"1", b"10", b"1", b"chr_of_more_than_twelve_bytes")[k % 4 if k % 11 else 3]
        pos = rng.choice([990, 999, 1000, 1001, 1500, 2000, 2001, 700, 1])
        ref = b"A" * (300 if k % 7 == 3 else 1 + k % 3)
        info = INFO_FORMS[k % len(INFO_FORMS)]
        lines.append(T.vcf_line(chrom, pos, ref=ref, info=info))
        rows.append((chrom, pos, ref, info))
    return b"".join(lines), rows


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 4097])
def test_region_keep_on_scanned_columns(gpu, n_rows):
    from exon_duckdb_amd import device
    text, rows = predicate_text(n_rows)
    base = 1 << 40
    d_in = device.upload(text)
    scan = device.VcfScan(len(text))
    scan.launch(d_in, payload_base=base)
    res = scan.fetch()
    assert res.error_code == 0 and res.n_records == n_rows
    for name, start, end in ((b"1", 1000, 2000), (b"10", 1000, 2000), (b"1", 1000, T.UNBOUNDED), (b"chr_of_more_than_twelve_bytes", 1, 1000),
                             (b"1", 1001, 1001)):
        words = device.vcf_region_keep(scan, n_rows, d_in, base, name, start, end)
        want = np.zeros(((n_rows + 63) // 64) * 64, np.uint8)
        want[:n_rows] = [T.keeps(c, p, r, i, name, start, end) for c, p, r, i in rows]
        assert np.array_equal(words, np.packbits(want, bitorder="little").view(np.uint64)), (name, start, end)   # (the tail bits are zero)
    if n_rows >= 63:
        assert 0 < int(want.sum()) < n_rows


# ---- generated files -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    out = {}
    for member_bytes in (512, 4096):
        path = str(tmp_path_factory.mktemp("region") / ("m%d.vcf.gz" % member_bytes))
        text = T.synth_vcf(100 + member_bytes)
        # (a member begins with the first line of contig 10: the chunk of region `10` begins at in-member offset 0)
        members, idx = T.write_indexed(path, text, member_bytes, cuts=[next(off for off, line in T.data_lines(text) if line.startswith(b"10\t"))])
        out[member_bytes] = (path, text, members, idx, T.member_offsets(open(path, "rb").read()))
    return out


def special_regions(text_rows):
    """regions that a deletion / an END= record reach into from the left (the long early SV among them), and all of contig 10, whose
    chunk begins with a member"""
    out = [(b"10", 1, T.UNBOUNDED)]
    for chrom, pos, ref, info, _ in text_rows:
        end = T.row_end(pos, ref, info)
        if end > pos + 20 and len(out) < 25:
            out += [(chrom, end, end + 5), (chrom, end + 1, end + 5), (chrom, pos + 1, pos + 1)]
    return out


@pytest.mark.parametrize("member_bytes", [512, 4096])
def test_generated_files_equal_brute_force(gpu, generated, member_bytes):
    from exon_duckdb_amd.reader import ShardReader
    path, text, members, idx, offsets = generated[member_bytes]
    text_rows = T.rows_of(text)
    rng = random.Random(member_bytes)
    regions = special_regions(text_rows) + T.random_regions(rng, idx, 100 - len(special_regions(text_rows)))
    assert len(regions) == 100
    seen = {"two_ranges": 0, "offset0": 0, "offset_in": 0, "seam": 0, "left": 0}
    for reg in regions:
        want = T.rows_in_region(text_rows, reg)
        rd = ShardReader(path, "vcf", region=T.region_text(reg), columns=[0, 1, 3])
        got = rd.rows()
        rd.close()
        assert got == [(r[0], r[1], r[2]) for r in want], reg          # no row twice, none missing, file order
        ranges = T.member_ranges(T.plan(idx, reg), offsets)
        seen["two_ranges"] += len(ranges) >= 2
        seen["offset0"] += any(skip == 0 for _, _, skip in ranges)
        seen["offset_in"] += any(skip > 0 for _, _, skip in ranges)
        # a line straddles the seam at a range's end: the text of its last member does not end with a newline
        seen["seam"] += any(b <= len(members) and text[members[b - 1][1] + members[b - 1][2] - 1:][:1] != b"\n" for _, b, _ in ranges)
        seen["left"] += any(r[1] < reg[1] for r in want)
    assert all(seen.values()), seen


def test_generated_file_whole_rows_through_the_table_function(con, generated):
    path, text, members, idx, offsets = generated[512]
    full = con.table_function("read_vcf", path).fetchall()
    text_rows = T.rows_of(text)
    assert len(full) == len(text_rows)
    sv = next(r for r in text_rows if b"SVTYPE" in r[3])
    for reg in ((sv[0], T.row_end(sv[1], sv[2], sv[3]) - 100, T.row_end(sv[1], sv[2], sv[3]) + 3000), (b"chrX:1", 1, T.UNBOUNDED), (b"10", 500000, 520000)):
        want = [full[i] for i in kept_indices(text_rows, reg)]
        assert con.table_function("vcf_query", path, region=T.region_text(reg)).fetchall() == want and want, reg


# ---- the index is used -----------------------------------------------------------------------------------------------------------
def test_the_index_is_used(gpu, tmp_path):
    from exon_duckdb_amd.reader import ShardReader
    text, members, idx, window = T.spread_file()
    path = str(tmp_path / "spread.vcf.gz")
    T.write_indexed(path, text, T.SPREAD_MEMBER_BYTES)
    offsets = T.member_offsets(open(path, "rb").read())
    planned = sum(b - a for a, b, _ in T.member_ranges(T.plan(idx, window), offsets)) + T.header_members(text, members)
    rd = ShardReader(path, "vcf", region=T.region_text(window))
    assert rd.count() == len(T.rows_in_region(T.rows_of(text), window)) == 40
    got = rd.stats()["region_members"]
    rd.close()
    assert len(members) >= 64 and got == planned and got < len(offsets) / 4, (got, planned, len(offsets))
    whole = ShardReader(path, "vcf", compression="gzip")
    assert whole.count() == 64 * 40 and whole.stats()["region_members"] == 0
    whole.close()


# ---- other behaviour -------------------------------------------------------------------------------------------------------------
def test_projection_filters_and_count(con, fixture_rows):
    from exon_duckdb_amd.table_function import F
    full, text = fixture_rows
    reg = (b"1", text[20][1], text[150][1])
    kept = [full[i] for i in kept_indices(text, reg)]
    rel = con.table_function("vcf_query", FIXTURE, region=T.region_text(reg))
    names = rel.names
    assert rel.fetchall(columns=["pos", "ref"]) == [(r[names.index("pos")], r[names.index("ref")]) for r in kept]     # projection
    assert rel.fetchall(columns=["info"]) == [(r[names.index("info")],) for r in kept]                               # a nested column alone
    assert rel.count() == len(kept)
    # a pushed-down qual / pos predicate ANDed with the region
    mid = text[80][1]
    quals = sorted({r[names.index("qual")] for r in kept if r[names.index("qual")] is not None})
    q = quals[len(quals) // 2]
    filters = {"pos": F.cmp(">=", mid), "qual": F.cmp("<=", q)}
    want = [r for r in kept if r[names.index("pos")] >= mid and r[names.index("qual")] is not None and r[names.index("qual")] <= q]
    assert rel.fetchall(filters=filters) == want and 0 < len(want) < len(kept)
    assert rel.count(filters=filters) == len(want)
    assert rel.count(filters={"chrom": F.cmp("=", b"2")}) == 0         # the region's chrom AND another: nothing


def test_memory_cap(gpu, generated, monkeypatch):
    from exon_duckdb_amd.reader import ShardReader
    path, text, members, idx, offsets = generated[4096]
    reg = (b"10", 1, T.UNBOUNDED)
    want = [(r[0], r[1]) for r in T.rows_in_region(T.rows_of(text), reg)]
    monkeypatch.setenv("EXG_DEVICE_MEM_CAP_MB", "1")      # (64 KiB device batches: the range takes several segments)
    rd = ShardReader(path, "vcf", region=T.region_text(reg), columns=[0, 1])
    assert rd.rows() == want
    st = rd.stats()
    rd.close()
    assert st["device_mem_cap"] == 1 << 20 and st["device_batch_bytes"] == 64 << 10 and st["decoded_segments"] >= 2


def test_a_stale_index_fails_with_the_message(con, generated, tmp_path):
    from exon_duckdb_amd import ExgError
    path, text, members, idx, offsets = generated[512]
    stale = str(tmp_path / "stale.vcf.gz")
    open(stale, "wb").write(T.bgzip(text, 700)[0])                     # the file compressed again: other member boundaries
    open(stale + ".tbi", "wb").write(open(path + ".tbi", "rb").read())
    with pytest.raises(ExgError, match="the index does not belong to this file"):
        con.table_function("vcf_query", stale, region="10")
    foreign = str(tmp_path / "foreign.vcf.gz")                          # another file's index: its offsets lie outside this file
    open(foreign, "wb").write(T.bgzip(T.HEADER + T.vcf_line(b"10", 5), 512)[0])
    open(foreign + ".tbi", "wb").write(open(path + ".tbi", "rb").read())
    with pytest.raises(ExgError, match="the index does not belong to this file"):
        con.table_function("vcf_query", foreign, region="10")
    assert con.table_function("vcf_query", path, region="10").count() > 0        # and the right pair still reads
    with pytest.raises(ExgError, match="no reference sequence named '3'"):      # a name the index does not hold: at bind
        con.table_function("vcf_query", FIXTURE, region="3")
