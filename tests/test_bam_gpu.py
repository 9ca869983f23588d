"""read_bam_file_records on the device, value for value and NULL for NULL against the independent Python reader of
tests/bam_files.py: the reference's fixtures, generated short-read files however their BGZF members and device batches fall,
edge records, long reads, inputs built to fool the record-start speculation, every record error, filters, the refusals at
the boundary, and bounded memory."""
import ctypes as C
import json
import os
import random
import struct

import pytest

import bam_files as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXPECTED = json.load(open(os.path.join(GOLDEN, "expected_bam.json")))
FN = "read_bam_file_records"
TILE = 32768
REFS = [(b"chr%d" % i, 250_000_000) for i in range(1, 23)] + [(b"chrX", 156_000_000), (b"a_decoy_contig_with_a_long_name", 5000)]


def as_row(values):
    return tuple(v.encode() if isinstance(v, str) else v for v in values)


def read_all(path, columns=None, **kw):
    """-> (rows, error or None, stats): the rows that came out before the reader failed, if it did"""
    from exon_duckdb_amd import ExgError
    from exon_duckdb_amd.reader import ShardReader
    from exon_duckdb_amd.table_function import Chunk, decode_vector
    r = ShardReader(str(path), "bam", columns=columns, **kw)
    rows, err = [], None
    want = range(len(r.names)) if r.columns is None else r.columns
    while True:
        ch = Chunk()
        rc = r._l.exg_next_chunk(r._r, C.byref(ch))
        if rc != 0:
            err = ExgError(rc, (r._l.exg_reader_error(r._r) or b"").decode("utf-8", "replace"))
            break
        if ch.n_rows == 0:
            break
        rows.extend(zip(*[decode_vector(ch.vectors[k].contents, r.trees[k]) for k in want]))
        r._l.exg_release_chunk(r._r, C.byref(ch))
    st = r.stats()
    r.close()
    return rows, err, st


def write_bam(path, refs, records, cuts=None, **kw):
    raw = B.header(refs) + b"".join(records)
    path.write_bytes(B.bgzf(raw, cuts=cuts, **kw))
    return raw


# ---------------------------------------------------------------- 1. the reference's fixtures
@pytest.mark.parametrize("name", ["bam/example1.bam", "bam/test.bam", "bam-index/test.bam"])
def test_fixtures(gpu, name):
    from exon_duckdb_amd import table_function as tf
    path = os.path.join(GOLDEN, name)
    want = B.parse(path).rows
    exp = EXPECTED[name]
    rel = tf.connect().table_function(FN, path)
    assert rel.names == B.NAMES and [tf.type_sql(t) for t in rel.trees] == B.TYPES
    got = rel.fetchall()
    assert got == want
    if "rows" in exp:
        assert got == [as_row(r) for r in exp["rows"]]
    if "first_row" in exp:
        assert got[0] == as_row(exp["first_row"])
    if "count" in exp:
        assert rel.count() == exp["count"] == len(got)
    assert rel.count() == len(want)
    for c, col in enumerate(B.NAMES):
        assert rel.fetchall(columns=[col]) == [(r[c],) for r in want], col
    assert tf.connect().from_path(path).count() == len(want)     # replacement scan: SELECT ... FROM 'x.bam'
    rows, err, st = read_all(path)
    assert err is None and rows == want and st["input_compression"] == 1
    if name == "bam/test.bam":
        assert st["bam_tiles"] >= 10 and st["bam_tiles_rewalked"] * 50 <= st["bam_tiles"], st


# ---------------------------------------------------------------- 2. short reads, however members and batches fall
@pytest.fixture(scope="module")
def illumina(tmp_path_factory):
    recs = B.illumina_pairs(100_000, REFS, seed=7)
    raw = B.header(REFS, b"@HD\tVN:1.6\tSO:unsorted\n") + b"".join(recs)
    rng = random.Random(3)
    cuts = sorted(rng.randrange(1, len(raw)) for _ in range(len(raw) // 40000))   # mid-record, mid-block_size, anywhere
    path = tmp_path_factory.mktemp("bam") / "illumina.bam"
    path.write_bytes(B.bgzf(raw, cuts=cuts, level=1))
    return path, B.parse_decoded(raw).rows


@pytest.mark.parametrize("batch", [64 << 10, 1 << 20, 0])
def test_short_reads_any_segmentation(gpu, illumina, monkeypatch, batch):
    path, want = illumina
    assert len(want) >= 200_000
    if batch:
        monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", str(batch))
    else:
        monkeypatch.delenv("EXG_DEVICE_BATCH_BYTES", raising=False)
    rows, err, st = read_all(path)
    assert err is None and len(rows) == len(want)
    assert rows == want
    print(f"batch {batch}: tiles {st['bam_tiles']} rewalked {st['bam_tiles_rewalked']} batches {st['device_batches']}")
    # the fast path is not quietly the fallback
    assert st["bam_tiles_rewalked"] * 50 <= st["bam_tiles"], st
    if batch == 64 << 10:
        assert st["device_batches"] > 500, st
    from exon_duckdb_amd.reader import ShardReader
    r = ShardReader(str(path), "bam")
    assert r.count() == len(want)
    r.close()


# ---------------------------------------------------------------- 2b. more rows in a segment than the vectors are provisioned for
@pytest.fixture(scope="module")
def smallest_records(tmp_path_factory):
    """60 000 records as small as a record can be with a name: one character, no CIGAR, no sequence, no aux — 38 bytes each,
    2.3 MB decoded.  Position and flag differ from row to row, so a row out of place is seen."""
    recs = [B.record(name=b"ACGT"[i % 4:i % 4 + 1], flag=(i * 37) % 256, ref=0, pos=i, mapq=i % 61) for i in range(60_000)]
    assert all(len(rec) == 38 for rec in recs)
    raw = B.header([(b"c", 1 << 28)]) + b"".join(recs)
    path = tmp_path_factory.mktemp("bam") / "smallest.bam"
    path.write_bytes(B.bgzf(raw, level=1))
    return path, B.parse_decoded(raw).rows


@pytest.mark.parametrize("filters", [None, "flag>=128"])
def test_smallest_records_overflow_the_provisioned_rows(gpu, smallest_records, monkeypatch, filters):
    """With 1 MiB batches the reader provisions 1 445 888 bytes of input and 1 445 888 / 64 + 4096 = 26 688 rows; a full segment
    of 38-byte records holds about 27 600.  The batch that says so frees every device buffer of the reader — the column vectors,
    the row map and the gather scratch among them — provisions them for the worst case and is scanned again: the rows of that batch
    and of those behind it must be the file's, unfiltered and through the row map."""
    path, want = smallest_records
    monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", str(1 << 20))
    rows, err, st = read_all(path, filters=filters)
    exp = [r for r in want if filters is None or r[1] >= 128]
    assert err is None and len(rows) == len(exp)
    assert rows == exp
    if filters:
        assert 0.4 < len(exp) / len(want) < 0.6
    print(f"filters {filters}: batches {st['device_batches']} segments {st.get('decoded_segments')}")


# ---------------------------------------------------------------- 3. edge records
def edge_records():
    all_ops = [(1, "M"), (2, "I"), (3, "D"), (4, "N"), (5, "S"), (6, "H"), (7, "P"), (8, "="), ((1 << 28) - 1, "X")]
    rng = random.Random(11)
    many = [(rng.choice((1, 9, 10, 99, 100, 12345, (1 << 28) - 1)), rng.randrange(9)) for _ in range(65535)]
    return [
        B.record(b"no_seq", 0, 0, 100, 30, [(10, "M")], 0, 200),                                          # l_seq = 0
        B.record(b"odd", 0, 0, 100, 30, [(13, "M")], 0, 200, 0, b"ACGTACGTACGTA", bytes(range(13))),       # odd l_seq, 13 bytes
        B.record(b"twelve", 0, 0, 0, 0, [(12, "M")], 0, 0, 0, b"ACGTACGTACGT", bytes(range(12))),          # exactly 12: inlined
        B.record(b"absent_qual", 16, 1, 7, 60, [(20, "M")], 1, 7, 0, b"ACGTNACGTNACGTNACGTN", None),       # 0xFF: empty string
        B.record(b"mapq255", 0, 0, 5, 255, [(1, "M")], 0, 5, 0, b"A", b"\x28"),
        B.record(b"no_refs", 4, -1, 50, 0, [(1, "M")], -1, -1, 0, b"C", b"\x00"),                          # refID / next_refID -1
        B.record(b"no_pos", 4, 2, -1, 0, [(1, "M")], 2, -1, 0, b"G", b"\x5d"),                             # pos -1, quality 93
        B.record(b"no_cigar", 4, -1, -1, 255, (), -1, -1, 0, b"ACGT" * 40, bytes([30]) * 160),
        B.record(b"all_ops", 0, 3, 999, 1, all_ops, 3, 999, 0, b"ACGT" * 5, bytes([20]) * 20),             # end beyond... no: fits INTEGER
        B.record(b"end_overflows", 0, 3, 2_000_000_000, 1, [((1 << 28) - 1, "M")] * 2, 3, 0, 0, b"A", b"\x01"),   # end outside INTEGER: NULL
        B.record(b"insertion_only", 0, 3, 0, 1, [(5, "I")], 3, 0, 0, b"ACGTA", bytes(5)),                  # span 0 at start 1: end 0 -> NULL
        B.record(b"many_ops", 0, 0, 0, 9, many, 0, 0, 0, b"AC", b"\x01\x02"),                              # 65535 operations
        B.record(b"x", 0, 0, 1, 2, [(1, "M")], 0, 1, 0, b"T", b"\x03"),                                    # a name of 1 character
        B.record(b"n" * 254, 0, 0, 1, 2, [(1, "M")], 0, 1, 0, b"T", b"\x03"),                              # ... of 254
        B.record(b"exactly12chr", 0, 23, 1, 2, [(123456, "M"), (1234, "N")], 23, 1, 0, b"=ACMGRSVTWYHKDBN", bytes(range(16))),  # cigar 12 chars
        B.record(b"exactly_13chr", 0, 23, 1, 2, [(1234567, "M"), (1234, "N")], 23, 1, 0, b"NBDKHYWTVSRGMCA=", bytes(range(16)), B.aux_z(b"XZ", b"skipped")),
    ]


def test_edge_records(gpu, tmp_path, monkeypatch):
    recs = edge_records()
    path = tmp_path / "edge.bam"
    raw = write_bam(path, REFS, recs, cuts=[len(B.header(REFS)) + 2, len(B.header(REFS)) + 37])
    want = B.parse_decoded(raw)
    assert want.error is None and len(want.rows) == len(recs)
    assert want.rows[9][4] is None and want.rows[10][4] is None and want.rows[8][4] is not None
    assert len(want.rows[11][6]) > 200_000 and want.rows[14][6] == b"123456M1234N" and len(want.rows[15][6]) == 13
    for batch in (None, 64 << 10):
        if batch:
            monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", str(batch))
        rows, err, _ = read_all(path)
        assert err is None and rows == want.rows
    for c in range(10):
        rows, err, _ = read_all(path, columns=[c])
        assert err is None and rows == [(r[c],) for r in want.rows], B.NAMES[c]


def test_header_only_empty_member_and_stored_blocks(gpu, tmp_path):
    from exon_duckdb_amd.reader import ShardReader
    p = tmp_path / "header_only.bam"
    p.write_bytes(B.bgzf(B.header(REFS)))
    rows, err, _ = read_all(p)
    assert err is None and rows == []
    r = ShardReader(str(p), "bam")
    assert r.count() == 0
    r.close()
    recs = B.illumina_pairs(300, REFS, seed=5)
    raw = B.header(REFS) + b"".join(recs)
    cut = len(raw) // 2 + 3
    q = tmp_path / "empty_member.bam"
    q.write_bytes(B.bgzf(raw[:cut], eof=False) + B.BGZF_EOF + B.bgzf(raw[cut:cut + 5000], stored=True, eof=False) + B.bgzf(raw[cut + 5000:]))
    rows, err, _ = read_all(q)
    assert err is None and rows == B.parse_decoded(raw).rows


def test_header_of_100000_references_through_64k_batches(gpu, tmp_path, monkeypatch):
    refs = [(b"scaffold_%06d_of_an_assembly_in_pieces" % i, 1000 + i) for i in range(100_000)]
    recs = [B.record(b"r%d" % i, 0, (i * 7919) % len(refs), i, 60, [(4, "M")], (i * 31) % len(refs), i, 0, b"ACGT", bytes(4)) for i in range(2000)]
    path = tmp_path / "many_refs.bam"
    raw = write_bam(path, refs, recs, level=1)
    assert len(B.header(refs)) > 4 << 20
    monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", str(64 << 10))
    rows, err, _ = read_all(path)
    assert err is None and rows == B.parse_decoded(raw).rows
    assert rows[1][2] == refs[7919][0] and len(rows[1][2]) > 12


# ---------------------------------------------------------------- 4. long reads
def test_long_reads_through_1mib_batches(gpu, tmp_path, monkeypatch):
    rng = random.Random(2)

    def read(i, n):
        seq = rng.randbytes(n).translate(B._TO_BASES)
        return B.record(b"long_read_%d" % i, 0, 0, 1000 * i, 60, [(n // 2, "M"), (5, "D"), (n - n // 2, "M")], -1, -1, 0, seq,
                        rng.randbytes(n).translate(B._TO_QUAL), B.aux_z(b"RG", b"nanopore"))
    recs = [read(i, 100_000) for i in range(6)] + [read(6, 5_000_000)] + [read(7, 100_000)] + B.illumina_pairs(50, REFS, seed=9)
    assert len(recs[6]) > 7_400_000                       # one record of ~7.5 MB: tiles without a record start in them
    path = tmp_path / "long.bam"
    raw = write_bam(path, REFS, recs, level=1)
    want = B.parse_decoded(raw).rows
    monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", str(1 << 20))
    rows, err, st = read_all(path)
    assert err is None and len(rows) == len(want)
    assert rows == want
    rows, err, _ = read_all(path, columns=[0, 4, 6])
    assert err is None and rows == [(r[0], r[4], r[6]) for r in want]


# ---------------------------------------------------------------- 5. inputs built to fool the speculation
def adversarial_stream():
    """records whose name, Z aux value and B aux array hold byte-exact copies of two complete plausible records (the second
    the plausible successor of the first), each placed so that the copy begins exactly at a tile boundary of a scan that
    starts at the stream's first record"""
    fake = B.record(b"f", 0, 0, 5, 7, (), 0, 5) + B.record(b"g", 0, 1, 6, 8, (), 1, 6)
    assert len(fake) == 76 and b"\0" in fake
    out, size = [], 0

    def add(rec):
        nonlocal size
        out.append(rec)
        size += len(rec)

    def pad_to(target):      # records up to a filler that ends exactly at `target`
        while target - size > 3000:
            for r in B.illumina_pairs(2, REFS, seed=size):
                add(r)
        gap = target - size
        assert gap >= 40
        add(B.record(b"p", 4, -1, -1, 255, (), -1, -1, 0, b"", None, b"\x55" * (gap - 38)))
        assert size == target

    seq, qual = b"ACGT" * 10, bytes([30]) * 40
    # a read name that IS two records (binary, NUL-terminated as a whole): the copy begins 36 bytes into the record
    pad_to(2 * TILE - 36)
    add(B.record(fake[:-1], 0, 0, 10, 20, [(40, "M")], 0, 10, 0, seq, qual))
    # a Z value: fixed fields 36, name 2, cigar 4, sequence 20, qualities 40, tag + type 3
    pad_to(5 * TILE - (36 + 2 + 4 + 20 + 40 + 3))
    add(B.record(b"z", 0, 0, 10, 20, [(40, "M")], 0, 10, 0, seq, qual, B.aux_z(b"XZ", fake)))
    # a B array of bytes: tag + type + subtype + count = 8
    pad_to(9 * TILE - (36 + 2 + 4 + 20 + 40 + 8))
    add(B.record(b"b", 0, 0, 10, 20, [(40, "M")], 0, 10, 0, seq, qual, B.aux_b_u8(b"XB", fake)))
    pad_to(12 * TILE + 999)
    return b"".join(out)


def test_adversarial_speculation(gpu, tmp_path):
    from exon_duckdb_amd import abi, device
    stream = adversarial_stream()
    for k in (2, 5, 9):
        assert stream[k * TILE + 36:k * TILE + 38] == b"f\0"       # a complete plausible record begins at the tile boundary
    want = B.parse_decoded(B.header(REFS) + stream)
    assert want.error is None
    scan = device.BamScan(len(stream), REFS)
    d_in = device.upload(stream)
    scan.launch(d_in, flags=abi.EXG_F_EOF)
    res = scan.fetch()
    assert res.error_code == 0 and res.n_records == len(want.rows) and res.consumed_bytes == len(stream)
    assert res.tiles == len(stream) // TILE + 1
    assert res.tiles_rewalked >= 3, "the test did not reach the second walk"
    assert scan.rows(res.n_records, res.side_bytes) == want.rows
    # and through the reader, wherever its batches happen to begin
    path = tmp_path / "adversarial.bam"
    path.write_bytes(B.bgzf(B.header(REFS) + stream))
    rows, err, _ = read_all(path)
    assert err is None and rows == want.rows


def test_scan_entry_tail_no_store_and_capacity(gpu):
    from exon_duckdb_amd import abi, device
    recs = B.illumina_pairs(400, REFS, seed=21)
    stream = b"".join(recs)
    want = B.parse_decoded(B.header(REFS) + stream).rows
    cut = len(stream) - 100                                  # the last record is incomplete: left to the next batch
    scan = device.BamScan(len(stream), REFS)
    d_in = device.upload(stream)
    scan.launch(d_in, n_bytes=cut, flags=0)
    res = scan.fetch()
    assert res.error_code == 0 and res.n_records == len(recs) - 1 and res.consumed_bytes == len(stream) - len(recs[-1])
    assert scan.rows(res.n_records, res.side_bytes) == want[:-1]
    scan.launch(d_in, n_bytes=cut, flags=abi.EXG_F_EOF)      # at the end of the stream the same tail is an error
    res = scan.fetch()
    assert res.error_code == abi.EXG_PE_BAM_TRUNCATED and res.error_record == len(recs) - 1 and res.n_records == len(recs) - 1
    scan.launch(d_in, flags=abi.EXG_F_EOF | abi.EXG_F_NO_STORE)
    res = scan.fetch()
    assert res.n_records == len(recs) and res.side_bytes == 0
    small = device.BamScan(len(stream), REFS, capacity_records=10)
    small.launch(d_in, flags=abi.EXG_F_EOF)
    res = small.fetch()
    assert res.flags & abi.EXG_RF_CAPACITY and res.n_records == len(recs)


# ---------------------------------------------------------------- 6. errors
def bad_records():
    seq, qual = b"ACGTACGTACGTACGTACGT", bytes([30]) * 20
    good = dict(flag=0, ref=0, pos=10, mapq=20, cigar=[(20, "M")], next_ref=0, next_pos=10, seq=seq, qual=qual)
    return {
        B.E_BLOCK_SIZE: B.record(b"bad", block_size=31, **good),
        B.E_READ_NAME: B.record(b"bad", l_read_name=0, **good),
        (B.E_READ_NAME, "nul"): B.record(raw_name=b"bad!", **good),
        B.E_REFERENCE_ID: B.record(b"bad", **dict(good, ref=len(REFS))),
        (B.E_REFERENCE_ID, "mate"): B.record(b"bad", **dict(good, next_ref=-2)),
        B.E_FIELD_LENGTHS: B.record(b"bad", l_seq=5000, **good),
        (B.E_FIELD_LENGTHS, "cigar"): B.record(b"bad", n_cigar=60000, **good),
        B.E_CIGAR_OP: B.record(b"bad", **dict(good, cigar=[(10, "M"), (10, 9)])),
        B.E_QUALITY: B.record(b"bad", **dict(good, qual=bytes([30]) * 19 + b"\x5e")),
        (B.E_QUALITY, "ff"): B.record(b"bad", **dict(good, qual=b"\xff" * 19 + b"\x00")),
    }


@pytest.mark.parametrize("case", list(bad_records()), ids=str)
def test_record_errors(gpu, tmp_path, case):
    from exon_duckdb_amd import abi
    from exon_duckdb_amd.reader import ShardReader
    code = case if isinstance(case, int) else case[0]
    front = B.illumina_pairs(1500, REFS, seed=13)            # 3000 records: more than one chunk in front of the bad one
    recs = front + [bad_records()[case]] + B.illumina_pairs(5, REFS, seed=14)
    path = tmp_path / "bad.bam"
    raw = write_bam(path, REFS, recs)
    want = B.parse_decoded(raw)
    assert want.error == (len(front), code) and len(want.rows) == len(front)
    rows, err, _ = read_all(path)
    assert rows == want.rows                                   # the rows in front of the bad record are delivered
    assert err is not None and err.code == abi.EXG_E_PARSE
    assert f"record {len(front)}" in str(err) and "bad.bam" in str(err), str(err)
    r = ShardReader(str(path), "bam")
    with pytest.raises(Exception) as e:
        r.count()
    assert f"record {len(front)}" in str(e.value)
    r.close()


def test_truncated_stream_bad_crc_not_gzip_not_bam(gpu, tmp_path):
    from exon_duckdb_amd import ExgError, abi
    recs = B.illumina_pairs(200, REFS, seed=15)
    raw = B.header(REFS) + b"".join(recs)
    p = tmp_path / "truncated.bam"
    p.write_bytes(B.bgzf(raw[:-7]))
    rows, err, _ = read_all(p)
    assert rows == B.parse_decoded(raw).rows[:-1] and err is not None and err.code == abi.EXG_E_PARSE
    assert f"record {len(recs) - 1}" in str(err) and "past the end" in str(err)
    comp = bytearray(B.bgzf(raw, level=6))
    first = struct.unpack_from("<H", comp, 16)[0] + 1         # BSIZE of the first member: its CRC is 8 bytes from its end
    comp[first - 8] ^= 0x01
    q = tmp_path / "bad_crc.bam"
    q.write_bytes(bytes(comp))
    rows, err, _ = read_all(q)
    assert err is not None and "record" not in str(err) and ("crc" in str(err).lower() or "checksum" in str(err).lower()), str(err)
    t = tmp_path / "text.bam"
    t.write_bytes(b"@HD\tVN:1.6\nthis is SAM text, not BGZF\n" * 100)
    with pytest.raises(ExgError) as e:
        rows, err, _ = read_all(t)
        if err:
            raise err
    assert "text.bam" in str(e.value)
    g = tmp_path / "gzip_of_text.bam"
    g.write_bytes(B.bgzf(b"hello, world: gzip members, but no BAM inside\n" * 10))
    rows, err, _ = read_all(g)
    assert err is not None and "not a BAM file" in str(err) and "gzip_of_text.bam" in str(err)


# ---------------------------------------------------------------- 7. filters
def test_filters(gpu, illumina, tmp_path):
    from exon_duckdb_amd import table_function as tf
    from exon_duckdb_amd.table_function import F
    path = os.path.join(GOLDEN, "bam/test.bam")
    want = B.parse(path).rows
    rel = tf.connect().table_function(FN, path)
    col = {n: i for i, n in enumerate(B.NAMES)}

    def check(filters, pred, columns=None):
        exp = [r for r in want if pred(r)]
        got = rel.fetchall(columns=columns, filters=filters)
        if columns:
            exp = [tuple(r[col[c]] for c in columns) for r in exp]
        assert got == exp, filters
        assert rel.count(filters=filters) == len(exp), filters
        return len(exp)

    flags = sorted({r[1] for r in want})
    starts = sorted(r[3] for r in want if r[3] is not None)
    lo, hi = starts[len(starts) // 4], starts[3 * len(starts) // 4]
    some_ref = want[len(want) // 2][2]
    assert check({"flag": F.cmp("=", flags[0])}, lambda r: r[1] == flags[0]) > 0
    assert check({"flag": F.cmp("<", flags[len(flags) // 2])}, lambda r: r[1] < flags[len(flags) // 2]) > 0
    assert check({"start": F.and_(F.cmp(">=", lo), F.cmp("<", hi))}, lambda r: r[3] is not None and lo <= r[3] < hi) > 0
    check({"start": F.or_(F.cmp("<", lo), F.cmp(">=", hi))}, lambda r: r[3] is not None and (r[3] < lo or r[3] >= hi))
    check({"end": F.cmp(">=", hi)}, lambda r: r[4] is not None and r[4] >= hi, columns=["name", "end"])
    check({"mapping_quality": F.isnull()}, lambda r: r[5] is None)
    check({"start": F.isnull()}, lambda r: r[3] is None)
    check({"end": F.notnull()}, lambda r: r[4] is not None)
    assert check({"reference": F.cmp("=", some_ref)}, lambda r: r[2] == some_ref) > 0
    check({"mate_reference": F.cmp("!=", some_ref)}, lambda r: r[7] is not None and r[7] != some_ref)
    check({"cigar": F.cmp("=", b"250M")}, lambda r: r[6] == b"250M", columns=["flag"])
    check({"name": F.cmp(">=", want[100][0])}, lambda r: r[0] >= want[100][0])
    check({"sequence": F.cmp("<", b"C")}, lambda r: r[8] < b"C", columns=["sequence", "quality_score"])
    check({"reference": F.cmp("=", some_ref), "flag": F.cmp(">=", 100), "start": F.cmp(">", lo)},
          lambda r: r[2] == some_ref and r[1] >= 100 and r[3] is not None and r[3] > lo)
    # the generated file: NULLs in every nullable column, several device batches
    ipath, iwant = illumina
    os.environ["EXG_DEVICE_BATCH_BYTES"] = str(4 << 20)
    try:
        irel = tf.connect().table_function(FN, str(ipath))
        assert irel.count(filters={"reference": F.isnull()}) == sum(1 for r in iwant if r[2] is None) > 0
        got = irel.fetchall(columns=["name", "start", "mapping_quality"], filters={"mapping_quality": F.cmp("=", b"60"), "start": F.cmp("<", 50_000_000)})
        assert got == [(r[0], r[3], r[5]) for r in iwant if r[5] == b"60" and r[3] is not None and r[3] < 50_000_000]
    finally:
        del os.environ["EXG_DEVICE_BATCH_BYTES"]


# ---------------------------------------------------------------- 8. refusals at the boundary
def test_boundary_errors(gpu, tmp_path):
    from exon_duckdb_amd import ExgError, abi
    from exon_duckdb_amd.reader import ShardReader
    path = os.path.join(GOLDEN, "bam/example1.bam")
    with pytest.raises(ExgError) as e:
        ShardReader(path, "bam", shard_index=1, shard_count=2)
    assert e.value.code == abi.EXG_E_UNSUPPORTED
    with pytest.raises(ExgError) as e:
        ShardReader(path, "sam")
    assert e.value.code == abi.EXG_E_UNSUPPORTED
    from exon_duckdb_amd.arrow import new_reader
    with pytest.raises(Exception) as e:
        new_reader(path, "bam").read_all()
    assert "chunk boundary only" in str(e.value)
    # the planner answers one shard, and shard_count = 0 reads the file as one stripe
    lib = gpu
    a = abi.OpenArgs(path.encode(), b"bam", None, 2048, 0, 0, None, 0, 1, 0, 0)
    n, devs = C.c_uint32(9), (C.c_int * 8)()
    os.environ["EXON_GPU_SHARDS"] = "4"
    try:
        assert lib.exg_plan_shards(C.byref(a), C.byref(n), devs, 8) == 0 and n.value == 1
        r = ShardReader(path, "bam", shard_count=0)
        assert len(r.rows()) == 1
        r.close()
    finally:
        del os.environ["EXON_GPU_SHARDS"]
    # a compression argument that says otherwise changes nothing: a BAM file is BGZF
    r = ShardReader(path, "bam", compression="uncompressed")
    assert r.count() == 1 and r.stats()["input_compression"] == 1
    r.close()


# ---------------------------------------------------------------- 9. bounded memory
def test_memory_stays_bounded(gpu, tmp_path, monkeypatch):
    from exon_duckdb_amd.reader import ShardReader
    cap_mb = 16
    run = B.illumina_pairs(10_000, REFS, seed=17)
    path = tmp_path / "big.bam"
    times = 22
    decoded = B.write_repeated(str(path), B.header(REFS), b"".join(run), times)
    assert decoded >= 8 * (cap_mb << 20)
    one = B.parse_decoded(B.header(REFS) + b"".join(run)).rows
    side = sum(len(v) for r in one for v in (r[0], r[6], r[8], r[9]) if len(v) > 12) * times
    n_rows = len(one) * times
    monkeypatch.delenv("EXG_DEVICE_MEM_CAP_MB", raising=False)
    r = ShardReader(str(path), "bam")
    free = r.digest(per_column=True)
    r.close()
    monkeypatch.setenv("EXG_DEVICE_MEM_CAP_MB", str(cap_mb))
    r = ShardReader(str(path), "bam", expect_chunks=True)
    capped = r.digest(per_column=True)
    st = r.stats()
    r.close()
    print(f"cap {cap_mb} MiB: peak {st['device_bytes_peak'] / 1048576:.2f} MiB, {st['decoded_segments']} segments, {st['device_batches']} batches")
    assert free == capped and capped[0] == n_rows
    assert st["device_bytes_peak"] <= cap_mb << 20, st
    assert st["decoded_segments"] >= 8 and st["device_batches"] >= 8, st
    # what crossed PCIe on the way back: the vectors (7 string_t + 3 INTEGER a row, validity words) and the side buffer —
    # no decoded segment (a host mirror would be the whole decoded stream on top)
    vectors = n_rows * (7 * 16 + 3 * 4)
    assert side + vectors <= st["host_vector_bytes"] <= side + vectors + 5 * 8 * (n_rows // 64 + 2 * st["device_batches"]), st
    r = ShardReader(str(path), "bam", columns=[1])
    assert len(r.rows()) == n_rows
    assert r.stats()["host_vector_bytes"] == 4 * n_rows      # flag alone: four bytes a row and nothing else
    r.close()
    r = ShardReader(str(path), "bam")
    assert r.count() == n_rows and r.stats()["host_vector_bytes"] == 0
    r.close()
