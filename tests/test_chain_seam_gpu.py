"""The chain stitch across its 2048-tile seam (exg_chain.hpp: k_stitch stages the tile table through LDS 2048 tiles — 64 MiB of
input — at a time).  One launch here covers more than 2048 tiles of 32 KiB, so the stitch reloads its table, rebases its tile
index, leaves the 64-tiles-a-step path near the end of what it loaded, and skips a chunk that one record jumps whole.  The
streams are mostly long filler records (aux bytes no column reads), so the rows number in the hundreds and every row is
compared with the Python reader — computed on the pieces: records are position independent.

One uploaded buffer serves several seam positions: the first filler's 38-byte head is rewritten in place at offset j and the
scan is launched from there, which moves the seam to byte j + SEAM of the buffer."""
import struct

import pytest

import bam_files as B
import bcf_files as BCF
import test_bam_gpu as T_BAM
import test_bcf_gpu as T_BCF

pytestmark = pytest.mark.gpu

TILE = 32768
SEAM = 2048 * TILE
REFS = T_BAM.REFS
PIECE = 8 << 20


def filler(size):
    """a record of exactly `size` bytes whose aux field is the bulk: one row, no side bytes"""
    assert size >= 38
    return B.record(b"p", 4, -1, -1, 255, (), -1, -1, 0, b"", None, b"\x55" * (size - 38))


def rows_of(records):
    p = B.parse_decoded(B.header(REFS) + records)
    assert p.error is None
    return p.rows


FILL_ROW = rows_of(filler(100))[0]


class Stream:
    """record bytes and the rows they stand for, grown piece by piece"""

    def __init__(self):
        self.parts, self.rows, self.size = [], [], 0

    def add(self, records, rows):
        self.parts.append(records)
        self.rows += rows
        self.size += len(records)
        return self

    def fill_to(self, target):
        while self.size < target:
            gap = target - self.size
            size = gap if gap <= PIECE + 64 else PIECE
            self.add(filler(size), [FILL_ROW])
        assert self.size == target
        return self

    def bytes(self):
        return b"".join(self.parts)


@pytest.fixture(scope="module")
def pieces():
    """short reads, parsed once: a block of 500 and one of 200, a single record and four more, and the decoy record whose read name is a
    byte-exact copy of two plausible records (test_bam_gpu.adversarial_stream)"""
    recs = B.illumina_pairs(353, REFS, seed=41)
    big, small, r, more = b"".join(recs[:500]), b"".join(recs[500:700]), recs[700], b"".join(recs[701:705])
    fake = B.record(b"f", 0, 0, 5, 7, (), 0, 5) + B.record(b"g", 0, 1, 6, 8, (), 1, 6)
    decoy = B.record(fake[:-1], 0, 0, 10, 20, [(40, "M")], 0, 10, 0, b"ACGT" * 10, bytes([30]) * 40)
    bad = B.record(b"bad_reference", 0, len(REFS), 10, 20, [(40, "M")], 0, 10, 0, b"ACGT" * 10, bytes([30]) * 40, b"\x55" * 100)
    assert decoy[72:74] == b"f\0" and len(bad) > 150       # (the copy begins 36 bytes into the record)
    return dict(big=(big, rows_of(big)), small=(small, rows_of(small)), r=(r, rows_of(r)), more=(more, rows_of(more)), decoy=(decoy, rows_of(decoy)), bad=bad)


class Scanned:
    """a stream on the device, scanned from byte j of the buffer (the first filler's head is rewritten there)"""

    def __init__(self, stream, capacity):
        from exon_duckdb_amd import device
        self.data = stream.bytes()
        self.first = len(stream.parts[0])
        assert self.data[:38] == filler(self.first)[:38]
        self.d_in = device.upload(self.data)
        self.scan = device.BamScan(len(self.data), REFS, capacity_records=capacity, side_capacity=4 << 20)

    def launch(self, j=0, n_bytes=None, flags=None):
        import torch
        from exon_duckdb_amd import abi
        head = bytearray(struct.pack("<I", self.first - j - 4) + self.data[4:38])      # filler(self.first - j)[:38]
        self.d_in[j:j + 38].copy_(torch.frombuffer(head, dtype=torch.uint8))
        n = (len(self.data) - j) if n_bytes is None else n_bytes
        self.scan.launch(self.d_in.data_ptr() + j, n_bytes=n, flags=abi.EXG_F_EOF if flags is None else flags)
        res = self.scan.fetch()
        assert res.tiles == n // TILE + 1 and not res.flags & abi.EXG_RF_CAPACITY, (res.tiles, n // TILE + 1, res.flags)
        return res

    def rows(self, res):
        return self.scan.rows(res.n_records, res.side_bytes)


def same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    if got != want:
        k = next(i for i, (g, w) in enumerate(zip(got, want)) if g != w)
        raise AssertionError((what, k, got[k], want[k]))


# ---------------------------------------------------------------- BAM: cases 1, 2, 3 on one buffer
@pytest.fixture(scope="module")
def around_the_seam(gpu, pieces):
    """[fillers][200 reads ending at SEAM][r][four reads][decoy][500 reads][fillers to tile 2100][200 reads].  The four reads keep
    the decoy out of the way of the other cases: a record in front of the decoy record is no plausible record start (its successor's
    name is binary), and a tile that begins inside r finds the read behind it"""
    s = Stream().fill_to(SEAM - len(pieces["small"][0]))
    s.add(*pieces["small"])
    assert s.size == SEAM
    s.add(*pieces["r"]).add(*pieces["more"]).add(*pieces["decoy"]).add(*pieces["big"])
    s.fill_to(2100 * TILE + 999).add(*pieces["small"])
    return Scanned(s, len(s.rows) + 16), s.rows


def test_a_record_starts_exactly_at_the_seam(around_the_seam):
    sc, want = around_the_seam
    res = sc.launch(0)
    print(f"case 1: tiles {res.tiles} rewalked {res.tiles_rewalked} records {res.n_records}")
    assert (res.error_code, res.n_records, res.consumed_bytes) == (0, len(want), len(sc.data))
    assert res.tiles > 2048 and res.tiles_rewalked <= 4
    same(sc.rows(res), want, "a record at SEAM")


@pytest.mark.parametrize("first", range(0, 36, 6))
def test_a_record_straddles_the_seam(around_the_seam, first):
    """each of the record's first 36 bytes in turn is the last byte in front of the seam"""
    sc, want = around_the_seam
    for k in range(first, first + 6):
        j = k + 1                                                  # the seam at buffer byte SEAM + j: the record's byte k = j - 1 is the last in front
        res = sc.launch(j)
        assert (res.error_code, res.n_records, res.consumed_bytes) == (0, len(want), len(sc.data) - j), (k, res.error_code, res.error_record)
        assert res.tiles > 2048 and res.tiles_rewalked <= 4
        same(sc.rows(res), want, f"byte {k} of the record is the last in front of the seam")


def test_a_decoy_at_the_seam_is_rewalked_as_the_first_tile_of_the_second_chunk(around_the_seam, pieces):
    sc, want = around_the_seam
    j = len(pieces["r"][0]) + len(pieces["more"][0]) + 36                              # the copy inside the decoy's read name begins at buffer byte SEAM + j
    assert sc.data[SEAM + j:SEAM + j + 40] == pieces["decoy"][0][36:76]
    base = sc.launch(0).tiles_rewalked
    res = sc.launch(j)
    print(f"case 3: tiles {res.tiles} rewalked {res.tiles_rewalked} (a record at the seam: {base})")
    assert (res.error_code, res.n_records, res.consumed_bytes) == (0, len(want), len(sc.data) - j)
    assert res.tiles > 2048 and res.tiles_rewalked >= 1 and res.tiles_rewalked > base
    same(sc.rows(res), want, "a decoy at SEAM")


# ---------------------------------------------------------------- case 4: one record longer than a chunk
def test_one_record_jumps_a_whole_chunk(gpu, pieces):
    s = Stream().fill_to(SEAM - (1 << 20) - len(pieces["small"][0])).add(*pieces["small"])
    s.add(filler(SEAM + (2 << 20) + 17), [FILL_ROW])            # begins in chunk 0, ends in chunk 2
    assert s.size // TILE >= 2 * 2048
    s.add(*pieces["big"]).fill_to(s.size + 3 * TILE + 5).add(*pieces["small"])
    sc = Scanned(s, len(s.rows) + 16)
    res = sc.launch(0)
    print(f"case 4: tiles {res.tiles} rewalked {res.tiles_rewalked} records {res.n_records}")
    assert (res.error_code, res.n_records, res.consumed_bytes) == (0, len(s.rows), len(sc.data))
    assert res.tiles > 2 * 2048 and res.tiles_rewalked <= 4
    same(sc.rows(res), s.rows, "records behind a jumped chunk")


# ---------------------------------------------------------------- cases 5 and 6: the input ends at the seam; an error behind it
def test_input_ends_at_the_seam_tail_and_error_behind_it(gpu, pieces):
    from exon_duckdb_amd import abi
    s = Stream().fill_to(SEAM - len(pieces["small"][0])).add(*pieces["small"])
    front = list(s.rows)
    s.add(pieces["bad"], []).add(*pieces["small"])
    sc = Scanned(s, len(front) + 300)
    # n == SEAM: 2049 tiles, the last one empty, the chain ends at the seam
    res = sc.launch(0, n_bytes=SEAM)
    print(f"case 5: tiles {res.tiles} rewalked {res.tiles_rewalked} records {res.n_records}")
    assert res.tiles == 2049 and (res.error_code, res.n_records, res.consumed_bytes) == (0, len(front), SEAM)
    same(sc.rows(res), front, "n == SEAM")
    # the same length, begun 100 bytes later: the last record is cut by the end of the input
    res = sc.launch(100, n_bytes=SEAM, flags=0)
    assert res.tiles == 2049 and (res.error_code, res.n_records, res.consumed_bytes) == (0, len(front), SEAM - 100)
    same(sc.rows(res), front, "a tail at n == SEAM")
    res = sc.launch(100, n_bytes=SEAM)
    assert (res.error_code, res.error_record, res.n_records, res.consumed_bytes) == (abi.EXG_PE_BAM_TRUNCATED, len(front), len(front), SEAM - 100)
    # case 6: the first record behind the seam is in error
    res = sc.launch(0)
    print(f"case 6: tiles {res.tiles} rewalked {res.tiles_rewalked} error {res.error_code} at record {res.error_record}")
    assert (res.error_code, res.error_record, res.error_offset, res.n_records, res.consumed_bytes) == (abi.EXG_PE_BAM_REFERENCE_ID, len(front), SEAM, len(front), SEAM)
    same(sc.rows(res), front, "the rows in front of an error behind SEAM")


# ---------------------------------------------------------------- BCF: k_count over every record behind the seam
def bcf_block(text, n, seed):
    """records without floats: the device's text is the renderer's byte for byte, so the lengths are too"""
    k = lambda name: T_BCF.K(text, name)
    return [BCF.record(chrom=(i + seed) % 3, pos=1000 * seed + i, id_=b"rs%d" % (i * seed), alleles=(b"A", b"CT", b"<DEL>")[:1 + i % 3], filters=[0] if i % 2 else None,
                       info=[(k("DP"), BCF.ints([i * 7 % 5000])), (k("DB"), BCF.flag()), (k("STR"), BCF.chars(b"tandem")),
                             (k("BIG"), BCF.ints(list(range(-i, 40 - i))))][:1 + i % 4]) for i in range(n)]


def bcf_filler(text, size):
    """a record of exactly `size` bytes: an int8 vector that begins with end-of-vector — `BIG=.` however long"""
    key = T_BCF.K(text, "BIG")
    make = lambda n: BCF.record(info=[(key, BCF.raw_value(1, n, b"\x81" + b"\x01" * (n - 1), long_form=True))])
    n = size - (len(make(40000)) - 40000)
    assert n > 32767
    rec = make(n)
    assert len(rec) == size
    return rec


def bcf_stream(text, at_seam):
    """[200 records][fillers to the seam][at_seam(size so far) -> records][200 records]; -> (bytes, rendered text)"""
    strings, contigs, n_samples = BCF.dictionaries(text)
    render = lambda recs: BCF.Rendered(b"".join(recs), strings, contigs, n_samples)
    parts, texts, size = [], [], 0

    def add(recs):
        nonlocal size
        r = render(recs)
        assert r.error is None
        parts.extend(recs)
        texts.append(r.text)
        size += sum(map(len, recs))
    add(bcf_block(text, 200, 1))
    lead = at_seam(None)
    while size < SEAM - lead:
        gap = SEAM - lead - size
        add([bcf_filler(text, gap if gap <= PIECE + 64000 else PIECE)])
    add(at_seam(size))
    add(bcf_block(text, 200, 2))
    return b"".join(parts), b"".join(texts)


@pytest.mark.parametrize("case", ["a record at the seam", "a decoy at the seam"])
def test_bcf_counts_every_record_behind_the_seam(gpu, case):
    from exon_duckdb_amd import abi
    text = T_BCF.header()
    k = lambda name: T_BCF.K(text, name)
    head = BCF.record(chrom=1, pos=12345, alleles=(b"A", b"C"), info=[(k("DP"), BCF.ints([9]))])

    def at_seam(size):
        if case == "a record at the seam":
            return 0 if size is None else bcf_block(text, 5, 3)
        if size is None:
            return 100                                             # the decoy's record begins 100 bytes in front of the seam
        rec = BCF.record(id_=b"i" * 200 + head + head + b"j" * 50)
        assert size + 100 == SEAM and len(rec) > 300
        return [rec]
    raw, want = bcf_stream(text, at_seam)
    assert len(raw) // TILE + 1 > 2048
    res, out = T_BCF.transcode(raw, text, capacity=0)
    print(f"bcf, {case}: rewalked {res.tiles_rewalked} text {res.text_bytes_needed}")
    assert (res.flags, res.n_records, res.error_code, res.text_bytes) == (abi.EXG_RF_CAPACITY, 0, 0, 0)
    assert res.text_bytes_needed == len(want) and res.consumed_bytes == 0
    if case == "a decoy at the seam":
        assert res.tiles_rewalked >= 1
    if case == "a record at the seam":                             # and once with room: the last 200 records lie behind the seam
        res, out = T_BCF.transcode(raw, text, capacity=len(want) + 64)
        assert (res.flags, res.error_code, res.consumed_bytes, res.text_bytes) == (0, 0, len(raw), len(want))
        assert res.n_records == want.count(b"\n")
        assert out[:res.text_bytes] == want and out[res.text_bytes:res.text_bytes + 64] == b"\xA5" * 64


# ---------------------------------------------------------------- the reader: a batch that crosses the seam against batches that never do
def test_reader_default_batch_crosses_the_seam(gpu, tmp_path, monkeypatch):
    import random
    from exon_duckdb_amd.reader import ShardReader
    rng = random.Random(6)

    def read(i, n=5000):
        return B.record(b"long_read_%d" % i, 0, i % 20, 1000 * i, 60, [(n // 2, "M"), (5, "D"), (n - n // 2, "M")], -1, -1, 0,
                        rng.randbytes(n).translate(B._TO_BASES), rng.randbytes(n).translate(B._TO_QUAL), B.aux_z(b"RG", b"nanopore"))
    run = b"".join(read(i) for i in range(40))
    times = (72 << 20) // len(run) + 1
    path = tmp_path / "seam.bam"
    decoded = B.write_repeated(str(path), B.header(REFS), run, times)
    assert decoded > SEAM + (4 << 20)
    digests, stats = [], []
    for batch in (None, 8388608):
        if batch:
            monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", str(batch))
        else:
            monkeypatch.delenv("EXG_DEVICE_BATCH_BYTES", raising=False)
        r = ShardReader(str(path), "bam")
        digests.append(r.digest(per_column=True))
        stats.append(r.stats())
        r.close()
    print(f"default: {stats[0]['device_batches']} batches, {stats[0]['bam_tiles']} tiles; 8 MiB: {stats[1]['device_batches']} batches")
    assert digests[0] == digests[1] and digests[0][0] == 40 * times
    assert decoded // stats[0]["device_batches"] > SEAM, stats[0]      # some batch of the default read is longer than a chunk of the stitch
    assert stats[1]["device_batches"] >= 8
