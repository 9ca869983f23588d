"""Pushed-down `filters` on the formats and paths that came behind tests/test_filters_gpu.py, against DuckDB's semantics
(tests/filter_oracle.py) — each of them feeds the row predicate something the paths tested there never do:

  * GTF: `score` is the one flat FLOAT the scan writes as a number with validity words of its own, and the one float column that can
    be negative (-inf, -0, -1e-45); the predicate is ANDed with the bitmap of the lines that are rows (`#` lines leave their slots
    unwritten), and `attributes` is built behind that merged row map;
  * FASTA: `sequence` is the one string column whose strings point into the joined payload, not into the input — through
    ShardReader and through new_reader;
  * BCF: VCF rows made from binary records, over BGZF members that the records straddle;
  * FASTQ through ShardReader (tests/test_filters_gpu.py reads it through new_reader only);
  * the GTF and FASTA files again as compressed copies and as three byte-range shards.

The files are those of tests/filter_format_sites.py: 333 rows each, read with the default device batch and with
EXG_DEVICE_BATCH_BYTES=4096.  The expected rows come from gtf_files.read, oracle.fasta_parse / fastq_parse, and oracle.vcf_parse over
the text bcf_files' renderer makes of the BCF records — never from the library.  tests/test_filters_formats_host.py checks without
a device that the files and the trees are what these tests take them to be."""
import bz2
import ctypes as C
import gzip

import pytest

import filter_format_sites as S
import test_filters_gpu as TF
from filter_oracle import cmp, or_

pytestmark = pytest.mark.gpu

N_ROWS = S.N_ROWS
fastq = TF.fastq                     # the FASTQ file of tests/test_filters_gpu.py, built once for this module


@pytest.fixture(scope="module")
def gtf(gpu, tmp_path_factory):
    site, keep = S.gtf_site(tmp_path_factory.mktemp("filters_gtf") / "edge.gtf")
    assert len(site.rows) == N_ROWS
    site.keep = keep
    return site


@pytest.fixture(scope="module")
def fasta(gpu, oracle, tmp_path_factory):
    site = S.fasta_site(oracle, tmp_path_factory.mktemp("filters_fasta") / "edge.fasta")
    assert len(site.rows) == N_ROWS
    return site


@pytest.fixture(scope="module")
def bcf(gpu, oracle, tmp_path_factory):
    return S.bcf_site(oracle, tmp_path_factory.mktemp("filters_bcf") / "edge.bcf")


@pytest.fixture(params=["default", "small"])
def batch(request, monkeypatch):
    if request.param == "small":
        monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", "4096")
    else:
        monkeypatch.delenv("EXG_DEVICE_BATCH_BYTES", raising=False)
    return request.param


def trees(site, key):
    n, seed = S.TREES[key]
    return TF.trees_for(site, n, seed)


# ---- 1. GTF --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col", S.GTF_FLAT)
def test_gtf_every_leaf(gtf, batch, col):
    TF.check_leaves(gtf, col, gtf.shard_rows)


def test_gtf_random_trees(gtf, batch):
    TF.check_trees(gtf, trees(gtf, "gtf"), gtf.shard_rows)


def batches_of(site):
    """(device batches scanned, row index of the first row of every batch that gave rows), from an unfiltered read"""
    from exon_duckdb_amd.reader import ShardReader
    from exon_duckdb_amd.table_function import Chunk
    r = ShardReader(site.path, site.fmt, columns=[1])
    starts, n, last = [], 0, None
    try:
        while True:
            ch = Chunk()
            assert r._l.exg_next_chunk(r._r, C.byref(ch)) == 0
            if ch.n_rows == 0:
                return r.stats()["device_batches"], starts
            if ch.batch_no != last:
                starts.append(n)
                last = ch.batch_no
            n += int(ch.n_rows)
            r._l.exg_release_chunk(r._r, C.byref(ch))
    finally:
        r.close()


def test_gtf_selection_shapes(gtf, batch):
    """the shapes of test_selection_shapes, and the rows around the lines that are no rows: k_row_map and the gathers behind a row
    map that merges the predicate with d_keep, exg_gtf_attributes behind it"""
    n_batches, starts = batches_of(gtf)
    behind_long = S.gtf_row_of_line(gtf.keep, S.GTF_LONG_RUN[-1] + 1)
    if batch == "small":
        assert len(starts) >= 3 and n_batches >= len(starts) + 2, (n_batches, starts)      # batches without a row: all comments
        assert behind_long in starts, (behind_long, starts)                                # the long run ends a batch, or fills it
    sel = lambda k: S.gtf_row_selector(gtf, k)
    behind_70, before_70 = S.gtf_row_of_line(gtf.keep, S.GTF_RUN70[-1] + 1), S.gtf_row_of_line(gtf.keep, S.GTF_RUN70[0] - 1)
    assert behind_70 == before_70 + 1
    shapes = {
        "no row": (cmp("start", "<", "0"), 0),
        "every row": (cmp("start", ">=", "1"), N_ROWS),
        "the last row": (sel(N_ROWS - 1), 1),
        "the first row of the last batch": (sel(starts[-1]), 1),
        "the first row": (sel(0), 1),
        "two rows with 199 and 132 rejected in a run": (or_(sel(0), sel(200)), 2),
        "the first and the last row": (or_(sel(0), sel(N_ROWS - 1)), 2),
        "the row behind the 70 comment lines": (sel(behind_70), 1),
        "the row in front of the 70 comment lines": (sel(before_70), 1),
        "only rows of the batch behind the batches that are all comments": (or_(sel(behind_long), sel(behind_long + 1), sel(behind_long + 2)), 3),
    }
    for name, (t, size) in shapes.items():
        want = gtf.want(t)
        assert len(want) == size, name
        assert gtf.shard_rows(TF.sql(t)) == want, name
        assert gtf.shard_count(TF.sql(t)) == len(want), name
        assert gtf.shard_rows(TF.sql(t), columns=["attributes"]) == gtf.want(t, ["attributes"]), name


# ---- 2. FASTA ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col", S.FA_FLAT)
def test_fasta_every_leaf(fasta, batch, col):
    TF.check_leaves(fasta, col, fasta.shard_rows)


@pytest.mark.parametrize("col", S.FA_FLAT)
def test_fasta_every_leaf_new_reader(fasta, batch, col):
    TF.check_leaves(fasta, col, fasta.arrow_rows)


def test_fasta_random_trees(fasta, batch):
    TF.check_trees(fasta, trees(fasta, "fasta"), fasta.shard_rows)


def test_fasta_random_trees_new_reader(fasta, batch):
    TF.check_trees(fasta, trees(fasta, "fasta new_reader"), fasta.arrow_rows, shard=False)


# ---- 3. BCF --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col", TF.VCF_FLAT)
def test_bcf_every_leaf(bcf, batch, col):
    TF.check_leaves(bcf, col, bcf.shard_rows)


def test_bcf_random_trees(bcf, batch):
    TF.check_trees(bcf, trees(bcf, "bcf"), bcf.shard_rows)


# ---- 4. FASTQ through ShardReader ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col", TF.FQ_FLAT)
def test_fastq_every_leaf_shard(fastq, batch, col):
    TF.check_leaves(fastq, col, fastq.shard_rows)


def test_fastq_random_trees_shard(fastq, batch):
    TF.check_trees(fastq, trees(fastq, "fastq shard"), fastq.shard_rows, shard=True)


# ---- 5. other sources and shards (the small batch only) --------------------------------------------------------------------------------
def zst(data):
    from zstd_util import compress
    return compress(data, 3, True)


COPIES = {"gtf zst": ("edge.gtf.zst", zst, None), "gtf gz": ("edge.one.gtf.gz", lambda d: gzip.compress(d, 6, mtime=0), None),
          "fasta gz": ("edge.fasta.gz", lambda d: gzip.compress(d, 6, mtime=0), None), "fasta bz2": ("edge.fasta.bz2", bz2.compress, "bzip2")}


@pytest.mark.parametrize("key", sorted(COPIES))
def test_filters_on_compressed_copies(gpu, oracle, tmp_path, monkeypatch, key):
    """the decoded segments of a compressed input are batches cut elsewhere than a text file's: rows and count through ShardReader"""
    name, pack, compression = COPIES[key]
    data = S.gtf_bytes() if key.startswith("gtf") else S.fasta_bytes()
    p = tmp_path / name
    p.write_bytes(pack(data))
    site = S.gtf_site(p, data)[0] if key.startswith("gtf") else S.fasta_site(oracle, p, data)
    monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", "4096")
    kw = {"compression": compression} if compression else {}
    for t in trees(site, key):
        want = site.want(t)
        assert site.shard_rows(TF.sql(t), **kw) == want, TF.sql(t)
        assert site.shard_count(TF.sql(t), **kw) == len(want), TF.sql(t)


@pytest.mark.parametrize("fmt", ["gtf", "fasta"])
def test_filters_on_three_shards(request, monkeypatch, fmt):
    """three byte ranges of the file, each under the filter: their rows in order are the file's, their counts add up"""
    site = request.getfixturevalue(fmt)
    monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", "4096")
    monkeypatch.setenv("EXG_SHARD_HALO", "512")                 # (the halo grows until it holds the record across the cut)
    parts = [len(site.shard_rows(b"", shard_index=i, shard_count=3)) for i in range(3)]
    assert min(parts) > 0 and sum(parts) == N_ROWS, parts       # every shard holds rows
    for t in trees(site, fmt + " shards"):
        want, got, n = site.want(t), [], 0
        for i in range(3):
            got += site.shard_rows(TF.sql(t), shard_index=i, shard_count=3)
            n += site.shard_count(TF.sql(t), shard_index=i, shard_count=3)
        assert got == want and n == len(want), TF.sql(t)


# ---- the columns that stay refused --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,text", [("gtf", "attributes = 'x'"), ("bcf", "info = 'x'")])
def test_nested_columns_stay_refused(request, fmt, text):
    from exon_duckdb_amd import ExgError
    from exon_duckdb_amd.reader import ShardReader
    site = request.getfixturevalue(fmt)
    with pytest.raises(ExgError):
        ShardReader(site.path, fmt, filters=text)
    assert site.shard_count(b"pos>=0" if fmt == "bcf" else b"start>=1") == N_ROWS        # and the next open is fine
