"""Differential fuzzing of the BED, SAM, BAM and BCF scans: the inputs of tests/fuzz_records.py (byte noise, near-miss fields,
records rebuilt with one or two faults) on the device against each format's Python reference — the row count, which record fails
with which code and where, where the scan stops, and every row (BCF: every line) in front of the error.  BED and SAM through
both drivers, stored and EXG_F_NO_STORE (test_bed_gpu.check / test_sam_gpu.check); BAM stored and EXG_F_NO_STORE; BCF with
the guard behind the text.  Then the binary formats through the reader, in 5 000-byte BGZF members and 64 KiB device batches.

Every failure names (format, seed, mutant index): fuzz_records.case(format, seed)[mutant] rebuilds the bytes without a GPU
(tests/test_fuzz_records_host.py holds the inputs themselves to account)."""
import ctypes as C

import pytest

import bam_files as BAM
import bcf_files as BCF
import fuzz_records as FZ
import test_bam_gpu as T_BAM
import test_bcf_gpu as T_BCF
import test_bed_gpu as T_BED
import test_sam_gpu as T_SAM

pytestmark = pytest.mark.gpu

READER_SEEDS = range(8)


def tagged(tag, fn, *args):
    try:
        return fn(*args)
    except AssertionError as e:
        raise AssertionError(f"{tag}: {e}") from e


# ---------------------------------------------------------------- BED, SAM
@pytest.mark.parametrize("seed", FZ.SEEDS)
def test_bed_fuzz(gpu, seed):
    for m, data in enumerate(FZ.case("bed", seed)):
        tagged(("bed", seed, m), T_BED.check, data)


@pytest.mark.parametrize("seed", FZ.SEEDS)
def test_sam_fuzz(gpu, seed):
    for m, data in enumerate(FZ.case("sam", seed)):
        tagged(("sam", seed, m), T_SAM.check, data)


@pytest.mark.parametrize("fmt,k", [(f, k) for f in ("bed", "sam") for k in range(4)])
def test_mutations_at_the_super_tile_boundary(gpu, fmt, k):
    check = T_BED.check if fmt == "bed" else T_SAM.check
    for m, data in enumerate(FZ.super_tile_case(fmt, k)):
        tagged((fmt, "super-tile", k, m), check, data)


# ---------------------------------------------------------------- BAM
def check_bam(stream):
    from exon_duckdb_amd import abi, device
    want = FZ.reference("bam", stream)
    scan = device.BamScan(len(stream), FZ.BAM_REFS)
    d_in = device.upload(stream)
    scan.launch(d_in, flags=abi.EXG_F_EOF)
    res = scan.fetch()
    got = (res.n_records, res.error_code, res.error_record if res.error_code else None, res.consumed_bytes)
    exp = (len(want.rows), want.code, want.error[0] if want.error else None, want.consumed)
    assert got == exp, f"(n_records, error_code, error_record, consumed_bytes) {got} != {exp}"
    assert not res.flags & abi.EXG_RF_CAPACITY
    if want.error:
        assert res.error_offset == want.error[2]
    rows = scan.rows(res.n_records, res.side_bytes)
    if rows != want.rows:
        k = next(i for i, (g, w) in enumerate(zip(rows, want.rows)) if g != w)
        raise AssertionError(f"row {k}: {rows[k]} != {want.rows[k]}")
    scan.launch(d_in, flags=abi.EXG_F_EOF | abi.EXG_F_NO_STORE)
    res2 = scan.fetch()
    got2 = (res2.n_records, res2.error_code, res2.error_record if res2.error_code else None, res2.consumed_bytes)
    assert got2 == exp and res2.side_bytes == 0, f"EXG_F_NO_STORE: {got2} != {exp}, side_bytes {res2.side_bytes}"
    return want


@pytest.mark.parametrize("seed", FZ.SEEDS)
def test_bam_fuzz(gpu, seed):
    for m, stream in enumerate(FZ.case("bam", seed)):
        tagged(("bam", seed, m), check_bam, stream)


# ---------------------------------------------------------------- BCF
def check_bcf(records):
    want = FZ.reference("bcf", records)
    res, out = T_BCF.transcode(records, FZ.bcf_text())
    got = (res.n_records, res.error_code, res.consumed_bytes, res.flags)
    exp = (len(want.rows), want.code, want.consumed, 0)
    assert got == exp, f"(n_records, error_code, consumed_bytes, flags) {got} != {exp} (error_record {res.error_record})"
    if want.error:
        assert (res.error_record, res.error_code, res.error_offset) == want.error
    assert res.text_bytes == res.text_bytes_needed
    diff = BCF.text_equal(out[:res.text_bytes], want.extra.text)
    assert diff is None, diff
    assert out[res.text_bytes:res.text_bytes + 64] == b"\xA5" * 64, "bytes written behind the text"
    return want


@pytest.mark.parametrize("seed", FZ.SEEDS)
def test_bcf_fuzz(gpu, seed):
    for m, records in enumerate(FZ.case("bcf", seed)):
        tagged(("bcf", seed, m), check_bcf, records)


# ---------------------------------------------------------------- through the reader
@pytest.fixture
def small_batches(monkeypatch):
    monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", "65536")


def reader_bam(tmp_path, m, stream):
    want = FZ.reference("bam", stream)
    path = tmp_path / f"fuzz{m}.bam"
    path.write_bytes(BAM.bgzf(FZ.BAM_HEADER + stream, member_bytes=5000))
    rows, err, _ = T_BAM.read_all(path)
    assert len(rows) == len(want.rows) and rows == want.rows, (len(rows), len(want.rows))      # the rows in front of the error are delivered
    if want.error is None:
        assert err is None, str(err)
    else:
        assert err is not None and f"record {want.error[0]}" in str(err) and path.name in str(err), str(err)


@pytest.mark.parametrize("seed", READER_SEEDS)
def test_reader_bam_fuzz(gpu, tmp_path, small_batches, seed):
    for m, stream in enumerate(FZ.case("bam", seed)):
        tagged(("bam", seed, m), reader_bam, tmp_path, m, stream)


def vcf_chunks(path):
    """test_bcf_gpu.read_chunks for a VCF file: (rows, error or None)"""
    from exon_duckdb_amd import ExgError
    from exon_duckdb_amd.reader import ShardReader
    from exon_duckdb_amd.table_function import Chunk, decode_vector
    r = ShardReader(str(path), "vcf")
    rows, err = [], None
    while True:
        ch = Chunk()
        rc = r._l.exg_next_chunk(r._r, C.byref(ch))
        if rc != 0:
            err = ExgError(rc, (r._l.exg_reader_error(r._r) or b"").decode("utf-8", "replace"))
            break
        if ch.n_rows == 0:
            break
        rows.extend(zip(*[decode_vector(ch.vectors[k].contents, r.trees[k]) for k in range(len(r.names))]))
        r._l.exg_release_chunk(r._r, C.byref(ch))
    r.close()
    return rows, err


def reader_bcf(tmp_path, m, records):
    """the rows are read_vcf's of the lines the renderer gives.  Where those lines are not VCF (a mutated byte made a tab, a letter
    in an integer field), the VCF stage stops both reads at the same row"""
    text = FZ.bcf_text()
    want = FZ.reference("bcf", records)
    path = tmp_path / f"fuzz{m}.bcf"
    path.write_bytes(BCF.bgzf_file(text, [records], member_bytes=5000))
    rows, err = T_BCF.read_chunks(path)
    (tmp_path / f"same{m}.vcf").write_bytes(text + want.extra.text)
    vrows, verr = vcf_chunks(tmp_path / f"same{m}.vcf")
    T_BCF.same_rows(rows, vrows)
    if verr is not None:
        assert err is not None and path.name in str(err), str(err)
        return
    assert len(rows) == len(want.rows)
    if want.error is None:
        assert err is None, str(err)
    else:
        assert err is not None and f"record {want.error[0]}" in str(err) and path.name in str(err), str(err)


@pytest.mark.parametrize("seed", READER_SEEDS)
def test_reader_bcf_fuzz(gpu, tmp_path, small_batches, seed):
    for m, records in enumerate(FZ.case("bcf", seed)):
        tagged(("bcf", seed, m), reader_bcf, tmp_path, m, records)
