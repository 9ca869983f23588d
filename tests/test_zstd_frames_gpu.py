"""The device zstd decoder on frames written field by field (tests/zstd_frames.py): every catalogue frame through
exg_zstd_decode against libzstd and the RFC's own expectation, invalid frames refused, catalogue frames in one stream
(entropy state and repeat offsets reset at every frame), generator seeds of several MiB (state that crosses the decoder's
chunks), FASTQ seeds through the reader in small rounds and through new_reader, windows of 64 and 128 MiB (offset codes
24 - 27) and one step above the limit, and the fetching index walks in a child process."""
import os
import subprocess
import sys

import pytest

import zstd_frames as zf
from test_streaming_gpu import _oracle_digest
from test_zstd_gpu import zstd_decode
from zstd_util import decompress_stream, skippable

pytestmark = pytest.mark.gpu

FQ_COLS = ["name", "description", "sequence", "quality_scores"]


def _check_valid(gpu, name, spec):
    comp = zf.encode(spec)
    want = zf.expected_output(spec)
    ok, lz = decompress_stream(comp)
    assert ok and lz == want, name
    rc, out = zstd_decode(gpu, comp)
    assert rc == 0, (name, out)
    assert out == want, (name, len(out), len(want), next((i for i, (a, b) in enumerate(zip(out, want)) if a != b), None))


def test_catalogue_through_exg_zstd_decode(gpu):
    for name, spec in sorted(zf.catalogue().items()):
        _check_valid(gpu, name, spec)
    for name, (spec, clause, _) in sorted(zf.invalid().items()):
        rc, msg = zstd_decode(gpu, zf.encode(spec))
        assert rc != 0 and msg, (name, clause)


def test_multi_frame_streams(gpu):
    cat = zf.catalogue()
    frames = [cat[n] for n in ("rep_offsets", "treeless_chain", "repeat_tables_far", "fse_accuracy_edges", "chunk_crossing",
                               "huf_weights_fse", "lits_huf_4streams_tiny", "blocks_between")]
    frames = [x for f in frames for x in (f if isinstance(f, list) else [f])] + cat["headers"] + cat["match_to_frame_start"]
    parts = []
    for i, f in enumerate(frames):
        parts.append(f)
        if i % 3 == 1:
            parts.append(skippable(b"s" * i, i % 16))
    _check_valid(gpu, "catalogue stream", parts)
    # a frame whose first block repeats a table or a tree, right behind a frame that defined them: refused (the state is reset)
    for bad in ("bad_repeat_table_first", "bad_treeless_first", "bad_rep3_zero"):
        spec = zf.invalid()[bad][0]
        rc, msg = zstd_decode(gpu, zf.encode([cat["repeat_tables_far"], cat["treeless_chain"], spec]))
        assert rc != 0 and msg, bad


def test_generator_seeds_through_exg_zstd_decode(gpu):
    for seed in range(100, 106):
        f = zf.random_frame(seed, 3 << 20, fastq=seed % 2 == 0)
        forms = zf.forms(f)
        assert len(zf.expected_output(f)) >= 3 << 20
        _check_valid(gpu, seed, f)
        assert "of:rep_at_block_start" in forms and ("tbl:rep_fse" in forms or "tbl:rep_pre" in forms), (seed, sorted(forms))


@pytest.fixture(scope="module")
def fastq_seed_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("zfq")
    out = []
    for seed in (201, 202):
        f = zf.random_frame(seed, 4 << 20, fastq=True)
        text = zf.expected_output(f)
        zp, fp = d / ("s%d.fastq.zst" % seed), d / ("s%d.fastq" % seed)
        zp.write_bytes(zf.encode(f))
        fp.write_bytes(text)
        out.append((zp, fp, text))
    return out


@pytest.mark.parametrize("round_out,prefix_index", [(128 << 10, False), (1 << 20, False), (1 << 20, True)], ids=["131072", "1048576", "1048576-prefix-index"])
def test_fastq_seeds_through_the_reader(gpu, oracle, fastq_seed_files, monkeypatch, round_out, prefix_index):
    from exon_duckdb_amd.reader import ShardReader
    monkeypatch.delenv("EXG_DEVICE_MEM_CAP_MB", raising=False)
    monkeypatch.setenv("EXG_STREAM_ROUND_OUT", str(round_out))
    if prefix_index:  # the first round on a prefix of the index and a guessed window (by itself: files of 256 MiB and more)
        monkeypatch.setenv("EXG_ZSTD_INDEX_OVERLAP_MIN", "0")
    for zp, _, text in fastq_seed_files:
        want = _oracle_digest(oracle.fastq_parse(text, want_string_t=False), FQ_COLS)
        r = ShardReader(str(zp), "fastq")
        got = r.digest()
        st = r.stats()
        r.close()
        assert got == want, zp.name
        assert st["decoded_segments"] >= (len(text) // round_out) // 2, st


def test_an_error_found_when_a_round_completes_is_reported_as_the_decoders(gpu, tmp_path):
    """a match that reaches in front of its frame is found when the round's execution is waited for: the reader says what the
    decoder said (the producer once took that error's code for "the consumer closed the stream", and the stream ended
    without its last segment)"""
    from exon_duckdb_amd import ExgError
    from exon_duckdb_amd.reader import ShardReader
    p = tmp_path / "bad.fastq.zst"
    p.write_bytes(zf.encode(zf.invalid()["bad_offset_past_start"][0]))
    with pytest.raises(ExgError, match="Data corruption detected"):
        ShardReader(str(p), "fastq").count()


def test_fastq_seed_through_new_reader(gpu, fastq_seed_files):
    from exon_duckdb_amd import arrow
    zp, fp, _ = fastq_seed_files[0]
    a = arrow.new_reader(str(zp), "fastq").read_all()
    b = arrow.new_reader(str(fp), "fastq").read_all()
    assert a.num_rows > 10000 and a.equals(b)


@pytest.mark.parametrize("window_log,codes", [(26, (24, 25, 26)), (27, (27,))])
def test_large_offsets(gpu, tmp_path, monkeypatch, window_log, codes):
    from exon_duckdb_amd.reader import ShardReader
    f = zf.big_window_frame(window_log, codes)
    comp = zf.encode(f)
    want = zf.expected_output(f)
    rc, out = zstd_decode(gpu, comp)
    assert rc == 0, out
    assert out == want
    del out
    zp, fp = tmp_path / "big.fastq.zst", tmp_path / "big.fastq"
    zp.write_bytes(comp)
    fp.write_bytes(want)
    n_rec = len(want) // 256
    del want
    monkeypatch.delenv("EXG_DEVICE_MEM_CAP_MB", raising=False)
    monkeypatch.setenv("EXG_STREAM_ROUND_OUT", str(1 << 20))
    r = ShardReader(str(zp), "fastq")
    got = r.digest()
    st = r.stats()
    r.close()
    assert got[0] == n_rec
    assert got == ShardReader(str(fp), "fastq").digest()
    assert st["decoded_segments"] >= 32, st
    if window_log == 27:
        over = zf.encode(zf.big_window_frame(27, codes, mantissa=1))   # Window_Size 1 << 27 + 1 << 24
        assert not decompress_stream(over)[0]
        rc, msg = zstd_decode(gpu, over)
        assert rc != 0 and "memory" in msg, msg


def test_fetching_index_walk_in_a_child(gpu, tmp_path):
    """EXG_ZSTD_INDEX_PREFETCH_MIN and EXG_ZSTD_CHUNK_BYTES are read once per process: a fresh child with both small reads
    FASTQ seed files (one frame; three frames with skippable frames between) and decodes catalogue frames"""
    files = []
    for seed in (301, 302):
        f = zf.random_frame(seed, 2 << 20, fastq=True)
        (tmp_path / ("c%d.fastq.zst" % seed)).write_bytes(zf.encode(f))
        (tmp_path / ("c%d.fastq" % seed)).write_bytes(zf.expected_output(f))
        files.append("c%d" % seed)
    fr = [zf.random_frame(s, 600_000, fastq=True) for s in (303, 304, 305)]
    (tmp_path / "m.fastq.zst").write_bytes(zf.encode([fr[0], skippable(b"x"), fr[1], skippable(b""), fr[2]]))
    (tmp_path / "m.fastq").write_bytes(zf.expected_output(fr))
    files.append("m")
    cat = zf.catalogue()
    for n in ("chunk_crossing", "rep_offsets", "repeat_tables_far", "nseq_edges", "blocks_between"):
        (tmp_path / (n + ".zst")).write_bytes(zf.encode(cat[n]))
        (tmp_path / (n + ".out")).write_bytes(zf.expected_output(cat[n]))
    here = os.path.dirname(os.path.abspath(__file__))
    code = (
        "import os, sys\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import torch\n"
        "from exon_duckdb_amd import load_library\n"
        "from exon_duckdb_amd.reader import ShardReader\n"
        "from test_zstd_gpu import zstd_decode\n"
        "d = %r\n"
        "lib = load_library()\n"
        "for f in %r:\n"
        "    a = ShardReader(os.path.join(d, f + '.fastq.zst'), 'fastq').digest()\n"
        "    b = ShardReader(os.path.join(d, f + '.fastq'), 'fastq').digest()\n"
        "    assert a == b and a[0] > 1000, (f, a, b)\n"
        "for n in %r:\n"
        "    rc, out = zstd_decode(lib, open(os.path.join(d, n + '.zst'), 'rb').read())\n"
        "    assert rc == 0 and out == open(os.path.join(d, n + '.out'), 'rb').read(), (n, rc)\n"
        "print('child ok')\n"
    ) % (os.path.dirname(here), here, str(tmp_path), files, ["chunk_crossing", "rep_offsets", "repeat_tables_far", "nseq_edges",
                                                              "blocks_between"])
    env = dict(os.environ, EXG_ZSTD_INDEX_PREFETCH_MIN="0", EXG_ZSTD_CHUNK_BYTES=str(16 << 10), EXG_STREAM_ROUND_OUT=str(128 << 10))
    env.pop("EXG_DEVICE_MEM_CAP_MB", None)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "child ok" in res.stdout, res.stdout[-1000:] + res.stderr[-3000:]
