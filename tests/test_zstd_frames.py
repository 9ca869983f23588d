"""The zstd frame writer of tests/zstd_frames.py proved against libzstd before it judges the device: every catalogue frame and
generator seed decodes under libzstd to exactly what the RFC's rules compute (expected_output), libzstd refuses the invalid
frames, the catalogue covers every form the list names, and the host block walks (memory, file, prefix) take the frames under
AddressSanitizer + UBSan, block for block alike (tests/host_asan_driver.cpp)."""
import os

import pytest

import zstd_frames as zf
from zstd_util import decompress_stream, skippable

SEEDS = list(range(60))


def _seed_frame(seed):
    return zf.random_frame(seed, 150_000, fastq=seed % 3 == 0)


@pytest.mark.parametrize("name", sorted(zf.catalogue()))
def test_catalogue_frame_decodes_to_expected(name):
    spec = zf.catalogue()[name]
    ok, out = decompress_stream(zf.encode(spec))
    assert ok, (name, out)
    assert out == zf.expected_output(spec), name


@pytest.mark.parametrize("window_log,codes", [(26, (24, 25, 26)), (27, (27,))])
def test_big_window_frames(window_log, codes):
    f = zf.big_window_frame(window_log, codes)
    comp = zf.encode(f)
    assert len(comp) < (400 << 10)          # filled by long matches, not literals
    ok, out = decompress_stream(comp)
    assert ok, out
    assert out == zf.expected_output(f)
    assert {"of:code%d" % c for c in codes} <= zf.forms(f)
    # one window step above libzstd's default limit (1 << 27): refused
    if window_log == 27:
        assert not decompress_stream(zf.encode(zf.big_window_frame(27, codes, mantissa=1)))[0]


def test_invalid_frames_are_refused():
    for name, (spec, clause, libzstd_refuses) in zf.invalid().items():
        ok, out = decompress_stream(zf.encode(spec))
        # (bad_rep3_zero: libzstd 1.4.8 reads an offset of 0 as 1; 1.5.x refuses it — only the device is held to the refusal)
        if libzstd_refuses:
            assert not ok, (name, clause)


def test_generator_seeds_decode_to_expected():
    for seed in SEEDS:
        f = _seed_frame(seed)
        ok, out = decompress_stream(zf.encode(f))
        assert ok, (seed, out)
        want = zf.expected_output(f)
        assert want == f._content, seed     # the generator's own content: the sequences it chose regenerate it
        assert out == want, seed


def test_fastq_generator_writes_fastq():
    f = zf.random_frame(7, 300_000, fastq=True)
    text = zf.expected_output(f)
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    for i in range(0, len(lines) - 1, 4):
        assert lines[i].startswith(b"@G") and lines[i + 2] == b"+" and len(lines[i + 1]) == len(lines[i + 3]) > 0


def test_catalogue_covers_every_form():
    seen = set()
    for spec in zf.catalogue().values():
        seen |= zf.forms(spec)
    for spec, _, _ in zf.invalid().values():
        seen |= zf.forms(spec)
    for wl, codes in ((26, (24, 25, 26)), (27, (27,))):
        seen |= zf.forms(zf.big_window_frame(wl, codes))
    missing = zf.REQUIRED_FORMS - seen
    assert not missing, sorted(missing)
    # the generator reaches repeat codes with ll == 0, Repeat_Mode tables and treeless literals by itself
    gen = set()
    for seed in SEEDS[:20]:
        gen |= zf.forms(_seed_frame(seed))
    assert {"of:rep1_ll0", "of:rep3_ll0", "tbl:rep_fse", "lit:treeless", "nseq:0", "blk:raw_between"} <= gen, sorted(gen)


def test_multi_frame_stream():
    cat = zf.catalogue()
    parts = [cat["rep_offsets"], skippable(b"between"), cat["treeless_chain"], cat["repeat_tables_far"], skippable(b"", 15),
             cat["match_to_frame_start"][0]]
    ok, out = decompress_stream(zf.encode(parts))
    assert ok, out
    assert out == zf.expected_output([p for p in parts if isinstance(p, zf.Frame)])


def test_catalogue_through_host_walks_under_asan(tmp_path):
    if not os.path.isdir("/opt/rocm/include"):
        pytest.skip("HIP headers not found")
    from test_host_asan import build_driver, run_driver
    exe = tmp_path / "host_asan"
    build_driver(exe)
    cat = zf.catalogue()
    small = [s for n, s in sorted(cat.items()) if n not in ("rle_codes_16m",)]
    files = {
        "catalogue.zst": zf.encode([x for s in small for x in (s if isinstance(s, list) else [s])]),
        "rle16m.zst": zf.encode(cat["rle_codes_16m"]),
        "invalid.zst": b"".join(zf.encode(s) for s, _, _ in zf.invalid().values()),
        "seeds.zst": zf.encode([_seed_frame(s) for s in (1, 3, 5)]),
        "fastq_seed.zst": zf.encode(zf.random_frame(9, 300_000, fastq=True)),
    }
    paths = []
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
        paths.append(str(tmp_path / name))
    res = run_driver(exe, paths)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "runs" in res.stdout
