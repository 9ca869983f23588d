"""Device bzip2 against the hand-built streams of tests/bzip2_frames.py (proved against libbz2 in tests/test_bzip2_frames.py):
every valid form alone and all of them as one input, every invalid one refused with its reason, every truncation, bit
flips of a hand-built stream, more block magics than the first discovery pass holds, and the reader in windows smaller
than a block (EXG_BZIP2_WINDOW_BYTES) with one block per round (EXG_STREAM_ROUND_OUT at its floor)."""
import random

import pytest

import bzip2_frames as F
from test_bzip2_frames import MAX_BLOCKS, SEEDS, WINDOWS, libbz2
from test_bzip2_gpu import bz_decode

pytestmark = pytest.mark.gpu


def first_difference(got, want):
    if len(got) != len(want):
        return "%d bytes, want %d" % (len(got), len(want))
    return "first difference at byte %d of %d" % (next(i for i in range(len(want)) if got[i] != want[i]), len(want))


def decode_all(gpu, cases):
    """cases: (name, stream, want) -> the list of those that fail"""
    wrong = []
    for name, s, want in cases:
        rc, out = bz_decode(gpu, s)
        if rc != 0:
            wrong.append((name, "refused", out))
        elif out != want:
            wrong.append((name, first_difference(out, want)))
    return wrong


def test_every_valid_form(gpu):
    wrong = decode_all(gpu, [(n, s, want) for n, (s, want) in sorted(F.catalogue().items())])
    assert not wrong, wrong


def test_generator_seeds(gpu):
    valid, wrong = [], []
    for seed in SEEDS:
        s, want, reason = F.generate(seed)
        if want is not None:
            valid.append(("seed %d" % seed, s, want))
            continue
        rc, msg = bz_decode(gpu, s)
        if rc == 0 or reason not in msg:
            wrong.append((seed, rc, msg if rc else "accepted"))
    assert 10 * len(valid) >= 9 * len(SEEDS)
    wrong += decode_all(gpu, valid)
    assert not wrong, wrong


def test_all_valid_forms_as_one_input(gpu):
    """blocks at every bit phase and streams of every level in one call.  A level-1 stream comes first, so the first round's
    slots hold 100 000 bytes: the level-9 block of 100 001 ends that round (kOverflow) and the next one has the larger slot"""
    cat = F.catalogue()
    names = ["header_level_1"] + [n for n in sorted(cat) if not n.startswith(F.TRAILING) and n != "header_level_1"]
    assert names.index("level_9_with_nblock_100001_then_level_1") > 0
    comp = b"".join(cat[n][0] for n in names)
    want = b"".join(cat[n][1] for n in names)
    assert libbz2(comp) == want
    rc, out = bz_decode(gpu, comp)
    assert rc == 0, out
    assert out == want, first_difference(out, want)


def wording(reason):
    return {F.R_TRUNCATED: "unexpected end of stream", F.R_NOT_BZIP2: "not a bzip2 stream"}.get(reason, reason)


def test_every_invalid_form_is_refused_with_its_reason(gpu):
    wrong = []
    for name, (s, reason, clause) in F.invalid().items():
        if name.startswith("truncated_at_"):
            continue
        rc, msg = bz_decode(gpu, s)          # (bz_decode asserts that a refusal leaves no output pointer)
        if rc == 0:
            wrong.append((name, "accepted", clause))
        elif wording(reason) not in msg:
            wrong.append((name, msg, "want", wording(reason)))
        elif name in F.BAD_BLOCK and "block %d:" % F.BAD_BLOCK[name] not in msg:
            wrong.append((name, msg, "want block", F.BAD_BLOCK[name]))
    assert not wrong, wrong


def test_every_truncation_is_refused(gpu):
    whole, cut_ok, first = F.truncation_stream()
    inv = F.invalid()
    wrong = []
    for cut in range(1, len(whole)):
        rc, out = bz_decode(gpu, whole[:cut])
        if cut == cut_ok:
            if rc != 0 or out != first:
                wrong.append((cut, "the cut behind stream 1 is valid", out))
            continue
        if rc == 0:
            wrong.append((cut, "accepted"))
        elif wording(inv["truncated_at_%d" % cut][1]) not in out:
            wrong.append((cut, out))
    assert not wrong, wrong


def three_blocks():
    """a code of 20 bits, six tables that switch every group, and a block of 17 byte values with an unused ramp table; every
    block longer than 618 bytes (libbz2 derandomises a block whose randomised bit a flip sets: from byte 618 on that breaks
    its CRC, the device refuses such a block outright)"""
    r = random.Random(77)
    d = bytes(r.choice(b"ABCDEFGHIJKLMNOPQRS") for _ in range(1500))
    a = F.data_block(d)
    alpha = len(set(a["L"])) + 2
    lens = [min(i + 1, 20) for i in range(alpha)]
    lens[-1] = 20
    a["tables"] = [lens, F.uniform_lengths(alpha)]
    b = F.with_tables(r, F.data_block(r.randbytes(1200)), 6, selectors=lambda n: [g % 6 for g in range(n)])
    c = F.data_block(bytes(r.choice(b"acgtnACGTN\n 0123456") for _ in range(900)))
    c["tables"] = [F.uniform_lengths(19 + 2), F.ramp_lengths(19 + 2)]
    assert 20 in lens and alpha == 21 and len(set(c["L"])) == 19
    return F.stream([a, b, c], 3)


def test_single_bit_flips_of_a_hand_built_stream_agree_with_libbz2(gpu):
    comp, want = three_blocks()
    assert libbz2(comp) == want
    r = random.Random(201)
    wrong, n_err = [], 0
    for _ in range(200):
        bit = r.randrange(len(comp) * 8)
        bad = bytearray(comp)
        bad[bit >> 3] ^= 0x80 >> (bit & 7)
        bad = bytes(bad)
        ref = libbz2(bad)
        rc, out = bz_decode(gpu, bad)
        n_err += ref is None
        if (ref is None) != (rc != 0) or (ref is not None and out != ref):
            wrong.append((bit, "libbz2 refuses" if ref is None else "libbz2 accepts", out if rc else first_difference(out, ref)))
    assert not wrong, wrong
    assert n_err > 0


def test_more_block_magics_than_the_first_discovery_pass_holds(gpu):
    """5000 level-1 streams of one tiny block: 10 000 magics against a first-pass cap of max(4096, n / 4096), so the
    second pass runs.  (Level 1 keeps the round's workspace near 3 GB: 10 000 columns and 5000 LF vectors of 100 000.)"""
    parts = [F.stream([F.data_block(b"payload %02d of sixteen\n" % k)], 1) for k in range(16)]
    r = random.Random(5000)
    pick = [r.randrange(16) for _ in range(5000)]
    comp = b"".join(parts[k][0] for k in pick)
    want = b"".join(parts[k][1] for k in pick)
    assert len(F.magic_offsets(comp[:len(parts[0][0]) * 2])) >= 4 and max(4096, len(comp) // 4096) < 10000
    rc, out = bz_decode(gpu, comp)
    assert rc == 0, out
    assert out == want, first_difference(out, want)


# ---------------------------------------------------------------- the reader in hand-built rounds
def _read(path, **kw):
    from exon_duckdb_amd.reader import ShardReader
    r = ShardReader(str(path), "fastq", **kw)
    try:
        rows = r.rows()
        return rows, r.stats()
    finally:
        r.close()


@pytest.fixture(scope="module")
def reader_case(tmp_path_factory):
    data, text, layout = F.reader_file()
    d = tmp_path_factory.mktemp("bzip2_frames")
    (d / "hand.fastq").write_bytes(text)
    (d / "hand.fastq.bz2").write_bytes(data)
    rows, _ = _read(d / "hand.fastq")
    assert len(rows) == text.count(b"\n") // 4 == 330
    return d, data, layout, rows


def set_rounds(monkeypatch, window, max_blocks):
    for name, value in (("EXG_BZIP2_WINDOW_BYTES", window), ("EXG_STREAM_ROUND_OUT", max_blocks)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))       # (EXG_STREAM_ROUND_OUT = 1: its floor, 128 KiB, one block a round)
    monkeypatch.delenv("EXG_DEVICE_MEM_CAP_MB", raising=False)


@pytest.mark.parametrize("max_blocks", MAX_BLOCKS)
@pytest.mark.parametrize("window", WINDOWS)
def test_reader_in_small_windows(gpu, reader_case, monkeypatch, window, max_blocks):
    d, data, layout, want = reader_case
    n_blocks = sum(k == "block" for k, _, _ in layout)
    rs = F.rounds(data, layout, window if window else 1 << 20, max_blocks)      # the producer's rounds, restated
    assert sum(x["blocks"] for x in rs) == n_blocks
    if window == 512:
        assert max(x["grow"] for x in rs) >= 8      # smaller than a block: the window doubles until it holds one
    set_rounds(monkeypatch, window, max_blocks)
    rows, st = _read(d / "hand.fastq.bz2", compression="bzip2")
    assert len(rows) == len(want) and rows == want
    if max_blocks == 1:
        # a round holds one block and pushes one segment; the count is that plus at most an empty last one and the one in hand
        assert n_blocks <= st["decoded_segments"] <= n_blocks + 2, (st["decoded_segments"], n_blocks)


def test_reader_names_the_damaged_block(gpu, reader_case, monkeypatch, tmp_path):
    from exon_duckdb_amd import ExgError
    from exon_duckdb_amd.reader import ShardReader
    d, data, layout, want = reader_case
    a, b = [(a, b) for k, a, b in layout if k == "block"][25]
    bad = bytearray(data)
    bad[(a + 48 + 13) >> 3] ^= 0x80 >> ((a + 48 + 13) & 7)         # a bit of block 25's stored CRC
    (tmp_path / "crc.fastq.bz2").write_bytes(bytes(bad))
    (tmp_path / "cut.fastq.bz2").write_bytes(data[:(a + b) // 16])  # the middle of block 25
    set_rounds(monkeypatch, 4096, 1)
    for name, texts in (("crc", ("block 25: block CRC mismatch",)), ("cut", ("block 25", "unexpected end"))):
        r = ShardReader(str(tmp_path / (name + ".fastq.bz2")), "fastq", compression="bzip2")
        with pytest.raises(ExgError) as e:
            r.count()
        r.close()
        assert any(t in str(e.value) for t in texts), (name, str(e.value))
    r = ShardReader(str(d / "hand.fastq.bz2"), "fastq", compression="bzip2")
    assert r.count() == len(want)
    r.close()
