"""bzip2 on the device (exg_bzip2_decode and the reader's bzip2 producer) against libbz2 (Python's bz2): every level,
block-limit edges, concatenated streams, hand-built streams libbz2 accepts but its encoder never writes (bzip2_frames.py),
corruption (an error wherever libbz2 gives one, the same bytes wherever it accepts), and reads through the reader."""
import bz2
import ctypes as C
import os
import random

import pytest

import bzip2_frames as F

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def bz_decode(lib, comp: bytes):
    """-> (rc, bytes | message)"""
    from exon_duckdb_amd import device
    d_comp = device.upload(comp if comp else b"\0")
    out = C.c_void_p()
    produced = C.c_uint64(0)
    rc = lib.exg_bzip2_decode(C.c_void_p(d_comp.data_ptr()), len(comp), C.byref(out), C.byref(produced), device.stream_ptr())
    if rc != 0:
        assert not out.value
        return rc, lib.exg_last_error_message().decode()
    n = produced.value
    buf = (C.c_uint8 * max(n, 1))()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(buf, out, n, 2) == 0
    lib.exg_free_device(out, n + 64)
    return 0, bytes(buf)[:n]


def libbz2(comp):
    try:
        return bz2.decompress(comp)
    except (OSError, ValueError, EOFError):
        return None


def fastq_text(n, seed=1):
    r = random.Random(seed)
    out = []
    for i in range(n):
        s = "".join(r.choice("ACGT") for _ in range(150))
        q = "".join(chr(33 + r.randint(2, 40)) for _ in range(150))
        out.append(f"@read{i} len=150\n{s}\n+\n{q}\n")
    return "".join(out).encode()


def payloads():
    r = random.Random(3)
    return {
        "empty": b"",
        "one": b"x",
        "all_bytes": bytes(range(256)),
        "run3": b"A" * 3,
        "run4": b"A" * 4,
        "run5": b"A" * 5,
        "run259": b"B" * 259,
        "run260": b"B" * 260,
        "run1e6": b"C" * 1000000,
        "random2mb": r.randbytes(2 << 20),
        "fastq": fastq_text(3000),
        "vcf_lines": b"chr1\t12345\trs99\tA\tG\t50.0\tPASS\tDP=10;AF=0.5\n" * 20000,
        "acgtn": bytes(r.choice(b"ACGTN") for _ in range(300000)),
        "groups_small": bytes(r.choice(b"AC") for _ in range(40)),      # few selectors: 2 groups
        "groups_mid": bytes(r.choice(b"ACGT") for _ in range(500)),     # 3..4 groups
        "groups_large": r.randbytes(3000),                              # 5..6 groups
    }


@pytest.fixture(scope="module")
def data():
    return payloads()


@pytest.mark.parametrize("name", list(payloads().keys()))
def test_levels(gpu, data, name):
    d = data[name]
    for level in (1, 5, 9):
        comp = bz2.compress(d, level)
        rc, out = bz_decode(gpu, comp)
        assert rc == 0, (name, level, out)
        assert out == d, (name, level, len(out), len(d))


def test_fifty_mb_of_one_byte(gpu):
    d = b"A" * (50 << 20)
    rc, out = bz_decode(gpu, bz2.compress(d, 9))
    assert rc == 0, out
    assert len(out) == len(d) and out == d


@pytest.mark.parametrize("level", [1, 9])
def test_block_limit_edges(gpu, level):
    # random bytes pass RLE1 unchanged: a block holds level x 100 000 - 19 of them (the encoder's margin)
    r = random.Random(level)
    lim = level * 100000 - 19
    for n in (lim - 1, lim, lim + 1):
        d = r.randbytes(n)
        rc, out = bz_decode(gpu, bz2.compress(d, level))
        assert rc == 0 and out == d, (level, n)


def test_concatenated_streams(gpu, data):
    parts = [bz2.compress(data["fastq"], 9), bz2.compress(b"", 1), bz2.compress(data["all_bytes"], 3), bz2.compress(b"", 9),
             bz2.compress(data["random2mb"][:300000], 1)]
    comp = b"".join(parts)
    assert libbz2(comp) is not None
    rc, out = bz_decode(gpu, comp)
    assert rc == 0, out
    assert out == libbz2(comp)
    rc, out = bz_decode(gpu, bz2.compress(b"", 9) * 3)
    assert rc == 0 and out == b""


def _check(gpu, comp, want=None):
    ref = libbz2(comp)
    assert ref is not None
    if want is not None:
        assert ref == want
    rc, out = bz_decode(gpu, comp)
    assert rc == 0, out
    assert out == ref


def test_hand_built_code_of_length_20(gpu):
    d = bytes(random.Random(1).choice(b"ABCDEFGHIJKLMNOPQRS") for _ in range(3000))
    blk = F.data_block(d)
    alpha = len(set(blk["L"])) + 2
    lens = [min(i + 1, 20) for i in range(alpha)]
    lens[-1] = 20
    blk["tables"] = [lens, F.uniform_lengths(alpha)]
    s, _ = F.stream([blk])
    _check(gpu, s, d)


def test_hand_built_six_tables_switching_every_group(gpu):
    r = random.Random(2)
    d = r.randbytes(5000)
    blk = F.data_block(d)
    used = sorted(set(blk["L"]))
    alpha = len(used) + 2
    syms = F.mtf_rle2(blk["L"], used)
    tables = []
    for t in range(6):
        base = F.uniform_lengths(alpha)
        k = base[0]
        # one short code and two long ones per table, at different symbols: still a prefix code
        lens = [k + 1] * alpha
        free = (1 << (k + 1)) - alpha
        for i in range(min(free, alpha)):
            lens[(i * 7 + t * 13) % alpha] = k
        tables.append(lens)
    blk.update(tables=tables, selectors=[g % 6 for g in range((len(syms) + 49) // 50)])
    s, _ = F.stream([blk])
    _check(gpu, s, d)


def test_hand_built_origptr_at_both_ends(gpu):
    for d in (b"abcdefgh", b"zabcdefg"):
        blk = F.data_block(d)
        assert blk["orig"] in (0, len(blk["L"]) - 1)
        s, _ = F.stream([blk])
        _check(gpu, s, d)
    seen = {F.data_block(d)["orig"] for d in (b"abcdefgh", b"zabcdefg")}
    assert seen == {0, 7}


def test_hand_built_one_byte_value(gpu):
    for d in (b"q", b"qq", b"qqq"):
        s, _ = F.stream([F.data_block(d)])
        _check(gpu, s, d)


def test_hand_built_block_magic_inside_huffman_bits(gpu):
    # 256 byte values, 8-bit codes for symbols 0..253: the symbol stream's bits are the MTF symbols themselves, so the
    # symbols 0x31 0x41 0x59 0x26 0x53 0x59 spell the block magic; L is searched until its LF mapping is one cycle
    used = list(range(256))
    lens = [8] * 254 + [9] * 4
    magic = [0x31, 0x41, 0x59, 0x26, 0x53, 0x59]
    r = random.Random(9)
    for attempt in range(200):
        idx = [r.randint(1, 200) for _ in range(300)]
        at = r.randint(10, 250)
        idx[at:at + 6] = [m - 1 for m in magic]
        L = F.inverse_mtf(idx, used)
        orig = r.randrange(len(L))
        if not F.one_cycle(L, orig):
            continue
        syms = [k + 1 for k in idx] + [257]
        blk = {"L": L, "orig": orig, "syms": syms, "used": used, "tables": [lens, lens]}
        s, out = F.stream([blk, F.data_block(b"tail block")])
        bits = bin(int.from_bytes(s, "big"))[2:].zfill(len(s) * 8)
        assert bits.count(format(0x314159265359, "048b")) >= 3  # two true block magics + the one in the Huffman data
        _check(gpu, s)
        return
    pytest.fail("no single-cycle block found")


def test_truncations_are_errors(gpu, data):
    comp = bz2.compress(data["fastq"], 9) + bz2.compress(data["random2mb"][:200000], 1)
    for cut in (1, 3, 4, 10, 20, len(comp) // 5, len(comp) // 2, len(comp) - 200, len(comp) - 11, len(comp) - 1):
        assert libbz2(comp[:cut]) is None or cut <= 4
        rc, out = bz_decode(gpu, comp[:cut])
        assert rc != 0, cut


def test_single_bit_flips_agree_with_libbz2(gpu):
    d = fastq_text(60, 4) + bytes(range(256)) + b"G" * 300
    comp = bz2.compress(d, 9)
    r = random.Random(200)
    n_err = 0
    for _ in range(200):
        bit = r.randrange(len(comp) * 8)
        bad = bytearray(comp)
        bad[bit >> 3] ^= 0x80 >> (bit & 7)
        bad = bytes(bad)
        ref = libbz2(bad)
        rc, out = bz_decode(gpu, bad)
        if ref is None:
            assert rc != 0, bit
            n_err += 1
        else:
            assert rc == 0 and out == ref, (bit, out if rc else len(out))
    assert n_err > 100


def test_wrong_crcs_and_randomised_blocks(gpu):
    blk = F.data_block(b"hello bzip2 world")
    good = F.crc(b"hello bzip2 world")
    s, _ = F.stream([dict(blk, block_crc=good ^ 1)])
    rc, msg = bz_decode(gpu, s)
    assert rc != 0 and "CRC" in msg and libbz2(s) is None
    s, _ = F.stream([blk], stream_crc=good ^ 0x100)
    rc, msg = bz_decode(gpu, s)
    assert rc != 0 and "CRC" in msg and libbz2(s) is None
    s, _ = F.stream([dict(blk, randomised=1)])
    rc, msg = bz_decode(gpu, s)
    assert rc != 0 and "randomised" in msg
    rc, msg = bz_decode(gpu, b"not bzip2 at all")
    assert rc != 0 and "not a bzip2 stream" in msg


# ---------------------------------------------------------------- reader level
def _write(tmp_path, name, raw, level=9):
    p = tmp_path / name
    p.write_bytes(bz2.compress(raw, level))
    return p


def test_reader_golden_files(gpu, tmp_path, oracle):
    from exon_duckdb_amd.reader import ShardReader
    for name, fmt, n in (("test.fastq", "fastq", 2), ("test.fasta", "fasta", 2), ("vcf/index.vcf", "vcf", 621)):
        raw = open(os.path.join(GOLDEN, name), "rb").read()
        p = _write(tmp_path, os.path.basename(name) + ".bz2", raw)
        r = ShardReader(str(p), fmt, compression="bzip2")
        got = r.count()
        st = r.stats()
        r.close()
        assert got == n, (name, got)
        assert st.get("input_compression", 3) == 3
        r = ShardReader(str(p), fmt, compression="bzip2")
        plain = ShardReader(os.path.join(GOLDEN, name), fmt)
        assert r.digest() == plain.digest(), name
        r.close()
        plain.close()


def test_table_function_and_new_reader(gpu, tmp_path):
    from exon_duckdb_amd import table_function as tf
    from exon_duckdb_amd.arrow import new_reader
    plain = os.path.join(GOLDEN, "vcf/index.vcf")
    p = _write(tmp_path, "index.vcf.bz2", open(plain, "rb").read())
    t = new_reader(str(p), "vcf", compression="bzip2").read_all()
    want = new_reader(plain, "vcf").read_all()
    assert t.num_rows == 621 and t.equals(want)
    row = t.slice(0, 1).to_pylist()[0]  # test_vcf_record_scan.test:10-19
    assert row["chrom"] == "1" and row["pos"] == 9999919 and row["ref"] == "G" and row["alt"] == ["<*>"]
    con = tf.connect()
    assert con.table_function("read_vcf", str(p), compression="bzip2").count() == 621
    q = _write(tmp_path, "test.fastq.bz2", open(os.path.join(GOLDEN, "test.fastq"), "rb").read())
    rel = con.table_function("read_fastq", str(q), compression="bzip2")
    assert rel.count() == 2


def test_directory_plain_extension_corrupt_and_shards(gpu, tmp_path):
    from exon_duckdb_amd import ExgError, abi
    from exon_duckdb_amd.reader import ShardReader
    raw = open(os.path.join(GOLDEN, "test.fastq"), "rb").read()
    d = tmp_path / "dir"
    d.mkdir()
    for i in range(3):
        _write(d, f"part{i}.fastq.bz2", raw)
    r = ShardReader(str(d), "fastq", compression="bzip2")
    assert r.count() == 6
    r.close()
    p = _write(tmp_path, "reads.fastq.bz2", raw)
    with pytest.raises(ExgError):  # no compression=: read as text, like the reference
        r = ShardReader(str(p), "fastq")
        r.count()
    with pytest.raises(ExgError) as e:
        ShardReader(str(p), "fastq", compression="bzip2", shard_index=0, shard_count=2)
    assert e.value.code == abi.EXG_E_UNSUPPORTED
    big = fastq_text(20000, 5)
    comp = bytearray(bz2.compress(big, 1))
    comp[len(comp) * 3 // 4] ^= 0x10
    q = tmp_path / "bad.fastq.bz2"
    q.write_bytes(bytes(comp))
    r = ShardReader(str(q), "fastq", compression="bzip2")
    with pytest.raises(ExgError):
        r.count()
    r.close()


def test_bounded_memory(gpu, oracle, tmp_path, monkeypatch):
    from exon_duckdb_amd.reader import ShardReader
    data = bytes(oracle.synth_fastq(332 * 420000))  # 139 MB
    p = tmp_path / "big.fastq.bz2"
    p.write_bytes(bz2.compress(data, 9))
    monkeypatch.delenv("EXG_DEVICE_MEM_CAP_MB", raising=False)
    r = ShardReader(str(p), "fastq", compression="bzip2")
    free = r.digest()
    r.close()
    monkeypatch.setenv("EXG_DEVICE_MEM_CAP_MB", "16")
    r = ShardReader(str(p), "fastq", compression="bzip2")
    capped = r.digest()
    st = r.stats()
    r.close()
    plain = tmp_path / "big.fastq"
    plain.write_bytes(data)
    monkeypatch.delenv("EXG_DEVICE_MEM_CAP_MB", raising=False)
    r = ShardReader(str(plain), "fastq")
    want = r.digest()
    r.close()
    assert free == capped == want
    assert st["device_bytes_peak"] <= 16 << 20, st
    assert st["decoded_segments"] >= 8, st
