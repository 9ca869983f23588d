"""Device inflate against the hand-built DEFLATE streams of tests/deflate_frames.py (proved against zlib in
tests/test_deflate_frames.py): every RFC 1951 form zlib's compressor never writes, through the members decoder
(exg_inflate_members, all streams of a kind as members of ONE launch, canaries between their outputs), the chunked decoder
(exg_inflate_stream) and the reader; every invalid stream refused with the class InflateStatus names."""
import ctypes as C
import random
import re
import struct
import zlib

import numpy as np
import pytest

import deflate_frames as df
from exon_duckdb_amd import abi
from test_deflate_frames import SEED_BYTES, SEEDS            # the seeds proved against zlib on the CPU
from test_inflate_gpu import index_members, inflate_gpu
from test_inflate_stream_gpu import stream_inflate

pytestmark = pytest.mark.gpu

CANARY = 64
FILL = 0xA5


def launch(lib, jobs):
    """jobs: (raw stream, comp_size or None = all of it, out_cap) -> one exg_inflate_members launch over all of them.  The
    streams lie back to back at staggered offsets (a stream's neighbour is what follows its last byte); the outputs at
    staggered offsets that are no multiple of 16, CANARY bytes and more apart, in a buffer filled with FILL.
    -> (output buffer as numpy, status array, members)"""
    import torch
    from exon_duckdb_amd import device
    comp = bytearray()
    members = []
    out_off = 0
    for k, (raw, comp_size, out_cap) in enumerate(jobs):
        comp += b"\xEE" * ((5 * k) % 13)
        out_off += CANARY + 1 + (7 * k) % 15
        if out_off % 16 == 0:
            out_off += 3
        members.append(abi.InflateMember(len(comp), len(raw) if comp_size is None else comp_size, out_off, out_cap))
        comp += raw
        out_off += out_cap
    total = out_off + CANARY
    d_comp = device.upload(bytes(comp))
    d_out = torch.full((total + 64,), FILL, dtype=torch.uint8, device="cuda")
    marr = (abi.InflateMember * len(members))(*members)
    d_members = torch.frombuffer(bytearray(bytes(marr)), dtype=torch.uint8).cuda()
    d_status = torch.zeros(len(members) * 24, dtype=torch.uint8, device="cuda")
    device.check(lib.exg_inflate_members(C.c_void_p(d_comp.data_ptr()), C.c_void_p(d_out.data_ptr()), C.c_void_p(d_members.data_ptr()),
                                         C.c_void_p(d_status.data_ptr()), len(members), device.stream_ptr()))
    torch.cuda.synchronize()
    st = np.frombuffer(d_status.cpu().numpy().tobytes(), dtype=np.dtype([("code", "<u4"), ("pad", "<u4"), ("produced", "<u8"), ("consumed", "<u8")]))
    return d_out.cpu().numpy(), st, members


def untouched(out, members, k, written):
    """everything between the first `written` bytes of member k's output and the next member's output still holds FILL"""
    lo = members[k].out_off + written
    hi = members[k + 1].out_off if k + 1 < len(members) else len(out)
    return bool((out[lo:hi] == FILL).all())


def check_valid(out, st, members, k, name, want, consumed):
    assert int(st["code"][k]) == 0, (name, st[k])
    assert int(st["produced"][k]) == len(want), (name, st[k], len(want))
    assert int(st["consumed"][k]) == consumed, (name, st[k], consumed)
    o = members[k].out_off
    got = out[o:o + len(want)].tobytes()
    if got != want:
        bad = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError((name, "first difference at byte", bad, "of", len(want)))
    assert untouched(out, members, k, len(want)), (name, "wrote past its output")
    assert bool((out[o - CANARY:o] == FILL).all()), (name, "wrote in front of its output")


@pytest.fixture(scope="module")
def cat():
    """name -> (raw, expected output, consumed), computed once"""
    return {n: (df.encode(s), df.expected_output(s), df.consumed(s)) for n, s in sorted(df.catalogue().items())}


@pytest.fixture(scope="module")
def seeds():
    out = []
    for seed in SEEDS:
        s = df.random_stream(seed, SEED_BYTES)
        out.append((df.encode(s), s._content, df.consumed(s)))
    return out


def test_catalogue_as_members_of_one_launch(gpu, cat):
    names = list(cat)
    out, st, members = launch(gpu, [(cat[n][0], None, len(cat[n][1])) for n in names])
    for k, n in enumerate(names):
        check_valid(out, st, members, k, n, cat[n][1], cat[n][2])


def test_generator_seeds_as_members_of_one_launch(gpu, seeds):
    out, st, members = launch(gpu, [(raw, None, len(want)) for raw, want, _ in seeds])
    for k, (raw, want, used) in enumerate(seeds):
        check_valid(out, st, members, k, "seed %d" % SEEDS[k], want, used)


def test_catalogue_as_bgzf_members(gpu, cat):
    """the same streams framed as BGZF blocks and found by the host index (exg_gzip_index), as a .bam / .vcf.gz would bring them"""
    blob, payload = [], []
    for n, (raw, want, used) in cat.items():
        bsize = 12 + 6 + used + 8
        if bsize > 65536:
            continue                      # (BSIZE is 16 bits: the 65535-byte stored block does not fit a BGZF block)
        blob.append(b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1)
                    + raw[:used] + struct.pack("<II", zlib.crc32(want), len(want)))
        payload.append(want)
    gz = b"".join(blob)
    members, total, _ = index_members(gpu, gz)
    assert len(members) == len(blob) >= 30
    out, st = inflate_gpu(gpu, gz, members, total)
    assert (st["code"] == 0).all(), st
    for m, s, want in zip(members, st, payload):
        assert int(s["produced"]) == len(want) and out[m.out_off:m.out_off + len(want)].tobytes() == want


def test_invalid_streams_are_refused_with_their_class(gpu, cat):
    """every invalid stream between two valid ones, all in one launch: refused with the class the comment on InflateStatus
    gives it (1 block type / stored length, 2 code lengths, 3 symbol or distance, 5 input exhausted — what follows a truncated
    stream's last byte is its neighbour's first, not padding), the valid neighbours decoded, no byte outside any output"""
    inv = df.invalid()
    base_len = len(df.expected_output(df.truncation_stream()))
    valid = [n for n in cat if len(cat[n][0]) < 700]
    jobs, kinds = [], []
    for k, (name, (spec, clause, klass)) in enumerate(inv.items()):
        raw = df.encode(spec)
        jobs.append((raw, None, 40_000 if "32767" in name else max(base_len, 1024)))
        kinds.append((name, klass, clause))
        v = valid[k % len(valid)]
        jobs.append((cat[v][0], None, len(cat[v][1])))
        kinds.append((v, 0, None))
    out, st, members = launch(gpu, jobs)
    wrong = []
    for k, (name, klass, clause) in enumerate(kinds):
        if klass == 0:
            check_valid(out, st, members, k, name, cat[name][1], cat[name][2])
            continue
        code, produced = int(st["code"][k]), int(st["produced"][k])
        if code != klass:
            wrong.append((name, "code", code, "want", klass, clause))
        assert produced <= members[k].out_cap, name
        assert untouched(out, members, k, members[k].out_cap), (name, "wrote past its output")
    assert not wrong, wrong


@pytest.mark.parametrize("short", ["one_short", "half"])
def test_out_cap_too_small_is_code_4(gpu, cat, short):
    """a member told too small an out_cap stops with code 4 and leaves what lies behind out_off + out_cap alone"""
    names = [n for n in cat if len(cat[n][1]) > 0]
    caps = [len(cat[n][1]) - 1 if short == "one_short" else len(cat[n][1]) // 2 for n in names]
    out, st, members = launch(gpu, [(cat[n][0], None, cap) for n, cap in zip(names, caps)])
    for k, (n, cap) in enumerate(zip(names, caps)):
        assert int(st["code"][k]) == 4, (n, st[k], cap)
        assert int(st["produced"][k]) <= cap, (n, st[k], cap)
        assert untouched(out, members, k, cap), (n, "wrote past out_off + out_cap")
        want = cat[n][1]
        o = members[k].out_off
        # (what it flushed before it stopped is a prefix of the right answer or still untouched: whole 1 KiB segments)
        flushed = int(st["produced"][k]) // 1024 * 1024
        seg = out[o:o + flushed].tobytes()
        assert all(seg[i:i + 1024] in (want[i:i + 1024], bytes([FILL]) * 1024) for i in range(0, flushed, 1024)), n


# ---- the chunked decoder ------------------------------------------------------------------------------------------------------
def text_stream(seed, n_out, history=b"", final=False, kinds=("long", "pairs", "short", "found", "stored")):
    """generator blocks that inflate to text at ~3 bytes per compressed byte (mostly literals and short matches)"""
    return df.random_stream(seed, n_out, final=final, history=history, p_lit=0.7, p_short=0.97, kinds=kinds)


def qualifying_starts(spec, chunk_bytes):
    """k_find_blocks' rules, restated on the writer's own account of the stream: per boundary k * chunk_bytes the finder takes
    the first bit offset in [k, k + 1) * chunk_bytes that (a) reads as a dynamic header with BFINAL = 0 and a complete
    code-length code of >= 2 codes — every non-final Dynamic block of this writer does — and (b), text mode, decodes 4096
    output symbols from there without a control character among the literals (or reaches the stream's end).  -> the block
    starts (bit offsets) that meet both; the finder may still meet a false start in front of one, which the chain survives"""
    info = df.stats(spec)
    clean_from = []            # per block: does its output hold a control character (as a literal or stored byte)?
    for b in spec.blocks:
        lits = b.data if isinstance(b, df.Stored) else bytes(t for t in b.tokens if isinstance(t, int))
        n = len(b.data) if isinstance(b, df.Stored) else sum(1 if isinstance(t, int) else t[0] for t in b.tokens)
        clean_from.append((n, not any(c < 9 or 13 < c < 32 or c == 127 for c in lits)))
    good = []
    for k in range(1, (len(df.encode(spec)) + chunk_bytes - 1) // chunk_bytes):
        lo, hi = 8 * k * chunk_bytes, 8 * (k + 1) * chunk_bytes
        for i, (start, _) in enumerate(info["blocks"]):
            b = spec.blocks[i]
            if not (lo <= start < hi and isinstance(b, df.Dynamic) and not b.final):
                continue
            n = 0
            for m, clean in clean_from[i:]:
                if not clean:
                    break
                n += m
                if n > 4096:
                    break
            if n > 4096 or all(c for _, c in clean_from[i:]):
                good.append(start)
                break
    return good


@pytest.fixture(scope="module")
def chunked_cases(cat):
    """name -> (spec, raw, expected).
    mixed: ~45 KB (compressed) of generator text, then every catalogue stream's blocks (binary, non-final), then generator text to
    ~200 KB.  At chunk_bytes = 32768 the boundaries at 64 K and 96 K fall among the hand-built blocks, whose literals are binary:
    the text probe refuses them.  The boundaries at 32 K and from 128 K on fall into generator text, whose dynamic blocks are
    non-final, carry complete code-length codes and are followed by far more than 4096 symbols of text: they qualify (asserted
    below with qualifying_starts: at least three), at least half of all boundaries do, so the finder stays in text mode, and
    the hand-built forms are decoded by chunks that start behind the first one.
    fixed_stored: fixed and stored blocks only: no chunk start anywhere, one chunk decodes it all."""
    cases = {}
    blocks = []
    a = text_stream(101, 130_000)
    blocks += a.blocks
    assert 34_000 < len(df.encode(df.Stream(blocks))) < 60_000
    for n, s in sorted(df.catalogue().items()):
        blocks += df.nonfinal(s)
    hist = df.expected_output(blocks)
    n_cat = len(blocks)
    blocks += text_stream(102, 330_000, history=hist[-40_000:], final=True).blocks
    spec = df.Stream(blocks)
    raw = df.encode(spec)
    assert 150_000 <= len(raw) <= 250_000, len(raw)
    first_cat = df.stats(spec)["blocks"][len(a.blocks)][0]
    assert first_cat > 8 * 32768                                     # hand-built forms: not in the first chunk
    assert df.stats(spec)["blocks"][n_cat][0] < 8 * 4 * 32768 + 8 * 20_000
    for chunk in (32768, 65536):
        good = qualifying_starts(spec, chunk)
        assert len(good) >= (3 if chunk == 32768 else 2), (chunk, good)
        assert 2 * len(good) >= (len(raw) + chunk - 1) // chunk - 1    # text mode stays
        assert any(g > first_cat for g in good) and (chunk > 32768 or any(g < first_cat for g in good))
    cases["mixed"] = (spec, raw, df.expected_output(spec))
    fs = text_stream(103, 420_000, final=True, kinds=("fixed", "fixed", "stored"))
    assert not any(isinstance(b, df.Dynamic) and not b.final for b in fs.blocks)
    raw = df.encode(fs)
    assert 100_000 <= len(raw) <= 250_000, len(raw)
    cases["fixed_stored"] = (fs, raw, df.expected_output(fs))
    for spec, raw, want in cases.values():
        assert zlib.decompressobj(-15).decompress(raw) == want       # the writer, proved on these too
        assert len(want) < 1_100_000
    return cases


def traced_stream_inflate(capfd, monkeypatch, lib, raw, chunk, pad):
    """stream_inflate + what the decoder itself says it did (its EXG_TRACE lines on stderr): -> (rc, output, consumed),
    block starts the finder found, chunks in the chain that made the output (0 when the call failed before it had one)"""
    monkeypatch.setenv("EXG_TRACE", "1")
    capfd.readouterr()
    res = stream_inflate(lib, raw, chunk, pad_front=pad)
    err = capfd.readouterr().err
    monkeypatch.delenv("EXG_TRACE")
    starts = re.findall(r"(\d+) block starts found", err)
    chunks = re.findall(r"(\d+) chunks in the chain", err)
    return res, int(starts[0]) if starts else 0, int(chunks[-1]) if chunks else 0


@pytest.mark.parametrize("name", ["mixed", "fixed_stored"])
def test_chunked_decoder_on_hand_built_blocks(gpu, chunked_cases, name, capfd, monkeypatch):
    """chunk_bytes = 32768: the hand-built blocks lie in chunks behind the first (the device reports how many chunks made the
    output).  At 65536 the first boundary falls among them, so most of them are decoded by the first chunk, the last ones and the
    text behind them by later chunks."""
    spec, raw, want = chunked_cases[name]
    for chunk in (32768, 65536):
        for pad in (0, 13):
            (rc, got, consumed), n_starts, n_chunks = traced_stream_inflate(capfd, monkeypatch, gpu, raw, chunk, pad)
            assert rc == 0, (chunk, pad, gpu.exg_last_error_message())
            assert consumed == len(raw), (chunk, pad, consumed, len(raw))
            assert got == want, (chunk, pad, len(got), len(want))
            if name == "mixed":
                # (a real block start the finder took is a chunk of the chain; one boundary may lose its start to a false one in front)
                good = len(qualifying_starts(spec, chunk))
                assert n_starts >= good - 1 and n_chunks >= good, (chunk, pad, n_starts, n_chunks, good)
            else:
                assert n_chunks == 1, (chunk, pad, n_starts, n_chunks)      # no real block start to cut at


def short_window_stream(with_front):
    """10 KB of text, 7000 empty stored blocks (35 KB of input that produce nothing: the boundary at 32768 falls among them),
    then dynamic blocks of text whose matches reach 3 .. 9 KB back.  The chunk that starts at the first of those blocks has
    10 KB in front of it: less than a window, so the window in front of IT is handed on (tail_symbol, k < 0).  Without the
    front the same bits point before the stream's first byte."""
    front = text_stream(201, 10_000)
    hist = df.expected_output(front)
    assert 10_000 <= len(hist) < 32_768                              # less than a window
    tail = text_stream(202, 30_000, history=hist, final=True, kinds=("long", "short", "pairs"))
    assert isinstance(tail.blocks[0], df.Dynamic)
    far = sum(1 for b in tail.blocks for t in getattr(b, "tokens", ()) if not isinstance(t, int) and t[1] >= 3000)
    assert far > 50
    empty = [df.Stored(b"") for _ in range(7000)]
    if with_front:
        return df.Stream(front.blocks + empty + tail.blocks), tail
    return df.Stream(empty + tail.blocks), tail


def test_chunk_behind_a_short_window(gpu, capfd, monkeypatch):
    spec, _ = short_window_stream(True)
    raw, want = df.encode(spec), df.expected_output(spec)
    assert zlib.decompressobj(-15).decompress(raw) == want
    assert len(qualifying_starts(spec, 32768)) >= 1
    for pad in (0, 13):
        (rc, got, consumed), n_starts, n_chunks = traced_stream_inflate(capfd, monkeypatch, gpu, raw, 32768, pad)
        assert rc == 0, gpu.exg_last_error_message()
        assert got == want and consumed == len(raw)
        assert n_starts >= 1 and n_chunks >= 2, (n_starts, n_chunks)    # the blocks behind the empty ones: a chunk of their own


def test_distance_before_the_stream_in_a_later_chunk_is_refused(gpu, capfd, monkeypatch):
    """the twin without its front: the matches of the chunk behind the empty stored blocks point before byte 0.  zlib: "invalid
    distance too far back".  (The resolver used to check the first chunk's markers only: the call returned 0 and bytes of the
    zeroed window.)  The finder reports the block start it found: the bad markers are those of a chunk other than the first."""
    spec, _ = short_window_stream(False)
    raw = df.encode(spec)
    with pytest.raises(zlib.error, match="too far back"):
        zlib.decompressobj(-15).decompress(raw)
    assert len(qualifying_starts(spec, 32768)) >= 1                  # the offending block starts a chunk of its own
    for pad in (0, 13):
        (rc, got, _), n_starts, _ = traced_stream_inflate(capfd, monkeypatch, gpu, raw, 32768, pad)
        assert rc != 0, "a distance before the start of the output passed as valid"
        assert n_starts >= 1, "the offending blocks were not decoded as a chunk of their own"


def test_invalid_streams_are_refused_by_the_chunked_decoder(gpu):
    accepted = []
    for name, (spec, clause, klass) in df.invalid().items():
        rc, got, _ = stream_inflate(gpu, df.encode(spec), 32768, pad_front=13 if len(name) % 2 else 0)
        if rc == 0:
            accepted.append((name, clause))
    assert not accepted, accepted


# ---- the reader ---------------------------------------------------------------------------------------------------------------
def test_reader_on_a_hand_coded_gzip(gpu, oracle, tmp_path):
    """a FASTQ file cut by the writer's own match finder and coded with its skewed codes, framed as one gzip member with zlib's
    CRC-32: read_fastq gives the oracle's rows"""
    from exon_duckdb_amd import table_function
    raw = bytes(oracle.synth_fastq_ragged(400, seed=5))
    rng = random.Random(9)
    tokens = df.tokenise(raw)
    blocks, i = [], 0
    while i < len(tokens):
        n = rng.choice((50, 700, 3000))
        mode = rng.choice(("long", "short", (True, False, True), (False, True, False), "fixed"))
        part = tokens[i:i + n]
        blocks.append(df.Fixed(part) if mode == "fixed" else df.coded_block(part, rng, mode))
        i += n
    blocks.append(df.Stored(b"", final=True))
    spec = df.Stream(blocks)
    assert df.expected_output(spec) == raw
    gz = b"\x1f\x8b\x08\x00" + b"\0" * 4 + b"\0\xff" + df.encode(spec) + struct.pack("<II", zlib.crc32(raw), len(raw) & 0xFFFFFFFF)
    assert zlib.decompress(gz, 31) == raw
    p = tmp_path / "hand.fastq.gz"
    p.write_bytes(gz)
    con = table_function.connect()
    exp = oracle.fastq_parse(raw, want_string_t=False)
    want = list(zip(*[exp.columns[k].to_list() for k in ("name", "description", "sequence", "quality_scores")]))
    rel = con.table_function("read_fastq", str(p))
    assert rel.count() == len(want) == 400
    assert rel.fetchall() == want
