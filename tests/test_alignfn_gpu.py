"""exg_align_score on the GPU: gap-affine global alignment scores of two duckdb::string_t columns in HBM against
tests/align_ref.py (a plain Gotoh DP in numpy that shares nothing with the library).  Every comparison is exact, float bits
included; no row is left out.  The oracle's results are cached per (text, pattern, parameters): the 8 192-byte pair costs it a
second and is used by three tests."""
import ctypes as C

import numpy as np
import pytest

import align_ref as ref
import seqfn_ref

pytestmark = pytest.mark.gpu

BASE_T, BASE_P = 1 << 40, 1 << 41
SENTINEL = -7.0
_cache = {}


def want_scores(texts, patterns, prm):
    out = np.empty(len(texts), np.float32)
    for i, (t, p) in enumerate(zip(texts, patterns)):
        key = (t or b"", p or b"", prm)
        if key not in _cache:
            _cache[key] = ref.score(t, p, *prm)
        out[i] = _cache[key]
    return out


class Launch:
    """one exg_align_score call on buffers of the test's own, sentinel-filled"""

    def __init__(self, d_text, d_tpay, d_pat, d_ppay, n, prm=ref.DEFAULTS, max_pair_bytes=0, max_penalty=0, lanes=0, valid=None,
                 workspace_bytes=None):
        import torch
        from exon_duckdb_amd import abi, device, load_library
        lib = load_library()
        self.n = n
        self.out = torch.full((max(n, 1) + 8,), SENTINEL, dtype=torch.float32, device="cuda")
        ws_bytes = int(lib.exg_align_workspace_bytes(n, max_pair_bytes, *prm)) if workspace_bytes is None else workspace_bytes
        self.ws = torch.empty(max(ws_bytes, 64) // 8 + 2, dtype=torch.int64, device="cuda")
        self.d_result = torch.full((8,), -1, dtype=torch.int64, device="cuda")
        self.valid = valid
        a = self.args = abi.AlignScoreArgs()
        a.d_text = d_text.data_ptr() if d_text is not None else None
        a.d_pattern = d_pat.data_ptr() if d_pat is not None else None
        a.d_text_payload, a.d_pattern_payload = d_tpay.data_ptr(), d_ppay.data_ptr()
        a.text_payload_base, a.pattern_payload_base = BASE_T, BASE_P
        a.n_rows = n
        a.mismatch, a.gap_opening, a.gap_extension = prm
        a.max_penalty, a.max_pair_bytes, a.lanes = max_penalty, max_pair_bytes, lanes
        a.d_out_float = self.out.data_ptr()
        a.d_out_valid = valid.data_ptr() if valid is not None else None
        a.d_workspace, a.workspace_bytes = self.ws.data_ptr(), ws_bytes
        a.d_result = self.d_result.data_ptr()
        a.stream = device.stream_ptr().value
        self.keep = (d_text, d_tpay, d_pat, d_ppay)
        self.rc = lib.exg_align_score(C.byref(a))
        self.message = lib.exg_last_error_message() if self.rc else b""
        self.result = abi.AlignScoreResult()
        if self.rc == 0:
            self.result_rc = lib.exg_align_result(C.c_void_p(self.d_result.data_ptr()), device.stream_ptr(), C.byref(self.result))
            self.message = lib.exg_last_error_message() if self.result_rc else b""

    def scores(self):
        host = self.out.cpu().numpy()
        assert (host[self.n:] == SENTINEL).all(), "floats written behind n_rows"
        return host[:self.n]


def upload(rows, base, **kw):
    import torch
    from exon_duckdb_amd import device
    col, payload = seqfn_ref.build_column(rows, payload_base=base, **kw)
    d_col = torch.from_numpy(col).cuda() if len(rows) else None
    return d_col, device.upload(payload.tobytes())


def run_pairs(texts, patterns, prm=ref.DEFAULTS, lanes=0, max_pair_bytes=None, tkw=None, pkw=None, **kw):
    """launch, and check everything the op owes for rows that are all admissible"""
    d_t, d_tp = upload(texts, BASE_T, **(tkw or {}))
    d_p, d_pp = upload(patterns, BASE_P, **(pkw or {}))
    longest = max([len(t or b"") + len(p or b"") for t, p in zip(texts, patterns)] + [0])
    run = Launch(d_t, d_tp, d_p, d_pp, len(texts), prm, longest if max_pair_bytes is None else max_pair_bytes, lanes=lanes, **kw)
    assert run.rc == 0 and run.result_rc == 0, run.message
    r = run.result
    assert (r.error_code, r.error_row, r.error_length, r.flags, bytes(r.pad)) == (0, 0, 0, 0, bytes(16))
    if not kw.get("max_penalty"):
        want = want_scores(texts, patterns, prm)
        got = run.scores()
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert len(bad) == 0, (bad[:8], got[bad[:8]], want[bad[:8]], texts[bad[0]][:40], patterns[bad[0]][:40])
        assert r.n_capped == 0
    return run


LADDER = [0, 1, 7, 8, 9, 12, 13, 15, 16, 17, 63, 64, 65]
LANES = [16, 32, 64]


@pytest.mark.parametrize("lanes", LANES)
def test_length_ladder_at_every_alignment(gpu, lanes):
    """identical pairs, pairs that differ only in the last byte, inlined rows (<= 12 bytes) against out-of-line rows, every
    source alignment 0..15 on either side (the two columns run through the alignments at different paces)"""
    rng = np.random.default_rng(1)
    texts, patterns = [], []
    for rep in range(16):
        for n in LADDER:
            s = ref.random_seq(rng, n)
            texts.append(s), patterns.append(s)                                   # identical
            if n:
                last = bytes([s[-1] ^ 6])
                texts.append(s), patterns.append(s[:-1] + last)                   # the last byte differs
                texts.append(s[:min(n, 12)]), patterns.append(s)                  # inlined against out-of-line
                texts.append(s), patterns.append(s[max(0, n - 11):])
    run = run_pairs(texts, patterns, lanes=lanes, tkw=dict(alignments=list(range(16))), pkw=dict(alignments=[(5 * k + 3) % 16 for k in range(16)]))
    got = run.scores()
    assert got[0] == 0 and np.signbit(got[0]) == False and (got[[i for i, (t, p) in enumerate(zip(texts, patterns)) if t == p]] == 0).all()  # noqa: E712


@pytest.mark.parametrize("lanes", LANES)
def test_extend_never_reads_past_a_strings_end(gpu, lanes):
    """the bytes BEHIND both strings of a pair are equal (the same slack follows every row of both columns): an extend that
    ignores a length then sees a longer match and scores too well"""
    rng = np.random.default_rng(2)
    slack = b"GATTACAGATTACAGATTACA"
    texts, patterns = [], []
    for n in (13, 14, 15, 16, 20, 31, 32, 33, 64, 150):
        s = ref.random_seq(rng, n)
        for k in (1, 3, 8, 9):
            texts.append(s), patterns.append(s + slack[:k])           # the pattern goes on exactly as the slack behind the text
            texts.append(s + slack[:k]), patterns.append(s)
            texts.append(s), patterns.append(s[:-k] if n - k > 12 else s)
        texts.append(s), patterns.append(s)
    run_pairs(texts, patterns, lanes=lanes, tkw=dict(slack=slack), pkw=dict(slack=slack))
    run_pairs(texts, patterns, (1, 1, 1), lanes=lanes, tkw=dict(slack=slack, lead=3), pkw=dict(slack=slack, lead=6))


def test_empty_and_null_rows(gpu):
    rng = np.random.default_rng(3)
    some = [ref.random_seq(rng, n) for n in (1, 3, 12, 13, 150)]
    run = run_pairs([b"", None] * 5 + some, some + some + [b"", None, b"", None, b""])
    assert run.scores()[0] == -(6 + 2 * 1)
    for rows in ([b""] * 1000, [None] * 1000):
        got = run_pairs(rows, rows).scores()
        assert (got.view(np.uint32) == 0).all()                      # +0.0f, not -0.0f
    assert run_pairs([b""], [b"ACG"]).scores()[0] == -12
    assert run_pairs([b"AACC"] * 2, [b"AACC", b"AAACC"]).scores().tolist() == [0.0, -8.0]       # test_align.test:24-26
    assert run_pairs([b"AACC"], [b"AAACC"], (1, 1, 1)).scores()[0] == -2


@pytest.mark.parametrize("lanes", LANES)
def test_wavefronts_wider_than_a_pairs_lanes(gpu, lanes):
    """random (unrelated) pairs of 40, 200 and 300 bytes: wavefronts wider than 16, 64 and 256 diagonals; unequal lengths"""
    rng = np.random.default_rng(4)
    texts, patterns = [], []
    for n, m in ((40, 40), (200, 200), (300, 300), (10, 300), (300, 10), (1, 200), (200, 0), (64, 65)) * 2:
        texts.append(ref.random_seq(rng, n)), patterns.append(ref.random_seq(rng, m))
    run_pairs(texts, patterns, lanes=lanes)
    run_pairs(texts, patterns, (1, 1, 1), lanes=lanes)


@pytest.mark.parametrize("prm", [(20, 2, 1), (3, 0, 2), (5, 200, 1), (2, 3, 1), (5, 40, 1), (1023, 1023, 1023), (1, 0, 1)], ids=str)
def test_ring_depths(gpu, prm):
    """ring wrap-around with the depth taken from x (20,2,1), o = 0, a ring too deep for LDS (5,200,1: 206 wavefronts of 301
    diagonals), the limits of every parameter"""
    rng = np.random.default_rng(5)
    texts, patterns = [], []
    for n in (5, 40, 150):
        for rate in (0.05, 0.3):
            s = ref.random_seq(rng, n)
            texts.append(s), patterns.append(ref.mutate(rng, s, rate))
        texts.append(ref.random_seq(rng, n)), patterns.append(ref.random_seq(rng, n + 3))
    run = run_pairs(texts, patterns, prm)
    if prm == (5, 200, 1):
        assert run.result.n_global > 0
    if prm == (2, 3, 1):
        assert run.result.n_global == 0


@pytest.fixture(scope="module")
def long_pairs():
    rng = np.random.default_rng(6)
    a = ref.random_seq(rng, 8192)
    return [(a, ref.mutate(rng, a, 0.01)), (ref.random_seq(rng, 2000), ref.random_seq(rng, 2000))]


def test_global_policy_long_pairs(gpu, long_pairs):
    """a random 2 000-byte pair and an 8 192-byte pair at 1 % divergence: wavefronts in the workspace, strings read in place"""
    texts, patterns = [t for t, _ in long_pairs], [p for _, p in long_pairs]
    run = run_pairs(texts, patterns, tkw=dict(alignments=[1, 6]), pkw=dict(alignments=[15, 2]))
    assert run.result.n_global == 2


def test_three_long_rows_among_5000_short_ones(gpu, long_pairs):
    rng = np.random.default_rng(7)
    distinct = []
    for _ in range(97):
        s = ref.random_seq(rng, 60)
        distinct.append((s, ref.mutate(rng, s, 0.05)))
    pairs = [distinct[i % 97] for i in range(5000)]
    for at in (0, 2500, 4999):
        pairs.insert(at, long_pairs[0])
    run = run_pairs([t for t, _ in pairs], [p for _, p in pairs])
    assert run.result.n_global == 3


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 100000])
def test_row_counts(gpu, n):
    rng = np.random.default_rng(8)
    distinct = []
    for k in range(257):
        s = ref.random_seq(rng, 20 + k % 30)
        distinct.append((s, ref.mutate(rng, s, 0.1)))
    pairs = [distinct[i % 257] for i in range(n)]
    run = run_pairs([t for t, _ in pairs], [p for _, p in pairs])
    if n == 0:
        assert bytes(run.result) == bytes(64)


def test_permuted_rows_and_two_launches(gpu, long_pairs):
    """the same rows permuted give the same scores; two launches are byte-identical"""
    rng = np.random.default_rng(9)
    pairs = [long_pairs[1]]
    for n in [150] * 300 + [0, 5, 13, 700]:
        s = ref.random_seq(rng, n)
        pairs.append((s, ref.mutate(rng, s, 0.04)))
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    a, b = run_pairs(texts, patterns), run_pairs(texts, patterns)
    assert a.scores().tobytes() == b.scores().tobytes() and bytes(a.result) == bytes(b.result)
    perm = rng.permutation(len(pairs))
    c = run_pairs([texts[i] for i in perm], [patterns[i] for i in perm])
    assert c.scores().tobytes() == a.scores()[perm].tobytes()


def test_max_penalty(gpu):
    """a row at exactly the cap holds its score; a row one above gets -inf, its validity bit cleared (and no other) and is
    counted"""
    import torch
    rng = np.random.default_rng(10)
    texts, patterns = [], []
    for n in [150] * 70 + [700, 13, 0]:
        s = ref.random_seq(rng, n)
        texts.append(s), patterns.append(ref.mutate(rng, s, 0.05))
    want = want_scores(texts, patterns, ref.DEFAULTS)
    pens = sorted(set(int(-w) for w in want))
    cap = pens[len(pens) // 2]                              # some rows at exactly the cap, some above
    words = (len(texts) + 63) // 64
    valid = torch.full((words + 1,), -1, dtype=torch.int64, device="cuda")
    run = run_pairs(texts, patterns, max_penalty=cap, valid=valid)
    got = run.scores()
    over = -want > cap
    assert over.any() and (-want == cap).any()
    assert np.array_equal(got[~over].view(np.uint32), want[~over].view(np.uint32))
    assert np.isneginf(got[over]).all() and run.result.n_capped == int(over.sum())
    bits = np.unpackbits(valid.cpu().numpy().view(np.uint8), bitorder="little")
    assert np.array_equal(bits[:len(texts)] == 0, over) and bits[len(texts):].all()
    # one above: cap - 1 for the rows that sat on the cap
    run = run_pairs(texts, patterns, max_penalty=cap - 1)
    assert np.isneginf(run.scores()[-want == cap]).all() and run.result.n_capped == int((-want >= cap).sum())
    assert run_pairs(texts, patterns, max_penalty=0x7FFFFFFF).result.n_capped == 0


def test_max_pair_bytes(gpu):
    """the lowest too-long row wins, with the error text"""
    from exon_duckdb_amd import abi
    rng = np.random.default_rng(11)
    texts = [ref.random_seq(rng, 150) for _ in range(400)]
    patterns = [ref.mutate(rng, s, 0.02) for s in texts]
    texts[300], texts[123], texts[124] = texts[300] + b"ACGT" * 50, texts[123] + b"A" * 150, texts[124] + b"A" * 900
    d_t, d_tp = upload(texts, BASE_T)
    d_p, d_pp = upload(patterns, BASE_P)
    limit = 320
    run = Launch(d_t, d_tp, d_p, d_pp, len(texts), max_pair_bytes=limit)
    length = len(texts[123]) + len(patterns[123])
    assert run.rc == 0 and run.result_rc == abi.EXG_E_PARSE
    r = run.result
    assert (r.error_code, r.error_row, r.error_length, r.error_limit) == (abi.EXG_PE_ALIGN_TOO_LONG, 123, length, limit)
    assert run.message == b"Alignment pair too long: %d bytes (at most %d) in row 123" % (length, limit)
    run = Launch(d_t, d_tp, d_p, d_pp, 123, max_pair_bytes=limit)
    assert run.rc == 0 and run.result_rc == 0
    assert np.array_equal(run.scores().view(np.uint32), want_scores(texts[:123], patterns[:123], ref.DEFAULTS).view(np.uint32))


def mixed_launch(lanes, valid=None):
    """one exg_align_score call over align_ref.mixed_phase_pairs() at its limits"""
    texts, patterns, _ = ref.mixed_phase_pairs()
    d_t, d_tp = upload(texts, BASE_T)
    d_p, d_pp = upload(patterns, BASE_P)
    return Launch(d_t, d_tp, d_p, d_pp, len(texts), max_pair_bytes=ref.MIXED_MAX_PAIR_BYTES, max_penalty=ref.MIXED_MAX_PENALTY, lanes=lanes,
                  valid=valid)


@pytest.mark.parametrize("lanes", LANES)
def test_pairs_in_every_phase_in_one_wave(gpu, lanes):
    """one call whose groups claim, step, end and go to the global pass at different times (at 16 and 32 lanes: inside one wave):
    scores, validity bits, n_capped, n_global and the error row are the oracle's, and a second launch is byte-identical"""
    import torch
    from exon_duckdb_amd import abi
    texts, patterns, kinds = ref.mixed_phase_pairs()
    done = (kinds != "capped") & (kinds != "long")
    want = want_scores([t for t, d in zip(texts, done) if d], [p for p, d in zip(patterns, done) if d], ref.DEFAULTS)
    capped = want_scores([t for t, k in zip(texts, kinds) if k == "capped"], [p for p, k in zip(patterns, kinds) if k == "capped"], ref.DEFAULTS)
    assert (-want <= ref.MIXED_MAX_PENALTY).all() and (-capped > ref.MIXED_MAX_PENALTY).all() and (want[kinds[done] == "same"] == 0).all()
    valid = torch.full((len(texts) // 64 + 2,), -1, dtype=torch.int64, device="cuda")
    run = mixed_launch(lanes, valid)
    first_long = int(np.flatnonzero(kinds == "long")[0])
    length = len(texts[first_long]) + len(patterns[first_long])
    assert length > ref.MIXED_MAX_PAIR_BYTES and run.rc == 0 and run.result_rc == abi.EXG_E_PARSE
    r = run.result
    assert (r.error_code, r.error_row, r.error_length, r.error_limit, r.flags) == (abi.EXG_PE_ALIGN_TOO_LONG, first_long, length, ref.MIXED_MAX_PAIR_BYTES, 0)
    assert (r.n_capped, r.n_global) == (4, 3)
    got = run.scores()
    assert np.array_equal(got[done].view(np.uint32), want.view(np.uint32))
    assert np.isneginf(got[kinds == "capped"]).all() and (got[kinds == "long"] == SENTINEL).all()
    bits = np.unpackbits(valid.cpu().numpy().view(np.uint8), bitorder="little")
    assert np.array_equal(bits[:len(texts)] == 0, kinds == "capped") and bits[len(texts):].all()
    again = mixed_launch(lanes)
    assert again.scores().tobytes() == got.tobytes() and bytes(again.result) == bytes(r)


def fastq(reads):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(reads))


def test_behind_the_fastq_scans(gpu, tmp_path):
    """two small generated FASTQ files, reads and mutated reads, through exg_fastq_scan; the two sequence columns aligned where
    the scans left them (pointers into the two inputs)"""
    from exon_duckdb_amd import device
    rng = np.random.default_rng(12)
    reads = [ref.random_seq(rng, 150 if i % 10 else 9 + i % 7) for i in range(600)]
    mutated = [ref.mutate(rng, s, 0.05 if i % 2 else 0.01) or b"A" for i, s in enumerate(reads)]
    scans = []
    for name, rows in (("reads.fastq", reads), ("mutated.fastq", mutated)):
        path = tmp_path / name
        path.write_bytes(fastq(rows))
        data = path.read_bytes()
        d_in = device.upload(data)
        scan = device.FastqScan(len(data))
        scan.launch(d_in, payload_base=BASE_T)
        res = scan.fetch()
        assert res.error_code == 0 and res.n_records == len(rows)
        scans.append((scan, d_in))
    (sa, da), (sb, db) = scans
    got, r = device.align_score(sa.cols[2], da, BASE_T, sb.cols[2], db, BASE_T, len(reads), 400)
    want = want_scores(reads, mutated, ref.DEFAULTS)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)) and r.n_capped == 0 and r.n_global == 0


def test_device_host_scalar_and_oracle_agree(gpu, long_pairs):
    from exon_duckdb_amd import table_function
    rng = np.random.default_rng(13)
    pairs = [long_pairs[1], (b"", b""), (None, b"ACGT"), (b"AACC", b"AAACC"), (b"acgt", b"ACGT"), (b"NNNN", b"NNNN"), (bytes(range(256)), bytes(range(1, 256)))]
    for n in (7, 13, 64, 150, 301):
        s = ref.random_seq(rng, n, b"ACGTN")
        pairs.append((s, ref.mutate(rng, s, 0.1)))
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    for prm in ((4, 6, 2), (2, 3, 1)):
        got = run_pairs(texts, patterns, prm).scores()
        for i, (t, p) in enumerate(pairs):
            host = table_function.alignment_score(t or b"", p or b"", *prm, "memory_high")
            assert np.float32(host).tobytes() == got[i].tobytes() == want_scores([t], [p], prm)[0].tobytes(), i
    assert got[4] == -8 and got[5] == 0                    # (2,3,1): case-sensitive, four mismatches; N equals N


def test_argument_errors(gpu):
    from exon_duckdb_amd import abi
    d_t, d_tp = upload([b"ACGT" * 10, b"AC"], BASE_T)
    d_p, d_pp = upload([b"ACGT" * 9, b"AC"], BASE_P)
    ok = Launch(d_t, d_tp, d_p, d_pp, 2, max_pair_bytes=100)
    assert ok.rc == 0 and ok.result_rc == 0
    for run in (Launch(None, d_tp, d_p, d_pp, 2, max_pair_bytes=100), Launch(d_t, d_tp, None, d_pp, 2, max_pair_bytes=100),
                Launch(d_t, d_tp, d_p, d_pp, 2, (0, 6, 2), 100, workspace_bytes=1 << 20), Launch(d_t, d_tp, d_p, d_pp, 2, (4, 1024, 2), 100, workspace_bytes=1 << 20),
                Launch(d_t, d_tp, d_p, d_pp, 2, (4, 6, 0), 100, workspace_bytes=1 << 20), Launch(d_t, d_tp, d_p, d_pp, 2, max_pair_bytes=(1 << 21) + 1, workspace_bytes=1 << 20),
                Launch(d_t, d_tp, d_p, d_pp, 2, max_pair_bytes=100, lanes=8),
                Launch(d_t, d_tp, d_p, d_pp, 2, max_pair_bytes=100, workspace_bytes=ok.args.workspace_bytes - 8)):
        assert run.rc == abi.EXG_E_INVALID_ARG and run.message.startswith(b"exg_align_score: ")
        assert (run.out.cpu().numpy() == SENTINEL).all() and (run.d_result.cpu().numpy() == -1).all()
