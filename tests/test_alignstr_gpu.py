"""exg_align_string on the GPU: the CIGARs of two duckdb::string_t columns in HBM.  Every case compares the device's two output
arrays BYTE FOR BYTE with the output contract built from tests/alignstr_ref.py (plain Python, dicts; shares nothing with the
library) and that oracle with the host scalar the shim registers: device == oracle == host scalar, no row left out.  The
oracle's results are cached per (text, pattern, parameters)."""
import ctypes as C

import numpy as np
import pytest

import align_ref
import alignstr_ref as ref
import seqfn_ref

pytestmark = pytest.mark.gpu

BASE_T, BASE_P, OUT_BASE = 1 << 40, 1 << 41, 1 << 47
GUARD, GUARD_BYTE = 64, 0xA5
SENTINEL = -7.0
LANES = [16, 32, 64]
_cache = {}


def oracle(texts, patterns, prm):
    """[(CIGAR, penalty)]: oracle (a) for every row; once per distinct pair it is held against check (b), which also gives the
    penalty, and against the host scalar"""
    from exon_duckdb_amd import table_function
    out = []
    for t, p in zip(texts, patterns):
        key = (t or b"", p or b"", prm)
        if key not in _cache:
            c = ref.cigar(t, p, *prm)
            assert table_function.alignment_string(t or b"", p or b"", *prm, "memory_high") == c, key
            _cache[key] = (c, ref.check(t, p, c, *prm))
        out.append(_cache[key])
    return out


def want_cigars(texts, patterns, prm):
    return [c for c, _ in oracle(texts, patterns, prm)]


def want_pens(texts, patterns, prm):
    return np.array([pen for _, pen in oracle(texts, patterns, prm)], np.int64)


class Launch:
    """one exg_align_string call on buffers of the test's own: sentinels in the outputs, guard bytes behind out_capacity"""

    def __init__(self, d_text, d_tpay, d_pat, d_ppay, n, prm=align_ref.DEFAULTS, max_pair_bytes=0, max_penalty=0, lanes=0, valid=None,
                 out_capacity=0, score=True, workspace_bytes=None, strings_offset=0):
        import torch
        from exon_duckdb_amd import abi, device, load_library
        lib = load_library()
        self.n, self.cap = n, out_capacity
        self.strings = torch.full(((max(n, 1) + 2) * 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.payload = torch.full((out_capacity + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.score = torch.full((max(n, 1) + 8,), SENTINEL, dtype=torch.float32, device="cuda")
        ws_bytes = int(lib.exg_align_string_workspace_bytes(n, max_pair_bytes, *prm, max_penalty, out_capacity)) if workspace_bytes is None else workspace_bytes
        self.ws = torch.empty(max(ws_bytes, 64) // 8 + 2, dtype=torch.int64, device="cuda")
        self.d_result = torch.full((8,), -1, dtype=torch.int64, device="cuda")
        self.valid = valid
        a = self.args = abi.AlignStringArgs()
        a.d_text = d_text.data_ptr() if d_text is not None else None
        a.d_pattern = d_pat.data_ptr() if d_pat is not None else None
        a.d_text_payload, a.d_pattern_payload = d_tpay.data_ptr(), d_ppay.data_ptr()
        a.text_payload_base, a.pattern_payload_base = BASE_T, BASE_P
        a.n_rows = n
        a.mismatch, a.gap_opening, a.gap_extension = prm
        a.max_penalty, a.max_pair_bytes, a.lanes = max_penalty, max_pair_bytes, lanes
        a.d_out_strings, a.d_out_payload = self.strings.data_ptr() + strings_offset, self.payload.data_ptr()
        a.out_capacity, a.out_payload_base = out_capacity, OUT_BASE
        a.d_out_score = self.score.data_ptr() if score else None
        a.d_out_valid = valid.data_ptr() if valid is not None else None
        a.d_workspace, a.workspace_bytes = self.ws.data_ptr(), ws_bytes
        a.d_result = self.d_result.data_ptr()
        a.stream = device.stream_ptr().value
        self.keep = (d_text, d_tpay, d_pat, d_ppay)
        self.rc = lib.exg_align_string(C.byref(a))
        self.message = lib.exg_last_error_message() if self.rc else b""
        self.result = abi.AlignStringResult()
        if self.rc == 0:
            self.result_rc = lib.exg_align_string_result(C.c_void_p(self.d_result.data_ptr()), device.stream_ptr(), C.byref(self.result))
            self.message = lib.exg_last_error_message() if self.result_rc else b""

    def outputs(self):
        """(string_t rows [n, 16] uint8, payload [out_capacity] uint8); nothing may be written behind either"""
        s, p = self.strings.cpu().numpy(), self.payload.cpu().numpy()
        assert (s[16 * self.n:] == GUARD_BYTE).all(), "strings written behind n_rows"
        assert (p[self.cap:] == GUARD_BYTE).all(), "payload written at or behind out_capacity"
        return s[:16 * self.n].reshape(self.n, 16), p[:self.cap]

    def scores(self):
        host = self.score.cpu().numpy()
        assert (host[self.n:] == SENTINEL).all(), "floats written behind n_rows"
        return host[:self.n]


def upload(rows, base, **kw):
    import torch
    from exon_duckdb_amd import device
    col, payload = seqfn_ref.build_column(rows, payload_base=base, **kw)
    d_col = torch.from_numpy(col).cuda() if len(rows) else None
    return d_col, device.upload(payload.tobytes())


def pair_bytes(texts, patterns):
    return [len(t or b"") + len(p or b"") for t, p in zip(texts, patterns)]


def check_outputs(run, want):
    """the output contract, byte for byte: inlined rows zero padded, long rows {length, prefix, OUT_BASE + prefix sum}, the
    payload packed in row order, out_bytes exact"""
    col, payload = seqfn_ref.expected_column(want, OUT_BASE)
    got_col, got_payload = run.outputs()
    assert run.result.out_bytes == len(payload)
    bad = np.flatnonzero((got_col != col).any(axis=1))
    assert len(bad) == 0, (bad[:8], bytes(got_col[bad[0]]), bytes(col[bad[0]]), want[bad[0]])
    assert got_payload[:len(payload)].tobytes() == payload.tobytes()
    assert (got_payload[len(payload):] == GUARD_BYTE).all(), "payload written behind out_bytes"


def run_pairs(texts, patterns, prm=align_ref.DEFAULTS, lanes=0, max_pair_bytes=None, tkw=None, pkw=None, out_capacity=None, some_capped=False, **kw):
    """launch, and check everything the op owes for rows that are all admissible (some_capped: the caller checks the rows)"""
    d_t, d_tp = upload(texts, BASE_T, **(tkw or {}))
    d_p, d_pp = upload(patterns, BASE_P, **(pkw or {}))
    lens = pair_bytes(texts, patterns)
    run = Launch(d_t, d_tp, d_p, d_pp, len(texts), prm, max(lens + [0]) if max_pair_bytes is None else max_pair_bytes, lanes=lanes,
                 out_capacity=2 * sum(lens) if out_capacity is None else out_capacity, **kw)
    assert run.rc == 0 and run.result_rc == 0, run.message
    r = run.result
    assert (r.error_code, r.error_row, r.error_length, r.flags) == (0, 0, 0, 0)
    if not some_capped:
        check_outputs(run, want_cigars(texts, patterns, prm))
        assert r.n_capped == 0
        if kw.get("score", True):
            assert np.array_equal(run.scores().view(np.uint32), (-want_pens(texts, patterns, prm)).astype(np.float32).view(np.uint32))
    return run


def test_pins_empty_and_null_rows(gpu):
    texts = [b"AACC", b"AAA", b"", b"ACG", b"ACGT", b"", None, None, b"ACG", b"AACC"]
    patterns = [b"AAACC", b"AAAA", b"ACG", b"", b"AGGT", b"", b"ACG", None, None, b"AACC"]
    want = [b"2M1D2M", b"3M1D", b"3D", b"3I", b"1M1X2M", b"", b"3D", b"", b"3I", b"4M"]
    run = run_pairs(texts, patterns)
    assert want_cigars(texts, patterns, align_ref.DEFAULTS) == want
    assert seqfn_ref.decode_column(*run.outputs(), OUT_BASE) == want
    assert run.scores().view(np.uint32)[5] == 0                           # +0.0f for the empty pair
    run = run_pairs(texts[:1], patterns[:1], (1, 1, 1))                   # (1,1,1,'memory_low')
    assert seqfn_ref.decode_column(*run.outputs(), OUT_BASE) == [b"2M1D2M"]
    run = run_pairs(texts[:1], patterns[:1], ref.fold(-1, 1, 2, 3))       # (-1,1,2,3,'memory_low'): the folded penalties
    assert seqfn_ref.decode_column(*run.outputs(), OUT_BASE) == [b"2M1D2M"]
    for rows in ([b""] * 1000, [None] * 1000):
        run = run_pairs(rows, rows)
        assert not run.outputs()[0].any() and run.result.out_bytes == 0


@pytest.mark.parametrize("lanes", LANES)
def test_length_ladder(gpu, lanes):
    """every n, m in 0..20 and 60..68 (900 related pairs), both payloads at byte offsets 0..3; prefix pairs whose slack goes on
    as the partner does, so that an extend that ignores a length sees a longer match; in the second launch there is no slack
    and the last strings end flush with their buffers"""
    rng = np.random.default_rng(1)
    ladder = list(range(21)) + list(range(60, 69))
    slack = b"GATTACAGATTACAGATTACA"
    texts, patterns = [], []
    for n in ladder:
        for m in ladder:
            s = align_ref.random_seq(rng, max(n, m))
            texts.append(s[:n]), patterns.append((align_ref.mutate(rng, s, 0.15) + align_ref.random_seq(rng, m))[:m])
        t = align_ref.random_seq(rng, n, b"AC")
        texts.append(t + slack[:3]), patterns.append(t)                                    # the slack behind p goes on as t does
        texts.append(t), patterns.append(t + slack[:9])
        texts.append(t), patterns.append(t[:n // 2])
    run_pairs(texts, patterns, lanes=lanes, tkw=dict(alignments=[0, 1, 2, 3], slack=slack), pkw=dict(alignments=[3, 1, 0, 2], slack=slack))
    run_pairs(texts, patterns, (1, 1, 1), lanes=lanes, tkw=dict(lead=3), pkw=dict(lead=6))   # no slack: flush with the buffer


def tie_pairs(prm):
    rng = np.random.default_rng(100 + sum(prm))
    return [(align_ref.random_seq(rng, int(rng.integers(0, 25)), b"AC"), align_ref.random_seq(rng, int(rng.integers(0, 25)), b"AC"))
            for _ in range(400)]


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("prm", [(4, 6, 2), (2, 0, 1), (1, 0, 1), (5, 40, 1)], ids=str)
def test_ties(gpu, prm, lanes):
    """the 400 low-complexity pairs of the host test: optima are rarely unique, the rule decides"""
    pairs = tie_pairs(prm)
    run_pairs([t for t, _ in pairs], [p for _, p in pairs], prm, lanes=lanes)


def test_score_output_equals_exg_align_score(gpu):
    """d_out_score is bit for bit what exg_align_score gives on the tie set; without d_out_score nothing else changes"""
    from exon_duckdb_amd import device
    pairs = tie_pairs((4, 6, 2))
    texts, patterns = [t for t, _ in pairs], [p for _, p in pairs]
    run = run_pairs(texts, patterns)
    (d_t, d_tp, d_p, d_pp) = run.keep
    scores, r = device.align_score(d_t, d_tp, BASE_T, d_p, d_pp, BASE_P, len(pairs), 48)
    assert scores.cpu().numpy().tobytes() == run.scores().tobytes() and r.n_capped == 0
    bare = run_pairs(texts, patterns, score=False)
    assert bare.strings.cpu().numpy().tobytes() == run.strings.cpu().numpy().tobytes() and (bare.score.cpu().numpy() == SENTINEL).all()


@pytest.mark.parametrize("lanes", LANES)
def test_wavefronts_wider_than_a_pairs_lanes(gpu, lanes):
    """200 bytes against 40 and 40 against 200; one pair of unrelated 150-byte strings: the worst case of the history bound at
    max_penalty = 0"""
    rng = np.random.default_rng(4)
    texts = [align_ref.random_seq(rng, n) for n in (200, 40, 150)]
    patterns = [align_ref.random_seq(rng, n) for n in (40, 200, 150)]
    run_pairs(texts, patterns, lanes=lanes)


@pytest.mark.parametrize("prm", [(20, 2, 1), (3, 0, 2), (5, 200, 1), (2, 3, 1), (5, 40, 1), (1023, 1023, 1023), (1, 0, 1)], ids=str)
def test_ring_depths(gpu, prm):
    """the parameter list of the score's test_ring_depths on 30 pairs of 0..60 bytes"""
    rng = np.random.default_rng(5)
    texts, patterns = [], []
    for it in range(30):
        s = align_ref.random_seq(rng, int(rng.integers(0, 61)))
        texts.append(s)
        patterns.append(align_ref.mutate(rng, s, 0.05 if it % 2 else 0.3) if it % 3 else align_ref.random_seq(rng, int(rng.integers(0, 61))))
    run = run_pairs(texts, patterns, prm)
    if prm == (2, 3, 1):
        assert run.result.n_global == 0


@pytest.fixture(scope="module")
def long_pairs():
    """three pairs of about 1 500 + 1 500 bytes at 2 %: a ring of 15 wavefronts of 3 000 diagonals does not fit a pair's LDS"""
    rng = np.random.default_rng(6)
    out = []
    for n in (1500, 1480, 1530):
        a = align_ref.random_seq(rng, n)
        out.append((a, align_ref.mutate(rng, a, 0.02)))
    return out


def test_global_policy(gpu, long_pairs):
    """a cap above every row's penalty keeps the history slots small; no row is capped"""
    texts, patterns = [t for t, _ in long_pairs], [p for _, p in long_pairs]
    assert want_pens(texts, patterns, align_ref.DEFAULTS).max() < 400
    run = run_pairs(texts, patterns, tkw=dict(alignments=[1, 6, 11]), pkw=dict(alignments=[15, 2, 5]), max_pair_bytes=3100, max_penalty=400)
    assert run.result.n_global == 3
    run = run_pairs(texts[:1], patterns[:1], max_pair_bytes=3100)          # and without a cap: the slot of the bound, 87 MB
    assert run.result.n_global == 1


def test_long_rows_among_2000_short_ones(gpu, long_pairs):
    rng = np.random.default_rng(7)
    distinct = []
    for _ in range(97):
        s = align_ref.random_seq(rng, 60)
        distinct.append((s, align_ref.mutate(rng, s, 0.05)))
    pairs = [distinct[i % 97] for i in range(2000)]
    for at, pair in zip((0, 1000, 2002), long_pairs):
        pairs.insert(at, pair)
    run = run_pairs([t for t, _ in pairs], [p for _, p in pairs], max_pair_bytes=3100, max_penalty=400)
    assert run.result.n_global == 3


@pytest.fixture(scope="module")
def mixed_rows():
    """300 rows whose CIGARs mix the inlined (<= 12 bytes) with longer ones, 13 bytes among them"""
    rng = np.random.default_rng(8)
    texts, patterns = [], []
    for i in range(300):
        s = align_ref.random_seq(rng, int(rng.integers(0, 120)))
        texts.append(s), patterns.append(align_ref.mutate(rng, s, (0.0, 0.02, 0.1, 0.3)[i % 4]))
    for n in (27, 32):                                   # 10M1X10M1X5M is 12 bytes, 10M1X10M1X10M is 13
        s = bytearray(align_ref.random_seq(rng, n))
        texts.append(bytes(s))
        s[10] ^= 6
        s[21] ^= 6
        patterns.append(bytes(s))
    return texts, patterns


def test_payload_placement(gpu, mixed_rows):
    from exon_duckdb_amd import abi
    texts, patterns = mixed_rows
    want = want_cigars(texts, patterns, align_ref.DEFAULTS)
    lens = np.array([len(c) for c in want])
    assert (lens <= 12).sum() > 30 and (lens > 12).sum() > 100 and want[-2:] == [b"10M1X10M1X5M", b"10M1X10M1X10M"]
    out_bytes = int(lens[lens > 12].sum())
    run = run_pairs(texts, patterns)                                          # the capacity that can never overflow
    rows = run.outputs()[0]
    ptrs = rows[:, 8:].copy().view(np.uint64)[:, 0]
    offsets = np.cumsum(np.where(lens > 12, lens, 0)) - np.where(lens > 12, lens, 0)
    for r in np.flatnonzero(lens > 12):
        assert ptrs[r] == OUT_BASE + offsets[r] and rows[r, 4:8].tobytes() == want[r][:4]
    assert run.result.out_bytes == out_bytes
    exact = run_pairs(texts, patterns, out_capacity=out_bytes)                # exactly enough: the guard sits right behind
    assert exact.strings.cpu().numpy().tobytes() == run.strings.cpu().numpy().tobytes()
    # one byte short: an error that reports the same out_bytes and leaves the guard alone
    d_t, d_tp = upload(texts, BASE_T)
    d_p, d_pp = upload(patterns, BASE_P)
    short = Launch(d_t, d_tp, d_p, d_pp, len(texts), max_pair_bytes=max(pair_bytes(texts, patterns)), out_capacity=out_bytes - 1)
    assert short.rc == 0 and short.result_rc == abi.EXG_E_CAPACITY
    assert short.message == b"exg_align_string: the CIGARs take %d payload bytes, out_capacity is %d" % (out_bytes, out_bytes - 1)
    assert short.result.out_bytes == out_bytes and short.result.flags == 0 and short.result.error_code == 0
    short.outputs()
    none = Launch(d_t, d_tp, d_p, d_pp, len(texts), max_pair_bytes=max(pair_bytes(texts, patterns)), out_capacity=0)
    assert none.result_rc == abi.EXG_E_CAPACITY and none.result.out_bytes == out_bytes
    none.outputs()


def test_permuted_rows_and_two_launches(gpu, mixed_rows):
    """permuted rows give the same strings; two launches are byte-identical in d_out_strings and d_out_payload"""
    texts, patterns = mixed_rows
    a, b = run_pairs(texts, patterns), run_pairs(texts, patterns)
    assert a.strings.cpu().numpy().tobytes() == b.strings.cpu().numpy().tobytes()
    assert a.payload.cpu().numpy().tobytes() == b.payload.cpu().numpy().tobytes() and bytes(a.result) == bytes(b.result)
    perm = np.random.default_rng(9).permutation(len(texts))
    c = run_pairs([texts[i] for i in perm], [patterns[i] for i in perm])
    got = seqfn_ref.decode_column(*c.outputs(), OUT_BASE)
    assert got == [seqfn_ref.decode_column(*a.outputs(), OUT_BASE)[i] for i in perm]


def test_max_penalty(gpu):
    """rows below, at and above the cap: a row at exactly the cap keeps its CIGAR; a row above is NULL (16 zero bytes), has its
    validity bit cleared (and no other), -inf as its score and is counted"""
    import torch
    rng = np.random.default_rng(10)
    texts, patterns = [], []
    for n in [150] * 70 + [300, 13, 0]:
        s = align_ref.random_seq(rng, n)
        texts.append(s), patterns.append(align_ref.mutate(rng, s, 0.05))
    cigars, pens = want_cigars(texts, patterns, align_ref.DEFAULTS), want_pens(texts, patterns, align_ref.DEFAULTS)
    cap = int(sorted(set(pens))[len(set(pens)) // 2])
    over = pens > cap
    assert over.any() and (pens == cap).any() and (pens < cap).any()
    for limit, gone in ((cap, over), (cap - 1, pens >= cap)):
        valid = torch.full(((len(texts) + 63) // 64 + 1,), -1, dtype=torch.int64, device="cuda")
        run = run_pairs(texts, patterns, max_penalty=limit, valid=valid, some_capped=True)
        want = [b"" if g else c for g, c in zip(gone, cigars)]
        check_outputs(run, want)
        assert not run.outputs()[0][gone].any() and run.result.n_capped == int(gone.sum()) and run.result.flags == 0
        bits = np.unpackbits(valid.cpu().numpy().view(np.uint8), bitorder="little")
        assert np.array_equal(bits[:len(texts)] == 0, gone) and bits[len(texts):].all()
        scores = run.scores()
        assert np.isneginf(scores[gone]).all() and np.array_equal(scores[~gone], -pens[~gone].astype(np.float32))
    run_pairs(texts, patterns, max_penalty=0x7FFFFFFF)


def test_max_pair_bytes(gpu):
    """the lowest too-long row wins, with the score's error text"""
    from exon_duckdb_amd import abi
    rng = np.random.default_rng(11)
    texts = [align_ref.random_seq(rng, 150) for _ in range(400)]
    patterns = [align_ref.mutate(rng, s, 0.02) for s in texts]
    texts[300], texts[123], texts[124] = texts[300] + b"ACGT" * 50, texts[123] + b"A" * 150, texts[124] + b"A" * 900
    d_t, d_tp = upload(texts, BASE_T)
    d_p, d_pp = upload(patterns, BASE_P)
    limit = 320
    run = Launch(d_t, d_tp, d_p, d_pp, len(texts), max_pair_bytes=limit, out_capacity=1 << 16)
    length = len(texts[123]) + len(patterns[123])
    assert run.rc == 0 and run.result_rc == abi.EXG_E_PARSE
    r = run.result
    assert (r.error_code, r.error_row, r.error_length, r.error_limit, r.flags) == (abi.EXG_PE_ALIGN_TOO_LONG, 123, length, limit, 0)
    assert run.message == b"Alignment pair too long: %d bytes (at most %d) in row 123" % (length, limit)
    run.outputs()
    run = Launch(d_t, d_tp, d_p, d_pp, 123, max_pair_bytes=limit, out_capacity=1 << 16)
    assert run.rc == 0 and run.result_rc == 0 and run.result.flags == 0
    check_outputs(run, want_cigars(texts[:123], patterns[:123], align_ref.DEFAULTS))


@pytest.mark.parametrize("lanes", LANES)
def test_pairs_in_every_phase_in_one_wave(gpu, lanes):
    """one call over align_ref.mixed_phase_pairs(), whose groups claim, step, trace, end and go to the global pass at different
    times (at 16 and 32 lanes: inside one wave): every string_t, the payload, out_bytes, the scores, validity bits, n_capped,
    n_global and the error row are the oracle's; exg_align_score gives the same scores; a second launch is byte-identical"""
    import torch
    import test_alignfn_gpu as score_suite
    from exon_duckdb_amd import abi
    texts, patterns, kinds = align_ref.mixed_phase_pairs()
    limit, cap = align_ref.MIXED_MAX_PAIR_BYTES, align_ref.MIXED_MAX_PENALTY
    done = (kinds != "capped") & (kinds != "long")
    found = iter(oracle([t for t, d in zip(texts, done) if d], [p for p, d in zip(patterns, done) if d], align_ref.DEFAULTS))
    want = [next(found) if d else (b"", None) for d in done]
    pens = np.array([pen for (_, pen), d in zip(want, done) if d], np.int64)
    assert (pens <= cap).all() and all(align_ref.penalty(t, p) > cap for t, p, k in zip(texts, patterns, kinds) if k == "capped")
    d_t, d_tp = upload(texts, BASE_T)
    d_p, d_pp = upload(patterns, BASE_P)

    def launch(valid=None):
        return Launch(d_t, d_tp, d_p, d_pp, len(texts), max_pair_bytes=limit, max_penalty=cap, lanes=lanes, valid=valid, out_capacity=1 << 16)

    valid = torch.full((len(texts) // 64 + 2,), -1, dtype=torch.int64, device="cuda")
    run = launch(valid)
    first_long = int(np.flatnonzero(kinds == "long")[0])
    length = len(texts[first_long]) + len(patterns[first_long])
    assert run.rc == 0 and run.result_rc == abi.EXG_E_PARSE
    r = run.result
    assert (r.error_code, r.error_row, r.error_length, r.error_limit, r.flags) == (abi.EXG_PE_ALIGN_TOO_LONG, first_long, length, limit, 0)
    assert (r.n_capped, r.n_global, r.out_capacity) == (4, 3, 1 << 16)
    check_outputs(run, [c for c, _ in want])
    assert not run.outputs()[0][~done].any()
    got = run.scores()
    assert np.array_equal(got[done].view(np.uint32), (-pens).astype(np.float32).view(np.uint32))
    assert np.isneginf(got[kinds == "capped"]).all() and (got[kinds == "long"] == SENTINEL).all()
    bits = np.unpackbits(valid.cpu().numpy().view(np.uint8), bitorder="little")
    assert np.array_equal(bits[:len(texts)] == 0, kinds == "capped") and bits[len(texts):].all()
    assert score_suite.mixed_launch(lanes).scores().tobytes() == got.tobytes()
    again = launch()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again.outputs(), run.outputs()))
    assert again.scores().tobytes() == got.tobytes() and bytes(again.result) == bytes(r)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 100000])
def test_row_counts(gpu, n):
    rng = np.random.default_rng(12)
    distinct = []
    for k in range(257):
        s = align_ref.random_seq(rng, 20 + k % 30)
        distinct.append((s, align_ref.mutate(rng, s, 0.1)))
    pairs = [distinct[i % 257] for i in range(n)]
    run = run_pairs([t for t, _ in pairs], [p for _, p in pairs], max_pair_bytes=120)
    if n == 0:
        assert bytes(run.result) == bytes(64)


def fastq(reads):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(reads))


def test_behind_the_scans_and_into_parse_cigar(gpu, tmp_path):
    """the sequence column of exg_fastq_scan of 2 000 reads against a mutated copy, aligned where the scans left them; the result
    column goes to exg_cigar_op(EXG_CIGAR_PARSE) without leaving the device, and its operations re-render to the same strings"""
    from exon_duckdb_amd import device
    rng = np.random.default_rng(13)
    reads = [align_ref.random_seq(rng, 150 if i % 10 else 9 + i % 7) for i in range(2000)]
    mutated = [align_ref.mutate(rng, s, 0.05 if i % 2 else 0.01) or b"A" for i, s in enumerate(reads)]
    scans = []
    for name, rows in (("reads.fastq", reads), ("mutated.fastq", mutated)):
        data = fastq(rows)
        d_in = device.upload(data)
        scan = device.FastqScan(len(data))
        scan.launch(d_in, payload_base=BASE_T)
        res = scan.fetch()
        assert res.error_code == 0 and res.n_records == len(rows)
        scans.append((scan, d_in))
    (sa, da), (sb, db) = scans
    n = len(reads)
    strings, payload, scores, r = device.align_string(sa.cols[2], da, BASE_T, sb.cols[2], db, BASE_T, n, 400,
                                                      2 * sum(pair_bytes(reads, mutated)), want_score=True)
    want = want_cigars(reads, mutated, align_ref.DEFAULTS)
    assert (r.flags, r.n_capped, r.n_global, r.error_code) == (0, 0, 0, 0)
    col = strings.cpu().numpy().view(np.uint8).reshape(n, 16)
    assert seqfn_ref.decode_column(col, payload.cpu().numpy(), device.ALIGN_OUT_BASE) == want
    assert r.out_bytes == sum(len(c) for c in want if len(c) > 12) == payload.numel()
    entries, op, length, pr = device.parse_cigar(strings, n, payload, device.ALIGN_OUT_BASE)
    assert pr.error_code == 0 and pr.flags == 0
    ent = entries.cpu().numpy().astype(np.int64)
    letters = op.cpu().numpy().view(np.uint8).reshape(-1, 16)[:, 4].tobytes()
    lens = length.cpu().numpy()
    for k in range(n):
        o, c = ent[k]
        assert b"".join(b"%d%c" % (lens[i], letters[i]) for i in range(o, o + c)) == want[k], k


def test_argument_errors(gpu):
    from exon_duckdb_amd import abi
    d_t, d_tp = upload([b"ACGT" * 10, b"AC"], BASE_T)
    d_p, d_pp = upload([b"ACGT" * 9, b"AC"], BASE_P)
    ok = Launch(d_t, d_tp, d_p, d_pp, 2, max_pair_bytes=100, out_capacity=256)
    assert ok.rc == 0 and ok.result_rc == 0 and ok.result.flags == 0
    kw = dict(max_pair_bytes=100, out_capacity=256)
    for run in (Launch(None, d_tp, d_p, d_pp, 2, **kw), Launch(d_t, d_tp, None, d_pp, 2, **kw),
                Launch(d_t, d_tp, d_p, d_pp, 2, (0, 6, 2), workspace_bytes=1 << 20, **kw),
                Launch(d_t, d_tp, d_p, d_pp, 2, (4, 1024, 2), workspace_bytes=1 << 20, **kw),
                Launch(d_t, d_tp, d_p, d_pp, 2, (4, 6, 0), workspace_bytes=1 << 20, **kw),
                Launch(d_t, d_tp, d_p, d_pp, 2, max_pair_bytes=(1 << 21) + 1, out_capacity=256, workspace_bytes=1 << 20),
                Launch(d_t, d_tp, d_p, d_pp, 2, lanes=8, **kw), Launch(d_t, d_tp, d_p, d_pp, 2, strings_offset=8, **kw),
                Launch(d_t, d_tp, d_p, d_pp, 2, workspace_bytes=ok.args.workspace_bytes - 8, **kw)):
        assert run.rc == abi.EXG_E_INVALID_ARG and run.message.startswith(b"exg_align_string: ")
        assert (run.strings.cpu().numpy() == GUARD_BYTE).all() and (run.payload.cpu().numpy() == GUARD_BYTE).all()
        assert (run.score.cpu().numpy() == SENTINEL).all() and (run.d_result.cpu().numpy() == -1).all()
