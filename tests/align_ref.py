"""The oracle of the alignment scores: a plain Gotoh dynamic programme over the whole n x m matrix, in numpy.  It shares nothing
with the library (no wavefronts, no diagonals): three penalties per cell,

    F[i][j] = min(H[i-1][j] + o + e, F[i-1][j] + e)                 a gap that consumes pattern bytes
    E[i][j] = min(H[i][j-1] + o + e, E[i][j-1] + e)                 a gap that consumes text bytes
    H[i][j] = min(H[i-1][j-1] + (0 if equal else x), E[i][j], F[i][j])

row by row.  Inside a row E depends on H of the same row; for o >= 0 opening a gap inside a gap never pays, so
E[j] = e * j + min over j' < j of (tmp[j'] + o - e * j') with tmp = min(diagonal, F): one running minimum.
score = float32(-H[m][n]); a NULL (None) string is an empty one."""
import numpy as np

DEFAULTS = (4, 6, 2)
PARAM_SETS = [(4, 6, 2), (1, 1, 1), (2, 3, 1), (20, 2, 1), (3, 0, 2), (5, 40, 1)]
INF = 1 << 60


def penalty(text, pattern, x=4, o=6, e=2):
    t = np.frombuffer(text or b"", np.uint8)
    p = np.frombuffer(pattern or b"", np.uint8)
    n = len(t)
    j = np.arange(n + 1, dtype=np.int64)
    h = o + e * j
    h[0] = 0
    f = np.full(n + 1, INF, np.int64)
    for c in p:
        f = np.minimum(h + (o + e), f + e)
        tmp = f.copy()
        np.minimum(tmp[1:], h[:-1] + np.where(t == c, 0, x), out=tmp[1:])
        run = np.minimum.accumulate(tmp + o - e * j)
        h = tmp
        np.minimum(h[1:], e * j[1:] + run[:-1], out=h[1:])
    return int(h[n])


def penalty_scalar(text, pattern, x=4, o=6, e=2):
    """the same recurrences cell by cell (checks the running-minimum form in the host tests)"""
    t, p = text or b"", pattern or b""
    n, m = len(t), len(p)
    H = [[INF] * (n + 1) for _ in range(m + 1)]
    E = [[INF] * (n + 1) for _ in range(m + 1)]
    F = [[INF] * (n + 1) for _ in range(m + 1)]
    H[0][0] = 0
    for i in range(m + 1):
        for j in range(n + 1):
            if i == 0 and j == 0:
                continue
            if j:
                E[i][j] = min(H[i][j - 1] + o + e, E[i][j - 1] + e)
            if i:
                F[i][j] = min(H[i - 1][j] + o + e, F[i - 1][j] + e)
            d = H[i - 1][j - 1] + (0 if t[j - 1] == p[i - 1] else x) if i and j else INF
            H[i][j] = min(d, E[i][j], F[i][j])
    return H[m][n]


def score(text, pattern, x=4, o=6, e=2):
    return np.float32(-penalty(text, pattern, x, o, e))


def scores(texts, patterns, x=4, o=6, e=2):
    return np.array([score(t, p, x, o, e) for t, p in zip(texts, patterns)], np.float32)


def random_seq(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def mutate(rng, s, rate):
    """s with substitutions, insertions and deletions (a third each) at about `rate` per byte"""
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < rate / 3:
            out.append(b"ACGT"[(b"ACGT".index(bytes([c])) + 1 + rng.integers(0, 3)) % 4] if bytes([c]) in b"ACGT" else ord("A"))
        elif r < 2 * rate / 3:
            out.append(c)
            out.append(b"ACGT"[rng.integers(0, 4)])
        elif r < rate:
            pass
        else:
            out.append(c)
    return bytes(out)


MIXED_MAX_PAIR_BYTES, MIXED_MAX_PENALTY = 4096, 400


def mixed_phase_pairs():
    """(texts, patterns, kinds): 200 rows in a fixed shuffled order whose pairs are in different phases of the forward pass at
    once when one wave holds several of them — kinds "empty" (0 + 0 and 0 + k bytes, NULL among them), "same" (done at s = 0),
    "near" (20..150 bytes at 5 %), "capped" (a penalty above MIXED_MAX_PENALTY), "long" (above MIXED_MAX_PAIR_BYTES) and "global"
    (2 x 1 200 bytes at 2 %: 74 454 bytes of rings and strings, more than a pair's LDS share at any lane width)"""
    rng = np.random.default_rng(2024)
    rows = [(b"", b"", "empty"), (None, None, "empty"), (None, b"ACGTACGTACGTA", "empty"), (b"", b"ACG", "empty")]
    rows += [(random_seq(rng, int(k)), b"" if k % 2 else None, "empty") for k in rng.integers(1, 40, 12)]
    for k in rng.integers(20, 151, 30):
        s = random_seq(rng, int(k))
        rows.append((s, s, "same"))
    for k in rng.integers(20, 151, 145):
        s = random_seq(rng, int(k))
        rows.append((s, mutate(rng, s, 0.05), "near"))
    rows += [(bytes([a]) * k, bytes([b]) * k, "capped") for a, b, k in zip(b"ACGT", b"CGTA", (150, 140, 130, 120))]
    for _ in range(3):
        s = random_seq(rng, 1200)
        rows.append((s, mutate(rng, s, 0.02), "global"))
    for k in (2100, 2049):
        s = random_seq(rng, k)
        rows.append((s, s[:-1], "long"))
    assert len(rows) == 200
    order = rng.permutation(len(rows))
    texts, patterns, kinds = zip(*[rows[i] for i in order])
    return list(texts), list(patterns), np.array(kinds)
