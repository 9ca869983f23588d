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
