"""The oracle of the alignment strings, in plain Python; it shares nothing with the library.

(a) cigar(text, pattern, x, o, e, match=0): a full-history wavefront pass over dicts keyed by (score, diagonal) and the
    backtrace rule of INTEGRATION.md, "Alignment strings", as written there — which optimum is OURS, so the oracle has to
    restate the rule; what it does not share is any code, any data layout or the visited-range bookkeeping.
(b) check(text, pattern, cigar, x, o, e): no wavefronts at all.  Parses the CIGAR, walks both strings (every M column equal,
    every X column unequal, exactly n and m bytes consumed, no two neighbouring runs with one letter) and compares the
    CIGAR's own penalty with align_ref.penalty, the Gotoh matrix.
A NULL (None) string is an empty one."""
import re

import align_ref

NONE = -(1 << 40)


def fold(match, x, o, e):
    """a match score a <= 0 folded into the penalties: minimising a #M + x #X + o #gaps + e gaplen under
    n + m = 2 #M + 2 #X + gaplen is minimising (2x - 2a) #X + 2o #gaps + (2e - a) gaplen"""
    return (2 * x - 2 * match, 2 * o, 2 * e - match) if match else (x, o, e)


def cigar(text, pattern, x=4, o=6, e=2, match=0):
    t, p = text or b"", pattern or b""
    x, o, e = fold(match, x, o, e)
    n, m = len(t), len(p)
    M, I, D = {}, {}, {}

    def rect(h, k):
        return h if 0 <= h <= n and 0 <= h - k <= m else NONE

    def extend(h, k):
        v = h - k
        while h < n and v < m and t[h] == p[v]:
            h, v = h + 1, v + 1
        return h

    s = 0
    M[0, 0] = extend(0, 0)
    lo = hi = 0
    live = {0}                      # the scores that have any entry: a score none of whose three sources is live has none
    while M.get((s, n - m), NONE) < n:
        s += 1
        if not live & {s - x, s - e, s - o - e}:
            continue
        live.add(s)
        for k in range(max(lo - 1, -m), min(hi + 1, n) + 1):
            i = rect(max(M.get((s - o - e, k - 1), NONE), I.get((s - e, k - 1), NONE)) + 1, k)
            d = rect(max(M.get((s - o - e, k + 1), NONE), D.get((s - e, k + 1), NONE)), k)
            best = max(rect(M.get((s - x, k), NONE) + 1, k), i, d)
            if i >= 0:
                I[s, k] = i
            if d >= 0:
                D[s, k] = d
            if best >= 0:
                M[s, k] = extend(best, k)
                lo, hi = min(lo, k), max(hi, k)
    # the backtrace: letters last column first
    out = []
    state, k, h = "M", n - m, n
    while True:
        if state == "M":
            if s == 0:
                out.append("M" * h)
                break
            sub, ins, dele = rect(M.get((s - x, k), NONE) + 1, k), I.get((s, k), NONE), D.get((s, k), NONE)
            pre = max(sub, ins, dele)
            assert 0 <= pre <= h
            out.append("M" * (h - pre))
            if sub == pre:
                out.append("X")
                s, h = s - x, pre - 1
            elif dele == pre:
                state, h = "D", pre
            else:
                state, h = "I", pre
        elif state == "D":
            out.append("D")
            if D.get((s - e, k + 1), NONE) == h:
                s -= e
            else:
                assert M.get((s - o - e, k + 1), NONE) == h
                s, state = s - o - e, "M"
            k += 1
        else:
            out.append("I")
            if I.get((s - e, k - 1), NONE) + 1 == h:
                s -= e
            else:
                assert M.get((s - o - e, k - 1), NONE) + 1 == h
                s, state = s - o - e, "M"
            k, h = k - 1, h - 1
    letters = "".join(out)[::-1]
    return "".join("%d%s" % (len(r.group(0)), r.group(1)) for r in re.finditer(r"(.)\1*", letters)).encode()


def runs(c):
    """[(count, letter)] of a CIGAR of M, X, I, D; raises on anything else"""
    c = c.decode() if isinstance(c, (bytes, bytearray)) else c
    got = re.findall(r"(\d+)([MXID])", c)
    assert "".join(a + b for a, b in got) == c, c
    return [(int(a), b) for a, b in got]


def check(text, pattern, c, x=4, o=6, e=2):
    """the CIGAR is an alignment of the pair, in canonical run-length form, and its penalty is the optimum"""
    t, p = text or b"", pattern or b""
    h = v = pen = 0
    last = ""
    for count, letter in runs(c):
        assert count > 0 and letter != last, c
        last = letter
        if letter in "MX":
            assert h + count <= len(t) and v + count <= len(p), c
            for q in range(count):
                assert (t[h + q] == p[v + q]) == (letter == "M"), (c, h + q, v + q)
            h, v = h + count, v + count
            pen += x * count if letter == "X" else 0
        elif letter == "I":
            h, pen = h + count, pen + o + e * count
        else:
            v, pen = v + count, pen + o + e * count
    assert (h, v) == (len(t), len(p)), (c, h, v)
    assert pen == align_ref.penalty(t, p, x, o, e), (c, pen)
    return pen
