"""A DEFLATE (RFC 1951) writer that takes orders: every field of a stream is chosen by the caller, nothing is optimised.

zlib's compressor visits a small part of the format (optimal codes, at least two distance codes, no 284+31, HCLEN as short
as it goes ...).  This writer builds the rest by hand, the way tests/zstd_frames.py does for zstd:

    spec            a Stream: a list of blocks (Stored / Fixed / Dynamic) + bytes behind the final block
    token           an int (literal), (length, distance) or (length, distance, 284) for 258 sent as 284 + 31;
                    the end-of-block code is written by the block itself.  Raw tokens for invalid streams:
                    ("lsym", s) a literal/length symbol's bare code, ("mraw", length, dist_symbol) a length followed by the
                    bare code of a distance symbol, ("bits", value, n) n plain bits
    encode(spec)            -> bytes
    expected_output(spec)   -> the bytes the tokens describe (byte by byte: overlapping matches are honoured)
    forms(spec)             -> names of the RFC forms the spec exercises (REQUIRED_FORMS lists what the catalogue must reach)
    catalogue()             -> name -> valid Stream
    invalid()               -> name -> (Stream or raw bytes, RFC clause, class as InflateStatus.code names it)
    random_stream(seed, n)  -> a Stream of random blocks whose codes are complete but deliberately NOT optimal

tests/test_deflate_frames.py proves the writer against zlib's decoder before it judges the device."""
import random

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
LONG, SHORT = 11, 9          # a code of >= 11 bits is long, one of <= 9 short, under both table-size builds of the decoder


class BitWriter:
    """LSB-first bit sink (RFC 1951 3.1.1); Huffman codes go in most significant bit first"""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, nbits):
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def align(self):
        if self.n:
            self.buf.append(self.acc & 255)
            self.acc = 0
            self.n = 0

    def raw(self, data):
        assert self.n == 0
        self.buf += data

    @property
    def bitpos(self):
        return 8 * len(self.buf) + self.n

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc & 255]) if self.n else b"")


def canonical(lengths):
    """code lengths -> {symbol: (code already bit-reversed for an LSB-first writer, length)} (RFC 1951 3.2.2)"""
    count = [0] * 17
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for sym, ln in enumerate(lengths):
        if ln:
            c = nxt[ln] & ((1 << ln) - 1)         # (over-subscribed lengths, invalid streams only, wrap around)
            nxt[ln] += 1
            out[sym] = (int(format(c, "0%db" % ln)[::-1], 2), ln)
    return out


def kraft(lengths):
    """sum of 2^-len in units of 2^-15: 32768 = complete"""
    return sum(32768 >> ln for ln in lengths if ln)


def length_symbol(length, as284=False):
    if length == 258:
        return (284, 31, 5) if as284 else (285, 0, 0)
    s = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + s, length - LEN_BASE[s], LEN_EXTRA[s]


def dist_symbol(dist):
    s = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return s, dist - DIST_BASE[s], DIST_EXTRA[s]


_LEN_SYM = {(ln, a): length_symbol(ln, a) for ln in range(3, 259) for a in (False, True) if ln == 258 or not a}
_DIST_SYM = {}


def _dsym(d):
    r = _DIST_SYM.get(d)
    if r is None:
        r = _DIST_SYM[d] = dist_symbol(d)
    return r


class Stored:
    def __init__(self, data=b"", final=False, nlen=None):
        self.data, self.final, self.nlen = bytes(data), final, nlen


class Fixed:
    def __init__(self, tokens=(), final=False, eob=True):
        self.tokens, self.final, self.eob = list(tokens), final, eob
        self.lit_lens, self.dist_lens = FIXED_LIT, FIXED_DIST


class Dynamic:
    """lit_lens: HLIT code lengths (257 .. 286 of them), dist_lens: HDIST (1 .. 30).  The lengths travel as `cl` says:
    "plain" (a code-length symbol per length), "rle" (greedy 16 / 17 / 18 over literal and distance lengths as ONE sequence,
    so a run may cross from one into the other) or an explicit list of (symbol, extra) operations.  cl_lens: {code-length
    symbol: bits} (default: a balanced complete code over the symbols used); hclen: how many of them are sent (default: as
    few as possible).  check = False lets lengths through that are not a legal code (invalid streams)."""

    def __init__(self, lit_lens, dist_lens, tokens=(), final=False, eob=True, cl="rle", cl_lens=None, hclen=None, check=True,
                 hlit_field=None, hdist_field=None):
        self.lit_lens, self.dist_lens, self.tokens = list(lit_lens), list(dist_lens), list(tokens)
        self.final, self.eob, self.cl, self.cl_lens, self.hclen, self.check = final, eob, cl, cl_lens, hclen, check
        self.hlit_field, self.hdist_field = hlit_field, hdist_field

    def cl_ops(self):
        seq = self.lit_lens + self.dist_lens
        if isinstance(self.cl, list):
            return self.cl
        if self.cl == "plain":
            return [(v, 0) for v in seq]
        ops, i = [], 0
        while i < len(seq):
            v, j = seq[i], i
            while j < len(seq) and seq[j] == v:
                j += 1
            run = j - i
            if v == 0:
                while run >= 11:
                    n = min(run, 138)
                    ops.append((18, n - 11))
                    run -= n
                if run >= 3:
                    ops.append((17, run - 3))
                    run = 0
                ops += [(0, 0)] * run
            else:
                ops.append((v, 0))
                run -= 1
                while run >= 3:
                    n = min(run, 6)
                    ops.append((16, n - 3))
                    run -= n
                ops += [(v, 0)] * run
            i = j
        return ops


class Stream:
    def __init__(self, blocks, trailing=b"", tags=()):
        self.blocks, self.trailing, self.tags = list(blocks), bytes(trailing), set(tags)


def _balanced(symbols):
    """a complete code over `symbols` (>= 2 of them) with lengths as equal as they go"""
    m = len(symbols)
    k = max(1, (m - 1).bit_length())
    short = (1 << k) - m
    return {s: (k - 1 if i < short else k) for i, s in enumerate(symbols)}


def _write_dynamic_header(w, b, info):
    ops = b.cl_ops()
    used = sorted({s for s, _ in ops})
    cl_lens = b.cl_lens
    if cl_lens is None:
        cl_lens = _balanced(used if len(used) > 1 else used + [s for s in (0, 8, 1) if s not in used][:1])
    lens19 = [cl_lens.get(s, 0) for s in range(19)]
    if b.check:
        assert kraft(lens19) == 32768 and all(lens19[s] for s in used), "code-length code"
        assert sum({16: 3 + x, 17: 3 + x, 18: 11 + x}.get(s, 1) for s, x in ops) == len(b.lit_lens) + len(b.dist_lens)
    hclen = b.hclen or max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if lens19[s]))
    w.bits(len(b.lit_lens) - 257 if b.hlit_field is None else b.hlit_field, 5)
    w.bits(len(b.dist_lens) - 1 if b.hdist_field is None else b.hdist_field, 5)
    w.bits(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        w.bits(lens19[s], 3)
    codes = canonical(lens19)
    idx, nlit = 0, len(b.lit_lens)
    for s, x in ops:
        w.bits(*codes[s])
        rep = 1
        if s == 16:
            w.bits(x, 2)
            rep = 3 + x
            if idx < nlit < idx + rep:
                info["forms"].add("hdr:rep16_across_boundary")
        elif s == 17:
            w.bits(x, 3)
            rep = 3 + x
        elif s == 18:
            w.bits(x, 7)
            rep = 11 + x
            if x == 127:
                info["forms"].add("hdr:rep18_138")
        idx += rep
    f = info["forms"]
    if hclen in (4, 5, 19):
        f.add("hdr:hclen%d" % hclen)
    if max(lens19) == 7:
        f.add("hdr:cl_7bit")
    if len(b.lit_lens) in (257, 286):
        f.add("hdr:hlit%d" % len(b.lit_lens))
    if len(b.dist_lens) == 30:
        f.add("hdr:hdist30")
    if b.dist_lens == [0]:
        f.add("hdr:hdist1_len0")
    if sorted(x for x in b.lit_lens if x) == list(range(1, 16)) + [15]:
        f.add("hdr:deepest_lit")
    if sorted(x for x in b.dist_lens if x) == list(range(1, 16)) + [15]:
        f.add("hdr:deepest_dist")
    if not b.tokens and b.eob:
        f.add("blk:eob_only")


def _write_tokens(w, b, info, dynamic):
    lit = canonical(b.lit_lens)
    dist = canonical(b.dist_lens)
    f = info["forms"]
    bits = w.bits
    prev_long = False
    run1 = run2 = 0
    single_dist = dynamic and [x for x in b.dist_lens if x] == [1]
    for k, t in enumerate(b.tokens):
        if isinstance(t, int):
            c = lit[t]
            bits(*c)
            is_long = c[1] >= LONG
            run1 = run1 + 1 if c[1] == 1 else 0
            run2 = 0
            if run1 == 256:
                f.add("tok:1bit_literals_x256")
        elif t[0] == "lsym":
            bits(*lit[t[1]])
            continue
        elif t[0] == "bits":
            bits(t[1], t[2])
            continue
        elif t[0] == "mraw":
            s, x, xb = _LEN_SYM[(t[1], False)]
            bits(*lit[s])
            bits(x, xb)
            if t[2] is not None:
                bits(*dist[t[2]])
            continue
        else:
            ln, d = t[0], t[1]
            s, x, xb = _LEN_SYM[(ln, len(t) > 2 and t[2] == 284)]
            ds, dx, dxb = _dsym(d)
            lc, dc = lit[s], dist[ds]
            bits(*lc)
            bits(x, xb)
            bits(*dc)
            bits(dx, dxb)
            is_long = lc[1] >= LONG or dc[1] >= LONG
            run1 = 0
            if ln == 258:
                f.add("tok:258_as_284_31" if s == 284 else "tok:258_as_285")
            if single_dist:
                f.add("hdr:single_dist_code")
            if lc[1] + xb + dc[1] + dxb == 48:
                f.add("tok:48bit")
            run2 = run2 + 1 if (ln == 258 and lc[1] + xb + dc[1] + dxb == 2) else 0
            if run2 == 64:
                f.add("tok:2bit_258")
            if dynamic and (lc[1] >= LONG or lc[1] <= SHORT) and (dc[1] >= LONG or dc[1] <= SHORT) and ln >= 11:
                f.add("tok:%s_len_%s_dist" % ("long" if lc[1] >= LONG else "short", "long" if dc[1] >= LONG else "short"))
            if dynamic:
                info["pairs"].append((lc[1], dc[1]))
            fx = info["fixed_syms"] if not dynamic else None
            if fx is not None:
                for kind in ((0, 1) if xb == 0 else ((0,) if x == 0 else (1,) if x == (1 << xb) - 1 else ())):
                    fx.add(("L", s, kind))
                for kind in ((0, 1) if dxb == 0 else ((0,) if dx == 0 else (1,) if dx == (1 << dxb) - 1 else ())):
                    fx.add(("D", ds, kind))
        if dynamic:
            info["n_tokens"] += 1
            info["n_long"] += is_long
            if is_long:
                if prev_long:
                    f.add("tok:long_back_to_back")
                if k == 0:
                    f.add("tok:long_first")
                if k == len(b.tokens) - 1 and b.eob:
                    f.add("tok:long_before_eob")
            prev_long = is_long
    if b.eob:
        bits(*lit[256])


def _encode(spec):
    if not isinstance(spec, Stream):
        spec = Stream(spec)
    w = BitWriter()
    info = {"forms": set(spec.tags), "pairs": [], "n_tokens": 0, "n_long": 0, "fixed_syms": set(), "blocks": [], "dynamic": []}
    f = info["forms"]
    empty_fixed = 0
    prev = None
    for b in spec.blocks:
        start = w.bitpos
        w.bits(1 if b.final else 0, 1)
        if isinstance(b, Stored):
            w.bits(0, 2)
            if prev is not None and not isinstance(prev, Stored):
                f.add("stored:after_phase%d" % (start % 8))
            w.align()
            n = len(b.data)
            w.bits(n, 16)
            w.bits((n ^ 0xFFFF) if b.nlen is None else b.nlen, 16)
            d0 = len(w.buf)
            w.raw(b.data)
            if n == 0:
                f.add("stored:len0_final" if b.final else "stored:len0")
            elif n in (1, 63, 64, 65, 65535):
                f.add("stored:len%d" % n)
            for edge, name in ((128, "stored:straddle128"), (256, "stored:straddle256")):
                m = (d0 // 256) * 256 + edge if edge == 128 else (d0 // 256 + 1) * 256
                if d0 < m < d0 + n:
                    f.add(name)
            empty_fixed = 0
        elif isinstance(b, Fixed):
            w.bits(1, 2)
            _write_tokens(w, b, info, False)
            empty_fixed = empty_fixed + 1 if not b.tokens else 0
            if empty_fixed == 40:
                f.add("fixed:empty_x40")
        else:
            w.bits(2, 2)
            _write_dynamic_header(w, b, info)
            before = (info["n_tokens"], info["n_long"])
            _write_tokens(w, b, info, True)
            info["dynamic"].append((getattr(b, "mode", None), info["n_tokens"] - before[0], info["n_long"] - before[1]))
            empty_fixed = 0
        info["blocks"].append((start, w.bitpos))
        prev = b
    if spec.blocks and spec.blocks[-1].final:
        f.add("end:phase%d" % (w.bitpos % 8))
    info["end_bit"] = w.bitpos
    w.align()
    if spec.trailing:
        f.add("end:trailing_bytes")
        w.raw(spec.trailing)
    fx = info["fixed_syms"]
    for kind in (0, 1):
        if all(("L", s, kind) in fx for s in range(257, 286)):
            f.add("fixed:all_len_syms_extra%d" % kind)
        if all(("D", s, kind) in fx for s in range(30)):
            f.add("fixed:all_dist_syms_extra%d" % kind)
    _match_forms(spec, f)
    return w.getvalue(), info


def _match_forms(spec, f):
    """forms that depend on where a match stands in the output"""
    pos = 0
    grid = set()
    at_ring = at_lag = 0
    for b in spec.blocks:
        if isinstance(b, Stored):
            pos += len(b.data)
            continue
        prev_match = None
        for t in b.tokens:
            if isinstance(t, int):
                pos += 1
                prev_match = None
            elif isinstance(t[0], int):
                ln, d = t[0], t[1]
                if d == pos:
                    f.add("match:dist_eq_pos")
                if d == 32768 and pos == 32768:
                    f.add("match:32768_at_32768")
                if d <= 16 and (ln <= 18 or ln == 258):
                    grid.add((d, ln))
                # The decoder's ring holds the newest 2048 bytes of [.., hi), hi = the end of the step the match is copied in:
                # pos + ln <= hi <= pos + ln + 770 (a step emits <= 512 bytes + one match).  The source [pos - d, pos - d + ln)
                # can lie across the ring's edge hi - 2048 for some such hi iff 1278 - ln < d < 2048.  What is older than the
                # ring was flushed in whole 1 KiB segments: a source of that reach that lies across a multiple of 1024
                if 1278 - ln < d < 2048:
                    at_ring += 1
                if ln <= d <= 1024 + 770 and (pos - d) // 1024 != (pos - d + ln - 1) // 1024:
                    at_lag += 1
                if prev_match and pos - d < prev_match[1] and pos - d + ln > prev_match[0]:
                    f.add("match:fed_by_match_same_step")
                prev_match = (pos, pos + ln)
                pos += ln
    if at_ring >= 100:
        f.add("match:src_straddles_ring")
    if at_lag >= 20:
        f.add("match:src_straddles_flush_lag")
    if all((d, ln) in grid for d in range(1, 17) for ln in list(range(3, 19)) + [258]):
        f.add("match:small_dist_grid")


def encode(spec):
    if isinstance(spec, (bytes, bytearray)):
        return bytes(spec)
    return _encode(spec)[0]


def forms(spec):
    return _encode(spec)[1]["forms"]


def stats(spec):
    """the encoder's own account of a spec: block bit ranges, end bit, (length code bits, distance code bits) per match of
    the dynamic blocks, and per dynamic block (the mode coded_block skewed it with, tokens, tokens with a code of >= 11 bits)"""
    return _encode(spec)[1]


def consumed(spec):
    """compressed bytes up to the byte boundary behind the final block"""
    return (_encode(spec)[1]["end_bit"] + 7) // 8


def expected_output(spec):
    blocks = spec.blocks if isinstance(spec, Stream) else spec
    out = bytearray()
    for b in blocks:
        if isinstance(b, Stored):
            out += b.data
            continue
        for t in b.tokens:
            if isinstance(t, int):
                out.append(t)
            elif isinstance(t[0], int):
                ln, d = t[0], t[1]
                assert 1 <= d <= len(out), "distance before the start of the output"
                if d >= ln:
                    out += out[len(out) - d:len(out) - d + ln]
                else:
                    for _ in range(ln):
                        out.append(out[-d])
    return bytes(out)


def nonfinal(spec):
    """the blocks of a stream, none of them final (to be followed by more)"""
    import copy
    out = []
    for b in spec.blocks:
        b = copy.copy(b)
        b.final = False
        out.append(b)
    return out


# ---- code lengths by order ---------------------------------------------------------------------------------------------------
def chain_lengths(n):
    """the deepest complete code over n symbols: 1, 2, ..., n - 1, n - 1 (n <= 16: 1 .. 14, 15, 15)"""
    assert 2 <= n <= 16
    return list(range(1, n)) + [n - 1]


def lens_of(assign, n):
    """{symbol: bits} -> list of n lengths"""
    out = [0] * n
    for s, ln in assign.items():
        out[s] = ln
    return out


def shaped_lengths(n, rng, deep):
    """n lengths (n >= 2) of a complete code, <= 15 bits, sorted longest first.  deep: the 1, 2, ..., 15, 15 chain first,
    further leaves by splitting random ones; else random splits from the root"""
    leaves = [1, 1]
    if deep:
        leaves = chain_lengths(min(n, 16))
    while len(leaves) < n:
        cand = [i for i, ln in enumerate(leaves) if ln < 15]
        i = rng.choice(cand)
        leaves[i] += 1
        leaves.append(leaves[i])
    return sorted(leaves, reverse=True)


def skewed_code(freq, n_syms, rng, long_syms, deep=True):
    """complete, NOT optimal: the symbols of `long_syms` (most frequent first) take the longest codes; the others the
    rest, most frequent shortest.  freq: {symbol: count} of the symbols used (>= 1; a second one is added where needed)"""
    used = sorted(freq, key=lambda s: (-freq[s], s))
    if len(used) == 1:
        used.append(next(s for s in range(n_syms) if s not in freq))
    shape = shaped_lengths(len(used), rng, deep)
    want_long = [s for s in used if s in long_syms]
    rest = [s for s in used if s not in long_syms]
    assign = {}
    for s in want_long:
        assign[s] = shape.pop(0)
    for s in rest:
        assign[s] = shape.pop()
    return assign


# ---- generator ----------------------------------------------------------------------------------------------------------------
TEXT = b"ACGTN\n@+FI#:0123456789"
BANDS = [(1, 16), (1, 16), (17, 200), (900, 1100), (1980, 2120), (3000, 9000), (32700, 32768)]


def tokenise(data, history=b"", min_len=3, max_chain=8):
    """greedy LZ77 over `data` (3-byte hash, the newest few candidates, the longest match wins): the writer's own match
    finder, for payloads that are given rather than drawn"""
    buf = bytes(history) + bytes(data)
    heads = {}
    i, n = len(history), len(buf)
    tokens = []
    for j in range(max(0, len(history) - 32768), len(history)):
        heads.setdefault(buf[j:j + 3], []).append(j)
    while i < n:
        best_len, best_d = 0, 0
        key = buf[i:i + 3]
        cands = heads.get(key)
        if cands and len(key) == 3:
            for j in reversed(cands[-max_chain:]):
                if i - j > 32768:
                    break
                ln = 3
                lim = min(258, n - i)
                while ln < lim and buf[j + ln] == buf[i + ln]:
                    ln += 1
                if ln > best_len:
                    best_len, best_d = ln, i - j
        step = 1
        if best_len >= min_len:
            tokens.append((best_len, best_d))
            step = best_len
        else:
            tokens.append(buf[i])
        for j in range(i, min(i + step, n - 2)):
            heads.setdefault(buf[j:j + 3], []).append(j)
        i += step
    return tokens


def coded_block(tokens, rng, mode, final=False, cl=None):
    """a Dynamic block around `tokens`.  mode: "long" (11 .. 15-bit codes for the most frequent literals, lengths and
    distances), "short" (1- and 2-bit codes for them), or a triple of booleans (long literals, long lengths, long distances)"""
    lf, df = {256: 1}, {}
    for t in tokens:
        if isinstance(t, int):
            lf[t] = lf.get(t, 0) + 1
        else:
            s = _LEN_SYM[(t[0], len(t) > 2 and t[2] == 284)][0]
            lf[s] = lf.get(s, 0) + 1
            ds = _dsym(t[1])[0]
            df[ds] = df.get(ds, 0) + 1
    if mode == "long":
        mode = (True, True, True)
    elif mode == "short":
        mode = (False, False, False)
    top = sorted(lf, key=lambda s: -lf[s])
    long_lit = {s for s in top if (s < 256 and mode[0]) or (s > 256 and mode[1])}
    # (the chain has six codes of >= 11 bits and random splits add more: the most frequent of the chosen class get them)
    long_lit = set(sorted(long_lit, key=lambda s: -lf[s])[:rng.choice((4, 6, 12, 40))])
    la = skewed_code(lf, 286, rng, long_lit, deep=any(mode[:2]) or rng.random() < 0.5)
    nlit = max(257, max(la) + 1)
    if rng.random() < 0.25:
        nlit = 286
    if not df:
        dist_lens = [0] if rng.random() < 0.5 else [1] + [0] * rng.randrange(0, 29)
    elif len(df) == 1 and rng.random() < 0.5:
        ds = next(iter(df))
        dist_lens = lens_of({ds: 1}, ds + 1)          # a single distance code: one bit, the other half unused
    else:
        long_d = set(sorted(df, key=lambda s: -df[s])[:rng.choice((2, 4, 6))]) if mode[2] else set()
        da = skewed_code(df, 30, rng, long_d, deep=mode[2] or rng.random() < 0.5)
        nd = max(da) + 1
        if rng.random() < 0.25:
            nd = 30
        dist_lens = lens_of(da, nd)
    b = Dynamic(lens_of(la, nlit), dist_lens, tokens, final=final, cl=cl or rng.choice(("rle", "rle", "plain")))
    b.mode = mode
    return b


def random_tokens(rng, out, n_tokens, alphabet=TEXT, p_lit=0.45, p_short=0.6):
    """tokens drawn, not found: literals of the alphabet; matches whose distance comes from bands around 1 - 16, the decoder's
    2 KiB ring edge, its 1 KiB flush lag and 32768, and whose length covers 3 .. 258.  `out` (bytearray) grows with them."""
    tokens = []
    for _ in range(n_tokens):
        if len(out) < 4 or rng.random() < p_lit:
            c = alphabet[rng.randrange(len(alphabet))]
            tokens.append(c)
            out.append(c)
            continue
        lo, hi = BANDS[rng.randrange(len(BANDS))]
        d = rng.randint(lo, hi)
        if d > len(out):
            d = rng.randint(1, min(len(out), 16))
        r = rng.random()
        ln = rng.randint(3, 18) if r < p_short else rng.randint(11, 258) if r < 0.95 else 258
        tokens.append((ln, d, 284) if ln == 258 and rng.random() < 0.5 else (ln, d))
        if d >= ln:
            out += out[len(out) - d:len(out) - d + ln]
        else:
            for _ in range(ln):
                out.append(out[-d])
    return tokens


def random_stream(seed, n_out, alphabet=TEXT, final=True, history=b"", p_lit=0.45, p_short=0.6, kinds=None):
    """random blocks of all three types around drawn tokens (random_tokens) and, now and then, a piece of text cut by the greedy
    match finder (tokenise); the dynamic blocks' codes are Kraft-exact and skewed the wrong way round in most of them"""
    rng = random.Random(seed)
    out = bytearray(history)
    blocks = []
    while len(out) - len(history) < n_out:
        kind = rng.choice(kinds or ("long", "long", "pairs", "pairs", "short", "fixed", "stored", "found"))
        n_tok = rng.choice((0, 1, 2, 5, 40, 300, 1500, 4000))
        if kind == "stored":
            data = bytes(alphabet[rng.randrange(len(alphabet))] for _ in range(rng.choice((0, 0, 1, 64, 700))))
            out += data
            blocks.append(Stored(data))
            continue
        if kind == "found":
            line = bytes(alphabet[rng.randrange(len(alphabet))] for _ in range(60))
            text = b"".join(line[:rng.randint(20, 60)] + b"\n" for _ in range(rng.randint(1, 30)))
            tokens = tokenise(text, history=bytes(out[-32768:]))
            out += text
            kind = rng.choice(("long", "short", "fixed"))
        else:
            tokens = random_tokens(rng, out, n_tok, alphabet, p_lit, p_short)
        if kind == "fixed":
            blocks.append(Fixed(tokens))
        elif kind == "pairs":
            blocks.append(coded_block(tokens, rng, (rng.random() < 0.5, rng.random() < 0.5, rng.random() < 0.5)))
        else:
            blocks.append(coded_block(tokens, rng, kind))
    if final:
        blocks.append(rng.choice((Stored(b"", final=True), Fixed([], final=True), coded_block([], rng, "short", final=True))))
    s = Stream(blocks)
    s._content = bytes(out[len(history):])
    return s


# ---- catalogue ------------------------------------------------------------------------------------------------------------------
def _fill(n, seed=1):
    """tokens of a fixed block that produce exactly n bytes: 64 random literals, then matches of every length"""
    rng = random.Random(seed)
    out = bytearray()
    tokens = []
    while len(out) < n:
        left = n - len(out)
        if len(out) < 64 or left < 3:
            c = rng.randrange(256)
            tokens.append(c)
            out.append(c)
        else:
            ln = min(left, rng.choice((3, 17, 100, 258, 258)))
            d = rng.randint(1, min(len(out), 32768))
            tokens.append((ln, d))
            for _ in range(ln):
                out.append(out[-d])
    return tokens


def _eob(**kw):
    return Fixed([], final=True, **kw)


def _chain_block(lit_order, dist_order, tokens, final=True, **kw):
    """lit_order / dist_order: symbols that take 1, 2, 3, ... bits in this order (the deepest code over them)"""
    ll = lens_of(dict(zip(lit_order, chain_lengths(len(lit_order)))), max(257, max(lit_order) + 1))
    dl = lens_of(dict(zip(dist_order, chain_lengths(len(dist_order)))), max(dist_order) + 1) if dist_order else [0]
    return Dynamic(ll, dl, tokens, final=final, **kw)


_CATALOGUE = None


def catalogue():
    global _CATALOGUE
    if _CATALOGUE is None:
        _CATALOGUE = _build_catalogue()
    return _CATALOGUE


def _build_catalogue():
    rng = random.Random(1951)
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))   # noqa: E731
    c = {}
    # -- stored
    c["stored_len0"] = Stream([Fixed(list(b"ab")), Stored(b""), Stored(b""), Fixed(list(b"cd")), Stored(b"", final=True)])
    c["stored_len0_only"] = Stream([Stored(b"", final=True)])
    c["stored_lens"] = Stream([Stored(rb(1)), Stored(rb(63)), Stored(rb(64)), Stored(rb(65)), Stored(rb(1), final=True)])
    c["stored_65535"] = Stream([Stored(rb(65535)), Fixed([(258, 65535 - 32767), (100, 32768)]), Stored(b"", final=True)])
    blocks = []
    for j in range(8):      # a fixed block from a byte boundary: 3 + 8 + 9 j + 7 bits -> the stored header starts at phase 2 + j
        blocks += [Fixed([97] + [200 + j] * j), Stored(rb(3 + j))]
    c["stored_after_every_phase"] = Stream(blocks + [_eob()])
    c["stored_straddles_input_ring"] = Stream([Fixed(list(b"ring")), Stored(rb(200)), Stored(rb(100)), Stored(rb(300)), _eob()])
    # -- fixed
    c["fixed_empty_x40"] = Stream([Fixed([]) for _ in range(40)] + [Fixed([65], final=True)])
    toks = _fill(32768 + 300, seed=2)
    for s in range(29):
        for x in {0, (1 << LEN_EXTRA[s]) - 1}:
            ln = LEN_BASE[s] + x
            toks.append((ln, rng.randint(1, 32768), 284) if s == 27 and ln == 258 else (ln, rng.randint(1, 32768)))
    for s in range(30):
        for x in {0, (1 << DIST_EXTRA[s]) - 1}:
            toks.append((rng.randint(3, 40), DIST_BASE[s] + x))
    c["fixed_every_symbol"] = Stream([Fixed(toks, final=True)])
    # -- dynamic headers
    lit257 = [8] * 255 + [9, 9]                                   # 255 / 256 + 2 / 512
    c["hlit257_hdist1_len0"] = Stream([Dynamic(lit257, [0], list(b"literals only") + [255, 0, 254], final=True)])
    ll = [0] * 286
    for s, ln in zip([65, 66, 256, 285, 257, 284], [1, 2, 3, 4, 5, 5]):
        ll[s] = ln
    dl = [5] * 28 + [4, 4]
    c["hlit286_hdist30"] = Stream([Fixed(_fill(32768, seed=3)), Dynamic(ll, dl, [65, 66, (258, 24577 + 8191), (258, 16385, 284), (3, 1)], final=True)])
    c["hclen5"] = Stream([Dynamic([0] + [8] * 256, [0], list(range(1, 256)), final=True, cl="plain", cl_lens={0: 1, 8: 1})])
    order = [101, 256, 32, 116, 97, 257, 111, 110, 258, 105, 115, 114, 104, 285, 100, 108]
    text = [101, 32, 116, 97, (3, 2), 111, 110, (4, 3), 105, 115, 114, 104, (258, 5), 100, 108, 108, 100]
    c["deepest_lit_hclen19"] = Stream([_chain_block(order, [1, 2, 4], text, cl="plain")])
    dorder = [0, 3, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 20, 21]
    dt = []
    for ds in dorder:
        dt += [(5, DIST_BASE[ds]), 65]
    c["deepest_dist"] = Stream([Stored(rb(2100)), _chain_block([65, 259, 256], dorder, dt + [(5, 1537 + 511)])])
    ll = lens_of({65: 1, 66: 2, 67: 3, 68: 4, 69: 5, 70: 6, 256: 7, 257: 7}, 258)
    seven = {0: 1, 1: 2, 2: 3, 3: 4, 4: 5, 5: 6, 6: 7, 7: 7}
    c["cl_7bit_codes"] = Stream([Dynamic(ll, [1, 1], [65, 66, 67, 68, 69, 70, (3, 1), (3, 2)], final=True, cl="plain", cl_lens=seven)])
    ll = [8] * 232 + [0] * 22 + [5, 5, 5]
    c["rep16_across_boundary"] = Stream([Dynamic(ll, [5] * 28 + [4, 4], [1, 2, 3, 254, 255, 231, 254], final=True, cl="rle")])
    ll = lens_of({10: 2, 65: 2, 67: 2, 71: 3, 256: 3}, 257)     # 84 .. 255: a run of 171 zeros = 18 x 138 + 18 x 33
    c["rep18_138"] = Stream([Dynamic(ll, [0], list(b"GATTACA".replace(b"T", b"C")) + [10], final=True, cl="rle")])
    c["single_dist_code"] = Stream([Dynamic(lens_of({65: 1, 257: 2, 256: 3, 265: 3}, 266), [0, 0, 0, 1], [65, 65, 65, 65, (3, 4), (11, 4), (12, 4)], final=True)])
    c["eob_only_block"] = Stream([Dynamic(lens_of({65: 1, 256: 1}, 257), [0], []), Dynamic(lens_of({65: 1, 256: 1}, 257), [1], [], cl="plain"),
                                  Fixed([66], final=True)])
    # -- tokens
    c["len258_both_ways"] = Stream([Fixed([7, (258, 1, 284), (258, 1), 8, (258, 2, 284), (258, 259)], final=True)])
    # 15-bit code of a length symbol with 5 extra bits + 15-bit code of a distance symbol with 13: 48 bits
    lo = [65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77, 256, 281, 284]
    do = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 28, 29]
    c["token_48_bits"] = Stream([Fixed(_fill(32768, seed=4)), _chain_block(lo, do, [(131 + 31, 16385 + 8191), 65, (258, 24577 + 8191, 284), (227, 24577), (131, 16385)])])
    # short / long code of the length x short / long code of the distance, lengths >= 11; long tokens first, back to back and last
    lo = [65, 265, 256, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 266, 90]      # 265: 2 bits (lengths 11, 12), 266: 15 (13, 14)
    do = [0, 6, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15]                   # 6: 2 bits (9 .. 12), 14 / 15: 15 bits (129 .., 193 ..)
    toks = [(13, 130), (14, 200), 90, 65, (11, 9), (12, 12), 65, (11, 129), (12, 256), (13, 10), (14, 11), 65, 65, (13, 140), 90, 90, (14, 250)]
    c["short_long_pairings"] = Stream([Stored(rb(300)), _chain_block(lo, do, toks, final=False), _chain_block(lo, do, [90]), ])
    c["one_bit_literals"] = Stream([Dynamic(lens_of({97: 1, 98: 2, 256: 2}, 257), [0], [97] * 700 + [98] + [97] * 300, final=True)])
    c["two_bit_258"] = Stream([Dynamic(lens_of({97: 2, 256: 2, 285: 1}, 286), [1, 1], [97] + [(258, 1)] * 200 + [97, (258, 2)] * 3, final=True)])
    # -- matches
    toks = [1, (3, 1), 2, 3, (5, 5)] + list(rb(290)) + [(258, 300)]
    c["distance_equals_position"] = Stream([Fixed(toks, final=True)])
    c["distance_32768_at_32768"] = Stream([Fixed(_fill(32768, seed=5) + [(258, 32768), (3, 32768), 9, (258, 32768)], final=True)])
    toks = list(rb(16))
    for d in range(1, 17):
        for ln in list(range(3, 19)) + [258]:
            toks += [(ln, d), rng.randrange(256)]
    c["small_distance_grid"] = Stream([Fixed(toks, final=True)])
    # sources around the edge of the decoder's 2 KiB ring (what is older was flushed) and around its 1 KiB flush lag
    toks = []
    for d in list(range(880, 1130, 3)) + list(range(1700, 2400, 3)):
        toks += [(rng.choice((3, 8, 9, 16, 17, 40, 64, 65, 130)), d)] + [rng.randrange(256)] * rng.randrange(0, 3)
    pos = 4200 + sum(1 if isinstance(t, int) else t[0] for t in toks)
    for _ in range(60):     # sources that lie across the newest 1 KiB segment edges behind the output position
        ln = rng.choice((3, 8, 9, 16, 17, 40, 64, 65))
        m = (pos - 1) // 1024 * 1024
        if pos - m <= ln + 8:
            m -= 1024
        d = pos - (m - rng.randint(1, ln - 1))
        toks += [(ln, d), rng.randrange(256)]
        pos += ln + 1
    c["sources_at_ring_edge_and_flush_lag"] = Stream([Stored(rb(4200)), Fixed(toks, final=True)])
    toks = list(rb(600)) + [(10, 500), (10, 10), (5, 3), (16, 16), (8, 20), (3, 8), (258, 258), (100, 300), (4, 2)]
    c["match_fed_by_match"] = Stream([Fixed(toks, final=True)])
    # -- endings: the final block ends at every bit phase; bytes behind it stay unread
    for j in range(8):      # 3 + 8 + 9 j + 7 bits
        s = Stream([Fixed([69] + [210] * j, final=True)], trailing=b"\xff\x00\xa5" * (j % 2))
        c["final_block_ends_at_phase_%d" % ((18 + 9 * j) % 8)] = s
    return c


REQUIRED_FORMS = frozenset(
    ["stored:len0", "stored:len0_final"] + ["stored:len%d" % n for n in (1, 63, 64, 65, 65535)]
    + ["stored:after_phase%d" % p for p in range(8)] + ["stored:straddle128", "stored:straddle256"]
    + ["fixed:empty_x40", "fixed:all_len_syms_extra0", "fixed:all_len_syms_extra1", "fixed:all_dist_syms_extra0",
       "fixed:all_dist_syms_extra1"]
    # HCLEN = 4 names only the code-length symbols 16, 17, 18 and 0: every length is 0, there is no end-of-block code and the
    # block is invalid (zlib: "missing end-of-block").  The shortest valid header has five: invalid() holds the one with four
    + ["hdr:hlit257", "hdr:hlit286", "hdr:hdist1_len0", "hdr:hdist30", "hdr:hclen5", "hdr:hclen19", "hdr:cl_7bit",
       "hdr:rep16_across_boundary", "hdr:rep18_138", "hdr:single_dist_code", "hdr:deepest_lit", "hdr:deepest_dist", "blk:eob_only"]
    + ["tok:258_as_284_31", "tok:258_as_285", "tok:48bit", "tok:short_len_short_dist", "tok:short_len_long_dist",
       "tok:long_len_short_dist", "tok:long_len_long_dist", "tok:long_back_to_back", "tok:long_before_eob", "tok:long_first",
       "tok:1bit_literals_x256", "tok:2bit_258"]
    + ["match:dist_eq_pos", "match:32768_at_32768", "match:small_dist_grid", "match:src_straddles_ring",
       "match:src_straddles_flush_lag", "match:fed_by_match_same_step"]
    + ["end:phase%d" % p for p in range(8)] + ["end:trailing_bytes"])

def truncation_stream():
    """the ~300-byte stream whose every byte-truncation invalid() lists: stored, fixed and two dynamic blocks"""
    cat = catalogue()
    rng = random.Random(5)
    blocks = [Stored(bytes(rng.randrange(256) for _ in range(40)))] + nonfinal(cat["deepest_lit_hclen19"]) \
        + [Fixed(list(b"fixed block") + [(20, 100), (5, 1)])] + nonfinal(cat["short_long_pairings"])[1:] + [Fixed([33], final=True)]
    return Stream(blocks)


# names of invalid() entries zlib's decoder takes (none so far) -> why
ZLIB_ACCEPTS = {}


def _raw_dynamic_header(hlit_field, hdist_field, hclen_field, cl3):
    w = BitWriter()
    w.bits(1, 1)
    w.bits(2, 2)
    w.bits(hlit_field, 5)
    w.bits(hdist_field, 5)
    w.bits(hclen_field, 4)
    for v in cl3:
        w.bits(v, 3)
    return w.getvalue() + b"\0" * 24


_INVALID = None


def invalid():
    """name -> (Stream or raw bytes, the clause of RFC 1951 it breaks, class: 1 block type / stored length, 2 code lengths,
    3 symbol or distance, 5 truncation).  Everything but the truncations is followed by zero bytes, so that no decoder can
    take it for merely cut short."""
    global _INVALID
    if _INVALID is not None:
        return _INVALID
    pad = b"\0" * 16
    ok_lit = lens_of({65: 1, 256: 2, 257: 2}, 258)
    inv = {}
    inv["block_type_3"] = (b"\x07" + pad, "3.2.3: BTYPE 11 is reserved", 1)
    w = BitWriter()
    w.bits(0, 1), w.bits(1, 2)
    for ch in b"abc":
        w.bits(*canonical(FIXED_LIT)[ch])
    w.bits(*canonical(FIXED_LIT)[256])
    w.bits(7, 3)                                                  # BFINAL 1, BTYPE 3 at a bit phase other than 0
    inv["block_type_3_mid_stream"] = (w.getvalue() + pad, "3.2.3: BTYPE 11 is reserved", 1)
    inv["stored_nlen_mismatch"] = (Stream([Stored(b"hello", final=True, nlen=5)], trailing=pad), "3.2.4: NLEN is the complement of LEN", 1)
    inv["stored_nlen_one_bit"] = (Stream([Fixed([65]), Stored(b"hello", final=True, nlen=(5 ^ 0xFFFF) ^ 0x0100)], trailing=pad),
                                  "3.2.4: NLEN is the complement of LEN", 1)
    cl = [0, 0, 0, 1, 1] + [0] * 14                                # symbols 0 and 8: a complete code-length code
    inv["hlit_287"] = (_raw_dynamic_header(30, 0, 15, cl), "3.2.7: HLIT + 257 <= 286", 2)
    inv["hlit_288"] = (_raw_dynamic_header(31, 0, 15, cl), "3.2.7: HLIT + 257 <= 286", 2)
    inv["hdist_31"] = (_raw_dynamic_header(0, 30, 15, cl), "3.2.7: HDIST + 1 <= 30", 2)
    inv["hdist_32"] = (_raw_dynamic_header(0, 31, 15, cl), "3.2.7: HDIST + 1 <= 30", 2)
    inv["cl_code_oversubscribed"] = (_raw_dynamic_header(0, 0, 15, [1, 1, 1] + [0] * 16), "3.2.2: code lengths over-subscribed (code-length code)", 2)
    inv["cl_code_incomplete"] = (_raw_dynamic_header(0, 0, 15, [2, 2, 2] + [0] * 16), "3.2.2: code lengths incomplete (code-length code)", 2)
    inv["cl_code_single"] = (Stream([Dynamic([8] * 257, [8], [], final=True, cl="plain", cl_lens={8: 1}, check=False)], trailing=pad),
                             "3.2.2: a code-length code of one code is incomplete", 2)
    inv["hclen_4_no_lengths"] = (Stream([Dynamic([0] * 257, [0], [], final=True, eob=False, cl=[(18, 127), (18, 98)], cl_lens={18: 1, 0: 1},
                                                 hclen=4, check=False)], trailing=pad),
                                 "3.2.7: HCLEN 4 names 16, 17, 18, 0 alone: all lengths 0, no end-of-block code", 2)
    inv["lit_code_oversubscribed"] = (Stream([Dynamic(lens_of({65: 1, 66: 1, 256: 1}, 257), [0], [], final=True, check=False)], trailing=pad),
                                      "3.2.2: code lengths over-subscribed (literal/length code)", 2)
    inv["dist_code_oversubscribed"] = (Stream([Dynamic(ok_lit, [1, 1, 1], [], final=True, check=False)], trailing=pad),
                                       "3.2.2: code lengths over-subscribed (distance code)", 2)
    inv["lit_code_incomplete"] = (Stream([Dynamic(lens_of({65: 2, 66: 2, 256: 2}, 257), [0], [], final=True, check=False)], trailing=pad),
                                  "3.2.2: code lengths incomplete (literal/length code)", 2)
    inv["dist_code_incomplete"] = (Stream([Dynamic(ok_lit, [2, 2, 2], [], final=True, check=False)], trailing=pad),
                                   "3.2.2: code lengths incomplete (distance code, more than one code)", 2)
    inv["dist_code_single_2_bits"] = (Stream([Dynamic(ok_lit, [2], [], final=True, check=False)], trailing=pad),
                                      "3.2.7: one distance code is sent with ONE bit", 2)
    inv["repeat_first"] = (Stream([Dynamic(ok_lit, [0], [], final=True, check=False,
                                           cl=[(16, 0), (18, 127), (18, 105), (1, 0), (2, 0), (2, 0), (0, 0)])], trailing=pad),
                           "3.2.7: 16 copies the PREVIOUS length: there is none", 2)
    inv["repeat_past_the_end"] = (Stream([Dynamic(ok_lit, [0], [], final=True, check=False,
                                                  cl=[(18, 54), (1, 0), (18, 127), (18, 41), (2, 0), (2, 0), (17, 7)])], trailing=pad),
                                  "3.2.7: a repeat runs past HLIT + HDIST lengths", 2)
    inv["no_end_of_block_code"] = (Stream([Dynamic(lens_of({65: 1, 66: 1}, 257), [0], [65, 66], final=True, eob=False, check=False)], trailing=pad),
                                   "3.2.3: every block ends with symbol 256: it needs a code", 2)
    for s in (286, 287):
        inv["literal_length_symbol_%d" % s] = (Stream([Fixed(list(b"abcdef") + [("lsym", s)], final=True)], trailing=pad),
                                               "3.2.6: literal/length values 286 - 287 never occur", 3)
    for s in (30, 31):
        inv["distance_symbol_%d" % s] = (Stream([Fixed(list(b"abcdef") + [(3, 2), ("mraw", 4, s)], final=True)], trailing=pad),
                                         "3.2.6: distance codes 30 - 31 never occur", 3)
    inv["single_dist_code_other_half"] = (Stream([Dynamic(ok_lit, [1], [65, 65, (3, 1), ("mraw", 3, None), ("bits", 1, 1)], final=True)], trailing=pad),
                                          "3.2.7: the unused half of a single distance code", 3)
    inv["length_without_distance_code"] = (Stream([Dynamic(ok_lit, [0], [65, 65, 65, ("mraw", 3, None)], final=True)], trailing=pad),
                                           "3.2.7: a block of literals only has no distance code to follow a length", 3)
    inv["distance_1_at_position_0"] = (Stream([Fixed([("mraw", 3, 0)], final=True)], trailing=pad), "3.2.5 / 2: a distance reaches before the output", 3)
    inv["distance_2_at_position_1"] = (Stream([Fixed([65, ("mraw", 3, 1)], final=True)], trailing=pad), "3.2.5 / 2: a distance reaches before the output", 3)
    far = Fixed(_fill(32767, seed=6) + [("mraw", 3, 29), ("bits", 8191, 13)], final=True)
    inv["distance_32768_at_position_32767"] = (Stream([far], trailing=pad), "3.2.5 / 2: a distance reaches before the output", 3)
    base = encode(truncation_stream())
    for k in range(len(base)):
        inv["truncated_at_%03d" % k] = (base[:k], "2: the stream ends before its final block does", 5)
    _INVALID = inv
    return inv
