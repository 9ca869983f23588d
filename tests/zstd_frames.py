"""Zstandard frames written field by field from RFC 8878 — tests only.

A frame is described as data (Frame, Raw, RLE, Comp, Lits, Table): the header fields, and for every compressed block its
literals section (raw, RLE, Huffman or treeless; the size format; 1 or 4 streams; weights in direct or FSE-coded form) and
its sequences section (nbSeq; each of the LL / OF / ML tables predefined, RLE, FSE with stated normalized counts, or Repeat;
the sequences as (literal length, match length, Offset_Value) — Offset_Value is the raw field, so repeat codes and the
ll == 0 shift are what the test states, not what an encoder chose).

encode(spec) writes the bytes; expected_output(spec) computes the content by the RFC's rules (an expectation that does not
come from libzstd); forms(spec) names the parts of the format a frame exercises, so that a test can prove what a catalogue
covers.  catalogue() holds named frames aimed at rarely met forms, invalid() frames that break one stated clause, and
random_frame(seed, ...) draws specs (random or FASTQ content) of any size."""
import random
from collections import Counter
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

MAGIC = 0xFD2FB528
BLOCK_MAX = 128 << 10

# ---------------------------------------------------------------------------------------------------------------- codes
# RFC 8878 3.1.1.3.2.1.1: Literals_Length and Match_Length codes (baseline, extra bits)
LL_BASE = [(i, 0) for i in range(16)] + [(16, 1), (18, 1), (20, 1), (22, 1), (24, 2), (28, 2), (32, 3), (40, 3), (48, 4), (64, 6),
                                         (128, 7), (256, 8), (512, 9), (1024, 10), (2048, 11), (4096, 12), (8192, 13),
                                         (16384, 14), (32768, 15), (65536, 16)]
ML_BASE = [(i + 3, 0) for i in range(32)] + [(35, 1), (37, 1), (39, 1), (41, 1), (43, 2), (47, 2), (51, 3), (59, 3), (67, 4),
                                              (83, 4), (99, 5), (131, 7), (259, 8), (515, 9), (1027, 10), (2051, 11), (4099, 12),
                                              (8195, 13), (16387, 14), (32771, 15), (65539, 16)]
# RFC 8878 3.1.1.3.2.2: the predefined distributions
LL_PRE = ([4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1], 6)
ML_PRE = ([1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7, 6)
OF_PRE = ([1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5, 5)
MAX_CODE = (35, 31, 52)   # LL, OF, ML
MAX_LOG = (9, 8, 9)


def _code(base, v):
    lo, hi = 0, len(base) - 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if base[mid][0] <= v:
            lo = mid
        else:
            hi = mid - 1
    b, n = base[lo]
    assert v - b < (1 << n), v
    return lo, v - b, n


def ll_code(ll):
    return _code(LL_BASE, ll)


def ml_code(ml):
    assert ml >= 3
    return _code(ML_BASE, ml)


def of_code(ofv):
    assert ofv >= 1
    c = ofv.bit_length() - 1
    return c, ofv - (1 << c), c


# ---------------------------------------------------------------------------------------------------------------- bits
class FwdBits:
    """forward bit writer, least significant bit first (FSE table descriptions)"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def backward_stream(fields):
    """a backward bitstream (RFC 8878 4.1 / 4.2.2): `fields` are (value, nbits) in the order the DECODER reads them.  The
    stream's last byte holds the 1 marker as its highest set bit; the decoder reads from just below it towards byte 0."""
    s = "1" + "".join(format(v, "0%db" % n) for v, n in fields if n)
    return int(s, 2).to_bytes((len(s) + 7) // 8, "little")


def backward_stream_str(bits):
    s = "1" + bits
    return int(s, 2).to_bytes((len(s) + 7) // 8, "little")


# ---------------------------------------------------------------------------------------------------------------- FSE
class FseTable:
    """the decoding table of RFC 8878 4.1.1 built from normalized counts (-1: "less than one"), with what an encoder needs:
    for every symbol and every next state, the one cell whose range holds it"""

    def __init__(self, counts, log):
        self.counts, self.log = list(counts), log
        size = 1 << log
        assert sum(1 if c == -1 else c for c in counts) == size, (counts, log)
        syms = [None] * size
        high = size - 1
        for s, c in enumerate(counts):
            if c == -1:
                syms[high] = s
                high -= 1
        step, mask, pos = (size >> 1) + (size >> 3) + 3, size - 1, 0
        for s, c in enumerate(counts):
            for _ in range(max(c, 0)):
                syms[pos] = s
                pos = (pos + step) & mask
                while pos > high:
                    pos = (pos + step) & mask
        assert pos == 0
        nxt = {s: (1 if c == -1 else c) for s, c in enumerate(counts) if c}
        self.cells = []
        for u in range(size):
            s = syms[u]
            ns = nxt[s]
            nxt[s] += 1
            nb = log - (ns.bit_length() - 1)
            self.cells.append((s, nb, (ns << nb) - size))
        self._find = {}

    @classmethod
    def rle(cls, code):
        t = cls.__new__(cls)
        t.counts, t.log, t.cells, t._find = None, 0, [(code, 0, 0)], {}
        t.rle_code = code
        return t

    def has(self, s):
        return any(c[0] == s for c in self.cells)

    def find(self, s, nxt_state):
        f = self._find.get(s)
        if f is None:
            f = [None] * len(self.cells)
            for u, (sym, nb, base) in enumerate(self.cells):
                if sym == s:
                    for t in range(base, base + (1 << nb)):
                        f[t] = u
            self._find[s] = f
        return f[nxt_state]

    def chain(self, symbols, last=None):
        """states S_0..S_{n-1} whose symbols are `symbols` and the bits of each transition S_i -> S_{i+1}"""
        n = len(symbols)
        st = [0] * n
        st[-1] = last if last is not None else next(u for u, c in enumerate(self.cells) if c[0] == symbols[-1])
        bits = [None] * n
        for i in range(n - 2, -1, -1):
            u = self.find(symbols[i], st[i + 1])
            assert u is not None, (symbols[i], "not in the table")
            st[i] = u
            bits[i] = (st[i + 1] - self.cells[u][2], self.cells[u][1])
        return st, bits


def fse_description(counts, log):
    """RFC 8878 4.1.1: Accuracy_Log - 5, then the probabilities (value + 1, with the short form below the threshold), a
    2-bit repeat flag chain behind every zero"""
    counts = list(counts)
    while counts and counts[-1] == 0:
        counts.pop()
    w = FwdBits()
    w.put(log - 5, 4)
    remaining, threshold, nbits = (1 << log) + 1, 1 << log, log + 1
    i, prev0 = 0, False
    while remaining > 1:
        if prev0:
            start = i
            while counts[i] == 0:
                i += 1
            run = i - start
            while run >= 3:
                w.put(3, 2)
                run -= 3
            w.put(run, 2)
        c = counts[i]
        i += 1
        mx = (2 * threshold - 1) - remaining
        remaining -= -c if c < 0 else c
        v = c + 1
        if v >= threshold:
            v += mx
        w.put(v, nbits - (1 if v < mx else 0))
        prev0 = c == 0
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
    assert remaining == 1 and i == len(counts), "counts do not sum to the table size"
    return w.bytes()


def normalize(hist, log, rng=None, lt1=0.0, min_syms=2):
    """normalized counts summing to 1 << log; every symbol of `hist` keeps a cell; with `rng` some single cells become -1"""
    size = 1 << log
    hist = dict(hist)
    while len(hist) < min_syms:  # (one symbol alone: give it a neighbour, so that no table is a single state)
        s = max(hist) + 1 if max(hist) + 1 not in hist else min(hist) - 1
        hist[s] = 1
    assert len(hist) <= size
    tot = sum(hist.values())
    cnt = {s: max(1, f * size // tot) for s, f in hist.items()}
    while sum(cnt.values()) > size:
        s = max(cnt, key=lambda k: cnt[k])
        cnt[s] -= 1
    while sum(cnt.values()) < size:
        s = max(hist, key=lambda k: hist[k] / cnt[k])
        cnt[s] += 1
    out = [0] * (max(cnt) + 1)
    for s, c in cnt.items():
        out[s] = -1 if (c == 1 and rng is not None and rng.random() < lt1) else c
    return out


# ---------------------------------------------------------------------------------------------------------------- Huffman
def huf_codes(weights):
    """canonical prefix codes from weights (RFC 8878 4.2.1.3): {symbol: (code, nbits)}, max bits"""
    total = sum(1 << (w - 1) for w in weights if w)
    mb = total.bit_length() - 1
    assert total == 1 << mb, "weights do not make a complete code"
    codes, nxt = {}, 0
    for w in range(1, mb + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (nxt, mb + 1 - w)
                nxt += 1
        nxt >>= 1
    return codes, mb


def huf_weights(data, max_bits=11):
    """weights of a (length-limited) Huffman code for the bytes of `data`; a lone symbol gets a neighbour"""
    import heapq
    freq = dict(Counter(data))
    if len(freq) == 1:
        s = next(iter(freq))
        freq[s ^ 1] = 1
    while True:
        h = [(f, i, (s,)) for i, (s, f) in enumerate(sorted(freq.items()))]
        heapq.heapify(h)
        depth = dict.fromkeys(freq, 0)
        k = len(h)
        while len(h) > 1:
            f1, _, a = heapq.heappop(h)
            f2, _, b = heapq.heappop(h)
            for s in a + b:
                depth[s] += 1
            heapq.heappush(h, (f1 + f2, k, a + b))
            k += 1
        mx = max(depth.values())
        if mx <= max_bits:
            break
        freq = {s: (f >> 1) | 1 for s, f in freq.items()}
    w = [0] * (max(freq) + 1)
    for s, d in depth.items():
        w[s] = mx + 1 - d
    return w


def huf_description(weights, form="auto", log=6):
    """the Huffman tree description (RFC 8878 4.2.1): every weight but the last (derived), direct (header >= 128, two 4-bit
    weights a byte) or FSE-coded (header < 128: a table description and a stream of two interleaved states)"""
    stated = list(weights[:-1])
    n = len(stated)
    huf_codes(weights)  # (asserts that the last weight is the one that completes the code)
    if form == "auto":
        form = "fse" if n >= 2 else "direct"
        if form == "fse":
            try:
                d = _huf_fse_weights(stated, log)
                if len(d) < 128:
                    return bytes([len(d)]) + d
            except AssertionError:
                pass
            form = "direct"
    if form == "direct":
        assert 1 <= n <= 128
        body = bytearray()
        for i in range(0, n, 2):
            body.append((stated[i] << 4) | (stated[i + 1] if i + 1 < n else 0))
        return bytes([127 + n]) + bytes(body)
    d = _huf_fse_weights(stated, log)
    assert len(d) < 128
    return bytes([len(d)]) + d


def _huf_fse_weights(stated, log):
    assert len(stated) >= 2  # the decoder always emits the symbols of both states
    counts = normalize(Counter(stated), log)
    t = FseTable(counts, log)
    n = len(stated)
    # the update behind stated[n-2] must read past the stream's start: its state is a cell with bits to read
    ends = {}
    x = (n - 2) % 2
    ends[x] = max((u for u, c in enumerate(t.cells) if c[0] == stated[n - 2]), key=lambda u: t.cells[u][1])
    assert t.cells[ends[x]][1] >= 1
    states, trans = {}, {}
    for par in (0, 1):
        pos = list(range(par, n, 2))
        if par == x:
            pos = [p for p in pos if p <= n - 2]
        else:
            pos = [p for p in pos if p <= n - 1]
        st, bits = t.chain([stated[p] for p in pos], ends.get(par))
        for p, s_, b in zip(pos, st, bits):
            states[p], trans[p] = s_, b
    fields = [(states[0], log), (states[1], log)] + [trans[i] for i in range(n - 2)]
    return fse_description(counts, log) + backward_stream(fields)


# ---------------------------------------------------------------------------------------------------------------- spec
@dataclass
class Lits:
    kind: str = "raw"                  # raw | rle | huf | treeless
    data: bytes = b""
    size_format: Optional[int] = None  # None: the smallest that fits (raw / RLE: header of 1, 2, 3 bytes -> 0, 1, 3)
    streams: Optional[int] = None      # None: 1 below 1024 literals, else 4
    weights: Optional[list] = None     # huf: every symbol's weight, the last one included; None: from the data
    weight_form: str = "auto"          # direct | fse | auto
    weight_log: int = 6


@dataclass
class Table:
    mode: str = "pre"                  # pre | rle | fse | rep
    code: int = 0
    counts: Optional[list] = None
    log: int = 0


PRE = Table("pre")
REP = Table("rep")


def rle(code):
    return Table("rle", code=code)


def fse(counts, log):
    return Table("fse", counts=list(counts), log=log)


@dataclass
class Raw:
    data: bytes


@dataclass
class RLE:
    byte: int
    n: int


@dataclass
class Comp:
    lits: Lits
    seqs: List[Tuple[int, int, int]] = field(default_factory=list)   # (ll, ml, Offset_Value)
    tables: Tuple[Table, Table, Table] = (PRE, PRE, PRE)               # LL, OF, ML
    nseq_bytes: Optional[int] = None


@dataclass
class Frame:
    blocks: list
    window_log: int = 17
    mantissa: int = 0
    single: bool = False
    fcs: object = None                # None: absent (single segment: present); True: the real size; an int: that value
    fcs_bytes: Optional[int] = None   # forced field width (1 only in single segment)
    checksum: bool = False
    reserved_type: Optional[int] = None   # (invalid frames: this block's header says type 3)

    def window(self):
        if self.single:
            return len(expected_output(self))
        return (1 << self.window_log) + ((1 << self.window_log) >> 3) * self.mantissa


# ---------------------------------------------------------------------------------------------------------------- writer
def _lit_header(kind, sf, regen, csize=0):
    t = {"raw": 0, "rle": 1, "huf": 2, "treeless": 3}[kind]
    if t < 2:
        if sf in (0, 2):
            assert regen < 32
            return bytes([t | (regen << 3)])
        if sf == 1:
            assert regen < 4096
            return bytes([t | 4 | ((regen & 15) << 4), regen >> 4])
        assert regen < (1 << 20)
        v = t | 12 | (regen << 4)
        return v.to_bytes(3, "little")
    bits, nb = {0: (10, 3), 1: (10, 3), 2: (14, 4), 3: (18, 5)}[sf]
    assert regen < (1 << bits) and csize < (1 << bits), (regen, csize, sf)
    v = t | (sf << 2) | (regen << 4) | (csize << (4 + bits))
    return v.to_bytes(nb, "little")


def _huf_streams(data, codes, streams):
    cs = {s: format(c, "0%db" % n) for s, (c, n) in codes.items()}

    def one(seg):
        return backward_stream_str("".join(cs[b] for b in seg))
    if streams == 1:
        return one(data)
    q = (len(data) + 3) // 4
    parts = [one(data[i * q:(i + 1) * q]) for i in range(3)] + [one(data[3 * q:])]
    jump = b"".join(len(p).to_bytes(2, "little") for p in parts[:3])
    return jump + b"".join(parts)


def lits_section(L: Lits, st):
    d = L.data
    if L.kind in ("raw", "rle"):
        sf = L.size_format
        if sf is None:
            sf = 0 if len(d) < 32 else 1 if len(d) < 4096 else 3
        if L.kind == "rle":
            assert len(set(d)) <= 1 and len(d) > 0
            return _lit_header("rle", sf, len(d)) + d[:1]
        return _lit_header("raw", sf, len(d)) + d
    if L.kind == "huf":
        w = L.weights if L.weights is not None else huf_weights(d)
        st["tree"] = w
        tree = huf_description(w, L.weight_form, L.weight_log)
    else:
        w = st.get("tree") or L.weights or huf_weights(d)   # (no tree in front: an invalid frame states one to write with)
        tree = b""
    codes, _ = huf_codes(w)
    streams = L.streams or (1 if len(d) < 1024 else 4)
    body = tree + _huf_streams(d, codes, streams)
    sf = L.size_format
    if sf is None:
        sf = 0 if streams == 1 else 1 if max(len(d), len(body)) < 1024 else 2 if max(len(d), len(body)) < 16384 else 3
    assert (sf == 0) == (streams == 1)
    return _lit_header(L.kind, sf, len(d), len(body)) + body


def _nseq(n, width=None):
    if width is None:
        width = 1 if n < 128 else 2 if n < 0x7F00 else 3
    if width == 1:
        assert n < 128
        return bytes([n])
    if width == 2:
        assert n < 0x7F00
        return bytes([128 + (n >> 8), n & 255])
    return bytes([255, (n - 0x7F00) & 255, (n - 0x7F00) >> 8])


def _table_of(kind, T: Table, st, codes):
    """the table a block decodes `kind` (0 LL, 1 OF, 2 ML) with, and the bytes that describe it"""
    if T.mode == "pre":
        t = FseTable(*(LL_PRE, OF_PRE, ML_PRE)[kind])
        st["tbl"][kind] = t
        return t, 0, b""
    if T.mode == "rle":
        t = FseTable.rle(T.code)
        st["tbl"][kind] = t
        return t, 1, bytes([T.code])
    if T.mode == "fse":
        t = FseTable(T.counts, T.log)
        st["tbl"][kind] = t
        return t, 2, fse_description(T.counts, T.log)
    t = st["tbl"][kind] or FseTable(*(LL_PRE, OF_PRE, ML_PRE)[kind])  # (nothing to repeat: an invalid frame)
    return t, 3, b""


def seqs_section(C: Comp, st):
    n = len(C.seqs)
    out = bytearray(_nseq(n, C.nseq_bytes))
    if n == 0:
        return bytes(out)
    lls = [ll_code(ll) for ll, _, _ in C.seqs]
    ofs = [of_code(o) for _, _, o in C.seqs]
    mls = [ml_code(ml) for _, ml, _ in C.seqs]
    modes, descs, tabs = 0, b"", []
    for k, (T, cs) in enumerate(zip(C.tables, (lls, ofs, mls))):
        t, m, d = _table_of(k, T, st, cs)
        modes |= m << (6 - 2 * k)
        descs += d
        tabs.append(t)
    out.append(modes)
    out += descs
    chains = [t.chain([c[0] for c in cs]) for t, cs in zip(tabs, (lls, ofs, mls))]
    (s_ll, b_ll), (s_of, b_of), (s_ml, b_ml) = chains
    fields = [(s_ll[0], tabs[0].log), (s_of[0], tabs[1].log), (s_ml[0], tabs[2].log)]
    for i in range(n):
        fields += [(ofs[i][1], ofs[i][2]), (mls[i][1], mls[i][2]), (lls[i][1], lls[i][2])]
        if i + 1 < n:
            fields += [b_ll[i], b_ml[i], b_of[i]]
    out += backward_stream(fields)
    return bytes(out)


def _block(last, btype, size, body):
    return (last | (btype << 1) | (size << 3)).to_bytes(3, "little") + body


def encode_frame(F: Frame, content=None):
    st = {"tree": None, "tbl": [None, None, None]}
    if content is None and (F.fcs is True or F.single or F.checksum):
        content = expected_output(F)
    fhd = (4 if F.checksum else 0) | (32 if F.single else 0)
    fcs_val = F.fcs if isinstance(F.fcs, int) and F.fcs is not True else (len(content) if (F.fcs is True or F.single) else None)
    fb = F.fcs_bytes
    if fcs_val is not None and fb is None:
        fb = (1 if F.single and fcs_val < 256 else 2 if 256 <= fcs_val < 65536 + 256 else 4 if fcs_val < (1 << 32) else 8)
    if fcs_val is None:
        fb = 0
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fb]
    assert fb != 1 or F.single
    fhd |= flag << 6
    out = bytearray(MAGIC.to_bytes(4, "little"))
    out.append(fhd)
    if not F.single:
        assert 10 <= F.window_log <= 41
        out.append(((F.window_log - 10) << 3) | F.mantissa)
    if fb:
        out += (fcs_val - (256 if fb == 2 else 0)).to_bytes(fb, "little")
    for i, B in enumerate(F.blocks):
        last = int(i == len(F.blocks) - 1)
        if isinstance(B, Raw):
            blk = _block(last, 0, len(B.data), B.data)
        elif isinstance(B, RLE):
            blk = _block(last, 1, B.n, bytes([B.byte]))
        else:
            body = lits_section(B.lits, st) + seqs_section(B, st)
            blk = _block(last, 2, len(body), body)
        if F.reserved_type == i:
            blk = bytes([blk[0] | 6]) + blk[1:]
        out += blk
    if F.checksum:
        out += xxh64_low32(content)
    return bytes(out)


def xxh64_low32(content):
    """Content_Checksum: the low 4 bytes of XXH64(content, seed 0) — read out of a frame libzstd writes over the same
    content with its checksum flag set (the frame's last 4 bytes)"""
    from zstd_util import compress
    return compress(content, 1, True)[-4:]


def encode(spec):
    """a Frame, or a list of Frames / bytes (skippable frames, raw bytes) in a row"""
    if isinstance(spec, Frame):
        return encode_frame(spec)
    return b"".join(s if isinstance(s, (bytes, bytearray)) else encode_frame(s) for s in spec)


# ---------------------------------------------------------------------------------------------------------------- content
def apply_ofv(hist, ll, ofv):
    """RFC 8878 3.1.1.5: (offset, new repeat-offset history) of one sequence"""
    r0, r1, r2 = hist
    if ofv > 3:
        off = ofv - 3
        return off, (off, r0, r1)
    idx = ofv - 1 + (ll == 0)
    if idx == 0:
        return r0, hist
    if idx == 1:
        return r1, (r1, r0, r2)
    if idx == 2:
        return r2, (r2, r0, r1)
    return r0 - 1, (r0 - 1, r0, r1)


def _copy(out, off, ml):
    assert 1 <= off <= len(out), ("offset", off, len(out))
    start = len(out) - off
    if off >= ml:
        out += out[start:start + ml]
        return
    while ml > 0:
        k = min(ml, len(out) - start)
        out += out[start:start + k]
        ml -= k


def frame_content(F: Frame, frame_start=0, out=None):
    out = bytearray() if out is None else out
    base = len(out)
    hist = (1, 4, 8)
    for B in F.blocks:
        if isinstance(B, Raw):
            out += B.data
        elif isinstance(B, RLE):
            out += bytes([B.byte]) * B.n
        else:
            lit = B.lits.data
            p = 0
            for ll, ml, ofv in B.seqs:
                out += lit[p:p + ll]
                p += ll
                assert p <= len(lit)
                off, hist = apply_ofv(hist, ll, ofv)
                assert off <= len(out) - base, "match reaches in front of the frame"
                _copy(out, off, ml)
            out += lit[p:]
    return out


def expected_output(spec):
    out = bytearray()
    for F in ([spec] if isinstance(spec, Frame) else spec):
        if isinstance(F, Frame):
            frame_content(F, out=out)
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------- forms
REQUIRED_FORMS = (
    # offsets
    {"of:rep3_ll0", "of:rep3_ll0_r0_symbolic", "of:rep_at_block_start", "of:rep_across_empty_blocks", "of:rep_src_128k_back",
     "of:match_to_frame_start", "of:rep1_ll0", "of:rep2_ll0", "of:rep1", "of:rep2", "of:rep3"}
    | {"of:code%d" % c for c in range(24, 28)}
    # entropy state carried between blocks
    | {"tbl:rep_fse", "tbl:rep_rle", "tbl:rep_pre", "tbl:rep_across_nseq0", "tbl:rep_across_raw", "tbl:rep_across_rle",
       "tbl:rep_src_128k_back", "lit:treeless", "lit:treeless_across_blocks", "lit:treeless_src_128k_back", "lit:treeless_4s"}
    # literals
    | {"lit:%s_h%d" % (k, h) for k in ("raw", "rle") for h in (1, 2, 3)}
    | {"lit:%s_%d" % (k, n) for k in ("raw", "rle") for n in (31, 32, 4095, 4096)}
    | {"lit:huf_sf%d" % s for s in range(4)} | {"lit:huf_%d" % n for n in (1023, 1024, 16383, 16384)} | {"lit:huf_128k"}
    | {"lit:4s_tiny_short_last", "lit:w_direct_odd", "lit:w_direct_even", "lit:w_direct_128", "lit:w_fse_2sym",
       "lit:w_fse_255", "lit:w_maxbits11"}
    # sequences
    | {"nseq:0", "nseq:127", "nseq:128", "nseq:0x7eff", "nseq:0x7f00", "nseq:>0x7f00"}
    | {"fse:ll_log5", "fse:ll_log9", "fse:of_log5", "fse:of_log8", "fse:ml_log5", "fse:ml_log9", "fse:lt1", "fse:zero_chain"}
    | {"rle:ll35", "rle:ml52", "ml:block_max"} | {"rle:of%d" % c for c in range(28)}
    # frame and block headers
    | {"fh:fcs0", "fh:fcs1", "fh:fcs2", "fh:fcs4", "fh:fcs8", "fh:single", "fh:mantissa", "fh:checksum",
       "blk:rle_128k_between", "blk:raw_between"}
    # errors
    | {"err:reserved_block", "err:block_over_window", "err:fcs_mismatch", "err:treeless_first", "err:repeat_first", "err:offset_past_start",
       "err:ml_past_block"}
)


def forms(spec):
    fs = set()
    for F in ([spec] if isinstance(spec, Frame) else spec):
        if isinstance(F, Frame):
            _frame_forms(F, fs)
    return fs


def _frame_forms(F, fs):
    fb = F.fcs_bytes
    has_fcs = F.fcs is not None or F.single
    if has_fcs and fb is None:
        v = F.fcs if isinstance(F.fcs, int) and F.fcs is not True else len(expected_output(F))
        fb = 1 if F.single and v < 256 else 2 if 256 <= v < 65792 else 4 if v < (1 << 32) else 8
    fs.add("fh:fcs%d" % (fb if has_fcs else 0))
    if F.single:
        fs.add("fh:single")
    if F.mantissa:
        fs.add("fh:mantissa")
    if F.checksum:
        fs.add("fh:checksum")
    if F.reserved_type is not None:
        fs.add("err:reserved_block")
    if isinstance(F.fcs, int) and F.fcs is not True and F.fcs != len(expected_output(F)):
        fs.add("err:fcs_mismatch")
    hist, produced = (1, 4, 8), 0
    win = None if F.single else F.window()
    for B in F.blocks:
        if isinstance(B, Raw) and win is not None and len(B.data) > min(win, BLOCK_MAX):
            fs.add("err:block_over_window")
    tree_at = None            # output position of the block that carried the tree
    tbl_at = [None] * 3
    F_last_seq_at = None      # output position where the last block with sequences ended
    since_seq = []            # block kinds since the last block with sequences
    kinds = [type(b).__name__ for b in F.blocks]
    for i, B in enumerate(F.blocks):
        if isinstance(B, (Raw, RLE)):
            n = len(B.data) if isinstance(B, Raw) else B.n
            if 0 < i < len(F.blocks) - 1 and "Comp" in kinds[:i] and "Comp" in kinds[i + 1:]:
                fs.add("blk:raw_between" if isinstance(B, Raw) else ("blk:rle_128k_between" if n == BLOCK_MAX else "blk:rle_between"))
            since_seq.append("raw" if isinstance(B, Raw) else "rle")
            produced += n
            continue
        L = B.lits
        n = len(L.data)
        if L.kind in ("raw", "rle"):
            sf = L.size_format if L.size_format is not None else (0 if n < 32 else 1 if n < 4096 else 3)
            fs.add("lit:%s_h%d" % (L.kind, {0: 1, 2: 1, 1: 2, 3: 3}[sf]))
            if n in (31, 32, 4095, 4096):
                fs.add("lit:%s_%d" % (L.kind, n))
        else:
            body = lits_section(L, {"tree": F_tree_guess(F, i)})
            sf = (body[0] >> 2) & 3
            fs.add("lit:%s_sf%d" % ("huf" if L.kind == "huf" else "treeless", sf))
            if L.kind == "huf" and n in (1023, 1024, 16383, 16384):
                fs.add("lit:huf_%d" % n)
            if L.kind == "huf" and n >= 120 << 10:
                fs.add("lit:huf_128k")
            if (L.streams or (1 if n < 1024 else 4)) == 4 and n < 16 and n - 3 * ((n + 3) // 4) < (n + 3) // 4:
                fs.add("lit:4s_tiny_short_last")
            if L.kind == "huf":
                w = L.weights if L.weights is not None else huf_weights(L.data)
                desc = huf_description(w, L.weight_form, L.weight_log)
                nw = len(w) - 1
                if desc[0] >= 128:
                    fs.add("lit:w_direct_odd" if nw % 2 else "lit:w_direct_even")
                    if nw == 128:
                        fs.add("lit:w_direct_128")
                else:
                    if sum(1 for x in w if x) == 2:
                        fs.add("lit:w_fse_2sym")
                    if nw >= 254:
                        fs.add("lit:w_fse_255")
                if huf_codes(w)[1] == 11:
                    fs.add("lit:w_maxbits11")
                tree_at = produced
            else:
                fs.add("lit:treeless")
                if tree_at is None:
                    fs.add("err:treeless_first")
                else:
                    if i > 0 and not (isinstance(F.blocks[i - 1], Comp) and F.blocks[i - 1].lits.kind == "huf"):
                        fs.add("lit:treeless_across_blocks")
                    if produced - tree_at >= 128 << 10:
                        fs.add("lit:treeless_src_128k_back")
                if (L.streams or (1 if n < 1024 else 4)) == 4:
                    fs.add("lit:treeless_4s")
        ns = len(B.seqs)
        for v, name in ((0, "0"), (127, "127"), (128, "128"), (0x7EFF, "0x7eff"), (0x7F00, "0x7f00")):
            if ns == v:
                fs.add("nseq:" + name)
        if ns > 0x7F00:
            fs.add("nseq:>0x7f00")
        if ns == 0:
            since_seq.append("nseq0")
            produced += n
            continue
        for k, T in enumerate(B.tables):
            nm = "ll of ml".split()[k]
            if T.mode == "rep":
                if tbl_at[k] is None:
                    fs.add("err:repeat_first")
                else:
                    fs.add("tbl:rep_" + tbl_at[k][1])
                    for s in set(since_seq):
                        fs.add("tbl:rep_across_" + s)
                    if produced - tbl_at[k][0] >= 128 << 10:
                        fs.add("tbl:rep_src_128k_back")
            else:
                tbl_at[k] = (produced, T.mode)
            if T.mode == "fse":
                fs.add("fse:%s_log%d" % (nm, T.log))
                if -1 in T.counts:
                    fs.add("fse:lt1")
                c = T.counts
                run = 0
                for x in c:
                    run = run + 1 if x == 0 else 0
                    if run >= 5:
                        fs.add("fse:zero_chain")
            if T.mode == "rle":
                if (k, T.code) in ((0, 35), (2, 52)):
                    fs.add("rle:%s%d" % (nm, T.code))
                if k == 1:
                    fs.add("rle:of%d" % T.code)
        out_before = produced
        explicit_seen = False
        last_seq_at = F_last_seq_at
        p = 0
        for j, (ll, ml, ofv) in enumerate(B.seqs):
            p += ll
            if ofv <= 3:
                tag = "of:rep%d%s" % (ofv, "_ll0" if ll == 0 else "")
                fs.add(tag)
                if not explicit_seen and out_before > 0:
                    fs.add("of:rep_at_block_start")
                    if since_seq:
                        fs.add("of:rep_across_empty_blocks")
                if ofv == 3 and ll == 0 and not explicit_seen and out_before > 0:
                    fs.add("of:rep3_ll0_r0_symbolic")
            else:
                explicit_seen = True
            off, nh = apply_ofv(hist, ll, ofv)
            cur = produced + p
            if off == cur:
                fs.add("of:match_to_frame_start")
            if off > cur or off == 0:
                fs.add("err:offset_past_start" if off > cur else "err:rep3_zero")
            if ofv <= 3 and not explicit_seen and last_seq_at is not None and out_before - last_seq_at >= 128 << 10:
                fs.add("of:rep_src_128k_back")
            hist = nh
            p += ml
            c = ofv.bit_length() - 1
            if c >= 24:
                fs.add("of:code%d" % c)
        if p + (n - sum(s[0] for s in B.seqs)) > BLOCK_MAX:
            fs.add("err:ml_past_block")
        elif p + (n - sum(s[0] for s in B.seqs)) == BLOCK_MAX and any(ml_code(s[1])[0] == 52 for s in B.seqs):
            fs.add("ml:block_max")
        produced += p + (n - sum(s[0] for s in B.seqs))
        F_last_seq_at = produced
        since_seq = []


def F_tree_guess(F, i):
    for B in reversed(F.blocks[:i]):
        if isinstance(B, Comp) and B.lits.kind == "huf":
            return B.lits.weights if B.lits.weights is not None else huf_weights(B.lits.data)
    return None


# ---------------------------------------------------------------------------------------------------------------- catalogue
def _alpha(n, seed, alphabet=b"ACGT"):
    r = random.Random(seed)
    return bytes(r.choice(alphabet) for _ in range(n))


def _noise(n, seed):
    return random.Random(seed).randbytes(n)


def _lits_headers():
    blocks = []
    for kind in ("raw", "rle"):
        for n, sf in ((31, 0), (31, 1), (32, 1), (4095, 1), (4096, 3), (5, 3), (0, 1), (17, 2)):
            if kind == "rle" and n == 0:   # (a compressed block is at least 3 bytes: an empty 1-byte header would leave 2)
                continue
            d = b"q" * n if kind == "rle" else _noise(n, n)
            blocks.append(Comp(Lits(kind, d, sf)))
    # raw literals with a sequence behind them
    blocks.append(Comp(Lits("raw", _noise(40, 1)), [(40, 10, 40 + 3)]))
    return Frame(blocks, window_log=17, fcs=True)


def _huf_sizes():
    blocks = []
    for n, streams, sf in ((1023, 1, 0), (1023, 4, 1), (1024, 4, 2), (16383, 4, 2), (16384, 4, 3), (300, 4, 3), (BLOCK_MAX, 4, 3)):
        blocks.append(Comp(Lits("huf", _alpha(n, n), sf, streams)))
    blocks.append(Comp(Lits("treeless", _alpha(1023, 7), 0, 1)))
    blocks.append(Comp(Lits("treeless", _alpha(16384, 8), 3, 4)))
    return Frame(blocks, window_log=17, fcs=True)


def _huf_4streams_tiny():
    return Frame([Comp(Lits("huf", b"ACGTACG", 1, 4)), Comp(Lits("huf", b"TTGACCAGTA", 1, 4)),
                  Comp(Lits("treeless", b"GATTACA", 1, 4), [(7, 4, 7 + 3)])], checksum=True, fcs=True)


def _zipf(nsym, n, seed, s=1.2):
    r = random.Random(seed)
    w = [1.0 / (k + 1) ** s for k in range(nsym)]
    d = bytearray(r.choices(range(nsym), weights=w, k=n))
    d += bytes(range(nsym))   # every symbol at least once
    return bytes(d)


def _huf_weights_direct():
    return Frame([Comp(Lits("huf", _zipf(6, 500, 1), weight_form="direct")),      # 5 stated weights
                  Comp(Lits("huf", _zipf(7, 500, 2), weight_form="direct")),      # 6
                  Comp(Lits("huf", _zipf(129, 20000, 3), None, 4, weight_form="direct"))], fcs=True)  # 128


def _huf_weights_fse():
    two = b"ab" * 50 + b"a" * 30
    w2 = [0] * 97 + [1, 1]
    return Frame([Comp(Lits("huf", two, weights=w2, weight_form="fse")),
                  Comp(Lits("huf", _zipf(256, 60000, 4, 2.0), None, 4, weight_form="fse")),   # 255 stated, max 11 bits
                  Comp(Lits("treeless", _zipf(256, 3000, 5, 2.0), None, 4))], fcs=True, checksum=True)


def _treeless_chain():
    d = _alpha(3000, 11, b"ACGTN")
    return Frame([Comp(Lits("huf", d, streams=4), [(100, 50, 100 + 3)]), Raw(_noise(500, 2)), RLE(7, 1000),
                  Comp(Lits("raw", b"xyz")), Comp(Lits("treeless", _alpha(900, 12, b"ACG")), [(5, 20, 1)]),
                  Comp(Lits("treeless", _alpha(5000, 13, b"TN"), streams=4), [(0, 30, 2), (10, 4, 3)])],
                 window_log=16, mantissa=3, checksum=True)


def _nseq_edges():
    blocks = [Raw(_noise(64, 3))]
    for n in (0, 127, 128, 0x7EFF, 0x7F00, 40000):
        lit = _noise(8, n)
        seqs = [(8, 3, 4 + 3)] + [(0, 3, 1)] * (n - 1) if n else []
        blocks.append(Comp(Lits("raw", lit), seqs))
    blocks.append(Comp(Lits("raw", b"ab"), [(2, 3, 1)] + [(0, 3, 1)] * 4, nseq_bytes=2))   # (a count of 5 in the 2-byte form)
    return Frame(blocks, window_log=17)


def _fse_edges():
    r = random.Random(21)
    lits = _noise(6000, 4)
    seqs = []
    lls = [0, 1, 24, 25, 2050]          # codes 0, 1, 20, 20, 30
    mls = [3, 12, 70, 515]               # codes 0, 9, 40, 45
    ofvs = [1, 2, 3, 5, 20, 100, 1000]
    used = 0
    for i in range(120):
        ll = r.choice(lls[:4]) if i != 7 else 2050
        seqs.append((ll, r.choice(mls), r.choice(ofvs) if i else 1000 + 3))
        used += ll
    assert used <= len(lits)
    ll_c = Counter(ll_code(s[0])[0] for s in seqs)
    of_c = Counter(of_code(s[2])[0] for s in seqs)
    ml_c = Counter(ml_code(s[1])[0] for s in seqs)
    # extra symbols at count 0 in the histogram: single cells, some of them "less than one"
    hi_ll, hi_of, hi_ml = {**ll_c, 35: 0, 33: 0}, {**of_c, 12: 0, 31: 0}, {**ml_c, 52: 0, 50: 0}
    big = (fse(normalize(hi_ll, 9, r, 1.0), 9), fse(normalize(hi_of, 8, r, 1.0), 8), fse(normalize(hi_ml, 9, r, 1.0), 9))
    small = (fse(normalize(ll_c, 5, r, 0.5), 5), fse(normalize(of_c, 5, r, 0.5), 5), fse(normalize(ml_c, 5, r, 0.5), 5))
    return Frame([Raw(_noise(4096, 5)), Comp(Lits("raw", lits), seqs, big), Comp(Lits("huf", _alpha(6000, 6)), seqs, small),
                  Comp(Lits("treeless", _alpha(6000, 7)), seqs, (REP, REP, REP))], window_log=18, fcs=True)


def _rle_codes_small():
    """RLE tables at the extreme codes: LL 35, ML 52, OF 0 .. 16"""
    blocks = [Raw(_noise(BLOCK_MAX, 6)), RLE(0x41, BLOCK_MAX)]
    lit = _noise(70000, 7)
    blocks.append(Comp(Lits("raw", lit), [(66000, 3, 9 + 3)], (rle(35), rle(of_code(12)[0]), rle(0))))
    blocks.append(Comp(Lits("raw", b"0123456789"), [(10, 65539 + 1000, 1)], (rle(10), rle(0), rle(52))))
    for k in range(17):
        ofv = (1 << k) + (k * 7919 % (1 << k) if k else 0)
        ll = 3 if ofv <= 3 else 2
        blocks.append(Comp(Lits("raw", _noise(ll, k)), [(ll, 5 + k, ofv)], (rle(ll_code(ll)[0]), rle(k), rle(ml_code(5 + k)[0]))))
    return Frame(blocks, window_log=17, fcs=True)


def _rle_codes_16m():
    """OF codes 17 .. 23 in RLE mode, over 16 MiB of history made of RLE blocks (each its own byte) and a random start"""
    blocks, produced = [Raw(_noise(1 << 16, 9))], 1 << 16
    todo = list(range(17, 24))
    b = 0
    while todo:
        k = todo[0]
        if produced + 3 >= (1 << k) + 1000:
            ofv = (1 << k) + 1000
            blocks.append(Comp(Lits("raw", b"@" * 4), [(4, 200, ofv)], (rle(4), rle(k), rle(ml_code(200)[0]))))
            produced += 204
            todo.pop(0)
            continue
        blocks.append(RLE(b & 255, BLOCK_MAX))
        produced += BLOCK_MAX
        b += 37
    return Frame(blocks, window_log=24)


def _rep_offsets():
    lit = _noise(200, 8)
    b1 = Comp(Lits("raw", lit), [(10, 5, 20 + 3), (5, 4, 1), (3, 4, 2), (2, 4, 3), (0, 4, 1), (0, 4, 2), (0, 4, 3), (0, 6, 40 + 3),
                                 (7, 5, 1), (0, 7, 3)],
              (fse(normalize(Counter([10, 5, 3, 2, 0, 7]), 6), 6), PRE, PRE))
    b2 = Comp(Lits("raw", _noise(30, 9)))                      # nbSeq 0
    b5 = Comp(Lits("raw", _noise(3, 10)), [(0, 5, 3), (3, 6, 1), (0, 4, 1), (0, 4, 2)], (REP, PRE, REP))   # r0 - 1 at the block's start
    b6 = Comp(Lits("raw", _noise(9, 11)), [(4, 5, 1), (5, 9, 2)], (PRE, PRE, PRE))
    return Frame([Raw(_noise(100, 7)), b1, b2, Raw(_noise(77, 12)), RLE(3, 500), b5, Raw(b"zz"), b6], window_log=12, checksum=True)


def _repeat_tables_far():
    lits = _noise(400, 13)
    s1 = [(3, 4, 50 + 3), (2, 4, 1), (5, 4, 60 + 3), (1, 4, 1)]
    ta = (fse(normalize(Counter(ll_code(s[0])[0] for s in s1), 7), 7), fse(normalize(Counter(of_code(s[2])[0] for s in s1), 5), 5), PRE)
    s2 = [(5, 4, 1), (3, 4, 50 + 3), (1, 4, 60 + 3)]
    s3 = [(3, 4, 1), (2, 4, 60 + 3)]
    t_rle = (rle(ll_code(2)[0]), rle(of_code(10 + 3)[0]), rle(ml_code(6)[0]))
    s4 = [(2, 6, 13), (2, 6, 13)]
    return Frame([Raw(_noise(300, 14)), Comp(Lits("raw", lits), s1, ta), Comp(Lits("raw", b"k" * 9)), Raw(b"raw"), RLE(1, 999),
                  Comp(Lits("rle", b"u" * 20), s2, (REP, REP, REP)), Comp(Lits("raw", b"ab")), Comp(Lits("raw", lits[:20]), s3, (REP, REP, REP)),
                  Comp(Lits("raw", b"1234"), s4, t_rle), RLE(9, 20), Comp(Lits("raw", b"5678"), s4, (REP, REP, REP))], window_log=11)


def _chunk_crossing():
    """repeat offsets, Repeat_Mode tables and a treeless tree whose source lies 256 KiB back (behind RLE blocks: another
    device chunk at its 128 KiB target)"""
    d = _alpha(4000, 15, b"ACGTN")
    s1 = [(100, 30, 777 + 3), (50, 40, 1)]
    tabs = (fse(normalize(Counter(ll_code(s[0])[0] for s in s1), 6), 6), fse(normalize(Counter(of_code(s[2])[0] for s in s1), 5), 5),
            fse(normalize(Counter(ml_code(s[1])[0] for s in s1), 6), 6))
    s2 = [(50, 40, 1), (100, 30, 1), (100, 40, 1)]
    return Frame([Raw(_noise(1000, 16)), Comp(Lits("huf", d), s1, tabs), RLE(0x30, BLOCK_MAX), RLE(0x31, BLOCK_MAX), Raw(_noise(1000, 17)),
                  Comp(Lits("treeless", _alpha(3000, 18, b"ACGTN")), s2, (REP, REP, REP)), RLE(0x32, BLOCK_MAX),
                  Comp(Lits("treeless", _alpha(300, 19, b"AC"), streams=4), [(0, 9, 2), (30, 3, 1)], (PRE, PRE, PRE))],
                 window_log=20, fcs=True, checksum=True)


def _headers():
    """frames of every Frame_Content_Size width, single segment, window mantissas"""
    fr = [Frame([Raw(b"single")], single=True),
          Frame([Raw(b"")], single=True),
          Frame([Raw(_noise(256, 20))], single=True),                                    # 2 bytes, 256 = the +256 form's 0
          Frame([RLE(5, 65535 - 2), Raw(_noise(258, 21))], window_log=17, fcs=True),      # 2 bytes, 65791: its largest
          Frame([RLE(5, 65536 - 2), Raw(_noise(258, 22))], window_log=17, fcs=True),      # 4 bytes, 65792
          Frame([Raw(_noise(100, 23))], fcs=True, fcs_bytes=8, window_log=10),
          Frame([Raw(_noise(100, 24))], fcs=True, fcs_bytes=4, window_log=10),
          Frame([Comp(Lits("huf", _alpha(3000, 25)), [(10, 20, 5 + 3)])], single=True, checksum=True),
          Frame([Comp(Lits("raw", _noise(2000, 26)), [(100, 700, 50 + 3)])], single=True, fcs_bytes=4)]
    for m in range(1, 8):
        fr.append(Frame([Raw(_noise(1024 + 128 * m, 30 + m)), Comp(Lits("raw", b"!"), [(1, 100, 1000 + 3)])], window_log=10, mantissa=m))
    return fr


def _blocks_between():
    d = _alpha(2000, 27)
    return Frame([Comp(Lits("huf", d), [(10, 100, 7 + 3)]), RLE(0x55, BLOCK_MAX), Comp(Lits("treeless", d[:500]), [(3, 200, 1)]),
                  Raw(_noise(BLOCK_MAX, 28)), Comp(Lits("raw", b"hello"), [(5, 1000, BLOCK_MAX + 3)]), RLE(0, 5)],
                 window_log=18, checksum=True, fcs=True)


def _match_to_frame_start():
    return [Frame([Comp(Lits("raw", b"0123456789"), [(10, 25, 10 + 3)])], fcs=True),
            Frame([Raw(b"abc"), Comp(Lits("raw", b"de"), [(0, 5, 3 + 3), (2, 9, 10 + 3)])], window_log=10)]


def _ml_block_max():
    return Frame([Raw(b"xyz"), Comp(Lits("raw", b"Q"), [(1, BLOCK_MAX - 1, 1 + 3)], (PRE, PRE, rle(52)))], window_log=17, fcs=True)


def catalogue():
    """name -> spec (a Frame or a list of Frames): the valid frames"""
    cat = {
        "lits_raw_rle_headers": _lits_headers(),
        "lits_huf_size_formats": _huf_sizes(),
        "lits_huf_4streams_tiny": _huf_4streams_tiny(),
        "huf_weights_direct": _huf_weights_direct(),
        "huf_weights_fse": _huf_weights_fse(),
        "treeless_chain": _treeless_chain(),
        "nseq_edges": _nseq_edges(),
        "fse_accuracy_edges": _fse_edges(),
        "rle_codes_small": _rle_codes_small(),
        "rle_codes_16m": _rle_codes_16m(),
        "rep_offsets": _rep_offsets(),
        "repeat_tables_far": _repeat_tables_far(),
        "chunk_crossing": _chunk_crossing(),
        "headers": _headers(),
        "blocks_between": _blocks_between(),
        "match_to_frame_start": _match_to_frame_start(),
        "ml_block_max": _ml_block_max(),
    }
    return cat


def big_window_frame(window_log, codes, fastq=True, mantissa=0):
    """a frame with a 1 << window_log window filled cheaply: 128 KiB blocks of one fresh 256-byte FASTQ record (literals) and
    a 130 816-byte match (ML code 52) 64 KiB back (a repeat offset from the second block on) — whole records, none of them
    at a period of the content — then matches whose offsets are the powers of two `codes` name (OF codes 24 .. 27)."""
    P, R = 1 << 16, 256
    rec = lambda k: (b"@r%09d\n" % k) + _alpha(120, k) + b"\n+\n" + bytes(33 + (k + i) % 40 for i in range(120)) + b"\n"
    assert len(rec(0)) == R
    first = b"".join(rec(k) for k in range(P // R))
    blocks = [Comp(Lits("huf", first))]
    produced, k = P, P // R
    need = (1 << max(codes)) if codes else 0
    n = 0
    while produced < need:
        blocks.append(Comp(Lits("raw", rec(k)), [(R, BLOCK_MAX - R, P + 3 if n == 0 else 1)], (PRE, PRE, rle(52))))
        produced += BLOCK_MAX
        k += 1
        n += 1
    for c in codes:
        # a fresh record, then a match that copies 64 KiB of whole records from exactly 1 << c bytes back (1 << c is a
        # multiple of the 256-byte record: the copy stays record-aligned)
        blocks.append(Comp(Lits("raw", rec(k)), [(R, P, (1 << c) + 3)], (PRE, rle(c), PRE)))
        k += 1
    return Frame(blocks, window_log=window_log, mantissa=mantissa)


# ---------------------------------------------------------------------------------------------------------------- invalid
def invalid():
    """name -> (spec, clause of RFC 8878 it breaks, libzstd refuses it).  Every one must be refused by a decoder."""
    w = huf_weights(b"ACGT" * 10)
    return {
        "bad_reserved_block_type": (Frame([Comp(Lits("raw", b"abc")), Raw(b"x")], reserved_type=1),
                                    "3.1.1.2.2: Block_Type 3 is reserved", True),
        "bad_treeless_first": (Frame([Comp(Lits("treeless", b"ACGT" * 10, weights=w))]),
                               "3.1.1.3.1.1: treeless literals reuse the previous Huffman tree; a frame begins with none", True),
        "bad_repeat_table_first": (Frame([Comp(Lits("raw", b"abcd"), [(4, 4, 1 + 3)], (REP, PRE, PRE))]),
                                   "3.1.1.3.2.1: Repeat_Mode in the frame's first block: no table to repeat", True),
        "bad_fcs_mismatch": (Frame([Raw(b"x" * 100)], fcs=101),
                             "3.1.1.1.4: Frame_Content_Size is the decompressed size", True),
        "bad_offset_past_start": (Frame([Comp(Lits("raw", b"0123456789"), [(10, 5, 11 + 3)])]),
                                  "3.1.1.5: a match may not reach in front of the frame's first byte", True),
        "bad_ml_past_block": (Frame([Raw(b"xyz"), Comp(Lits("raw", b"QR"), [(2, BLOCK_MAX - 1, 1 + 3)], (PRE, PRE, rle(52)))], window_log=17),
                              "3.1.1.2.4: a block regenerates at most Block_Maximum_Size (128 KiB)", True),
        "bad_block_over_window": (Frame([Raw(b"w" * 1024), Raw(b"x" * 1025)], window_log=10),
                                  "3.1.1.2.3: Block_Size may not exceed Block_Maximum_Size = min(Window_Size, 128 KiB)", True),
        # libzstd 1.4.8 turns an offset of 0 into 1 (later versions refuse it): the device is held to the refusal alone
        "bad_rep3_zero": (Frame([Raw(b"abcdef"), Comp(Lits("raw", b""), [(0, 5, 3)])]),
                          "3.1.1.5: Offset_Value 3 with Literals_Length 0 is Repeated_Offset1 - 1: 0 here", False),
    }


# ---------------------------------------------------------------------------------------------------------------- generator
def _fastq_records(r, n0, count, L):
    """fixed-size FASTQ records (so that distances between record starts are multiples of the size)"""
    out = []
    for k in range(n0, n0 + count):
        if r.random() < 0.05:
            seq, qual = b"A" * L, b"I" * L
        else:
            seq = bytes(r.choice(b"ACGT") for _ in range(L))
            qual = bytes(r.randint(33, 73) for _ in range(L))
        out.append(b"@G%09d\n" % k + seq + b"\n+\n" + qual + b"\n")
    return out


def _pieces_random(r, size, window):
    """('lit', bytes) / ('match', offset, length) / ('run', byte, n) pieces whose content is about `size` bytes"""
    alpha = bytes(r.sample(range(256), r.choice((2, 4, 5, 20, 60, 256))))
    recent = []
    produced = 0
    while produced < size:
        x = r.random()
        if x < 0.35 or produced < 16:
            n = r.choice((r.randint(1, 20), r.randint(1, 300), r.randint(300, 5000))) if r.random() < 0.95 else r.randint(20000, 70000)
            yield ("lit", bytes(r.choice(alpha) for _ in range(n)))
            produced += n
        elif x < 0.97:
            lim = min(produced, window)
            y = r.random()
            if recent and y < 0.55:
                off = r.choice(recent[-3:])
            elif recent and y < 0.65:
                off = recent[-1] - 1
            else:
                off = r.randint(1, lim) if r.random() < 0.5 else r.randint(1, min(lim, 64))
            if not (1 <= off <= lim):
                off = r.randint(1, lim)
            ml = r.choice((r.randint(3, 12), r.randint(3, 60), r.randint(60, 2000))) if r.random() < 0.97 else r.randint(2000, 140000)
            yield ("match", off, ml)
            recent.append(off)
            produced += ml
        else:
            n = r.randint(4, 200000)
            yield ("run", r.randrange(256), n)
            produced += n


def _pieces_fastq(r, size, window, L):
    R = 12 + 2 * L + 4
    recs_src = []       # start of each record's body (seq line) in the content
    dists = []
    produced, k = 0, 0
    while produced < size:
        x = r.random()
        if x < 0.35 or len(recs_src) < 8:
            for rec in _fastq_records(r, k, r.randint(1, 6), L):
                hdr = rec[:12]
                if rec[12:12 + L] == b"A" * L and r.random() < 0.5:
                    yield ("lit", hdr)
                    yield ("run", 0x41, L)
                    yield ("lit", b"\n+\n")
                    yield ("run", 0x49, L)
                    yield ("lit", b"\n")
                else:
                    yield ("lit", rec)
                recs_src.append(produced + 12)
                produced += R
                k += 1
        else:
            # a run of records with fresh headers whose bodies are copied from as many consecutive earlier records (a repeat
            # offset per record); sometimes the quality line from another record (ll == 0)
            span = [s for s in recs_src if produced + 12 - s <= window]
            if not span:
                continue
            if dists and r.random() < 0.5:
                d = r.choice(dists[-3:])
                if d > produced + 12 - recs_src[0] or d > window:
                    d = produced + 12 - r.choice(span)
            else:
                d = produced + 12 - r.choice(span)
            dists.append(d)
            for _ in range(r.randint(1, 20)):
                yield ("lit", b"@G%09d\n" % k)
                if r.random() < 0.3 and len(dists) > 1:
                    d2 = dists[-2]
                    yield ("match", d, L + 3)
                    if d2 <= produced + 12 + L + 3 - recs_src[0] and d2 <= window:
                        yield ("match", d2, L + 1)
                    else:
                        yield ("match", d, L + 1)
                else:
                    yield ("match", d, 2 * L + 4)
                recs_src.append(produced + 12)
                produced += R
                k += 1


def random_frame(seed, size=200_000, fastq=False):
    """a random spec of about `size` bytes of content: random tables, literal forms and block kinds, repeat codes wherever the
    history allows them (ll == 0 often); `fastq`: the content is FASTQ text (fixed-size records, bodies copied)"""
    r = random.Random(seed)
    single = size < (1 << 20) and r.random() < 0.15
    wlog = r.choice((17, 18, 20, 22)) if not single else 0
    window = (1 << wlog) if not single else 1 << 40
    L = r.choice((50, 100, 150))
    pieces = _pieces_fastq(r, size, window, L) if fastq else _pieces_random(r, size, window)
    out = bytearray()
    blocks = []
    st = {"hist": (1, 4, 8), "tree": None, "tbl": [None, None, None]}
    cur = {"lits": bytearray(), "seqs": [], "ll": 0, "out": 0}
    target = [r.choice((r.randint(100, 5000), r.randint(5000, BLOCK_MAX)))]

    def flush():
        if cur["out"] == 0 and not cur["seqs"]:
            return
        begin = len(out) - cur["out"]
        _emit_comp(r, blocks, st, bytes(cur["lits"]), cur["seqs"], bytes(out[begin:]))
        cur.update(lits=bytearray(), seqs=[], ll=0, out=0)
        target[0] = r.choice((r.randint(100, 5000), r.randint(5000, BLOCK_MAX), BLOCK_MAX))

    def room():
        return min(BLOCK_MAX, target[0]) - cur["out"]

    def add_lits(b):
        while b:
            if room() <= 0:
                flush()
            k = min(len(b), room())
            cur["lits"] += b[:k]
            cur["ll"] += k
            cur["out"] += k
            out.extend(b[:k])
            b = b[k:]

    for pc in pieces:
        if pc[0] == "lit":
            if r.random() < 0.04:
                flush()
                for i in range(0, len(pc[1]), BLOCK_MAX):
                    blocks.append(Raw(pc[1][i:i + BLOCK_MAX]))
                out += pc[1]
            else:
                add_lits(pc[1])
        elif pc[0] == "run":
            _, b, n = pc
            if r.random() < 0.6:
                flush()
                while n:
                    k = min(n, BLOCK_MAX, window)
                    blocks.append(RLE(b, k))
                    out += bytes([b]) * k
                    n -= k
            elif n >= 4:
                add_lits(bytes([b]))
                _add_match(cur, out, 1, n - 1, room, flush, add_lits)
            else:
                add_lits(bytes([b]) * n)
        else:
            _add_match(cur, out, pc[1], pc[2], room, flush, add_lits)
    flush()
    if not blocks:
        blocks.append(Raw(b""))
    F = Frame(blocks, window_log=wlog or 17, single=single, checksum=r.random() < 0.5, fcs=True if r.random() < 0.5 else None,
              mantissa=0)
    F._content = bytes(out)
    return F


def _add_match(cur, out, off, ml, room, flush, add_lits):
    while ml > 0:
        if room() < 3:
            flush()
        k = min(ml, room())
        if ml - k and ml - k < 3:
            k = ml - 3 if ml - 3 >= 3 else k
        if k < 3:   # (a remainder too short for a match: literals, taken from the content itself)
            src = len(out) - off
            add_lits(bytes(out[src:src + k]) if off >= k else bytes(out[src + (i % off)] for i in range(k)))
            ml -= k
            continue
        cur["seqs"].append((cur["ll"], k, off))
        cur["ll"] = 0
        cur["out"] += k
        _copy(out, off, k)
        ml -= k


def _emit_comp(r, blocks, st, lits, seqs, content):
    """one compressed block (Offset_Values, literal form and tables drawn here), or raw blocks when it would not fit"""
    hist = st["hist"]
    coded = []
    for ll, ml, off in seqs:
        r0, r1, r2 = hist
        cand = [(1, r0), (2, r1), (3, r2)] if ll else [(1, r1), (2, r2), (3, r0 - 1)]
        reps = [v for v, o in cand if o == off]
        ofv = reps[0] if reps and r.random() < 0.9 else off + 3
        o2, hist = apply_ofv(hist, ll, ofv)
        assert o2 == off
        coded.append((ll, ml, ofv))
    # literals
    tree = st["tree"]
    x = r.random()
    n = len(lits)
    if n and len(set(lits)) == 1 and x < 0.6:
        L = Lits("rle", lits, r.choice((None, 1, 3)) if n < 4096 else None)
    elif n >= 10 and tree is not None and all(b < len(tree) and tree[b] for b in set(lits)) and x < 0.45:
        L = Lits("treeless", lits, None, 1 if n < 1024 and r.random() < 0.5 else 4)
    elif n >= 10 and x < 0.85:
        L = Lits("huf", lits, None, 1 if n < 1024 and r.random() < 0.5 else 4, weight_form=r.choice(("auto", "auto", "direct")))
        if L.weight_form == "direct" and max(lits) > 128:
            L.weight_form = "auto"
    else:
        L = Lits("raw", lits, None if n >= 32 or r.random() < 0.5 else 1)
    # tables
    tabs = []
    for k, codes in enumerate(([ll_code(s[0])[0] for s in coded], [of_code(s[2])[0] for s in coded], [ml_code(s[1])[0] for s in coded])):
        if not codes:
            break
        h = Counter(codes)
        prev = st["tbl"][k]
        opts = ["fse", "fse"]
        if len(h) == 1:
            opts += ["rle", "rle"]
        if k != 1 or max(h) <= 28:
            opts.append("pre")
        if prev is not None and all(prev[1].has(c) for c in h):
            opts += ["rep", "rep", "rep"]
        m = r.choice(opts)
        if m == "fse":
            need = max(5, (len(h) + 2).bit_length())
            lg = r.randint(min(need, MAX_LOG[k]), MAX_LOG[k])
            if len(h) + 2 > (1 << lg):
                m = "pre" if (k != 1 or max(h) <= 28) else "rle"
            else:
                extra = {c: 0 for c in r.sample(range(MAX_CODE[k] + 1), 2) if c not in h}
                tabs.append(fse(normalize({**h, **extra}, lg, r, 0.5), lg))
                continue
        tabs.append({"rle": lambda: rle(codes[0]), "pre": lambda: PRE, "rep": lambda: REP}[m]() if m != "rle" or len(h) == 1 else PRE)
    B = Comp(L, coded, tuple(tabs) if coded else (PRE, PRE, PRE))
    trial = {"tree": tree, "tbl": [t[1] if t else None for t in st["tbl"]]}
    try:
        body = lits_section(B.lits, trial) + seqs_section(B, trial)
    except AssertionError:
        body = None
    if body is None or len(body) >= BLOCK_MAX:
        for i in range(0, len(content), BLOCK_MAX):
            blocks.append(Raw(content[i:i + BLOCK_MAX]))
        return
    blocks.append(B)
    st["hist"] = hist
    st["tree"] = trial["tree"]
    for k in range(3):
        if coded and B.tables[k].mode != "rep":
            st["tbl"][k] = (B.tables[k].mode, trial["tbl"][k])
