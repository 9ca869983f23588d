"""A small bzip2 encoder for tests: streams that libbz2 accepts but its encoder never writes (a code of length 20, six
tables that switch every group, origPtr at either end, one byte value in use, block magic spelled by Huffman bits).

Blocks are built from their BWT column L and origPtr (any L whose LF mapping the decoder walks), their symbol stream
(MTF / RLE2) and Huffman code lengths chosen by the caller; the block CRC is taken from the block's output as libbz2
computes it (nblock steps along the LF mapping from origPtr, then RLE1 undone)."""


def _crc_table():
    t = []
    for i in range(256):
        c = i << 24
        for _ in range(8):
            c = ((c << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if c & 0x80000000 else (c << 1) & 0xFFFFFFFF
        t.append(c)
    return t


_T = _crc_table()


def crc(data):
    c = 0xFFFFFFFF
    for b in data:
        c = ((c << 8) & 0xFFFFFFFF) ^ _T[(c >> 24) ^ b]
    return c ^ 0xFFFFFFFF


def rle1(data):
    out, i = bytearray(), 0
    while i < len(data):
        j = i
        while j < len(data) and data[j] == data[i] and j - i < 259:
            j += 1
        run = j - i
        out += bytes([data[i]]) * min(run, 4) + (bytes([run - 4]) if run >= 4 else b"")
        i = j
    return bytes(out)


def bwt(s):
    n = len(s)
    rots = sorted(range(n), key=lambda i: s[i:] + s[:i])
    return bytes(s[(i - 1) % n] for i in rots), rots.index(0)


def inverse(L, orig):
    """libbz2's output for a BWT column: nblock steps from origPtr, then RLE1 undone"""
    n = len(L)
    cnt = [0] * 256
    for b in L:
        cnt[b] += 1
    cf, s = [], 0
    for c in range(256):
        cf.append(s)
        s += cnt[c]
    nxt = [0] * n
    for i, b in enumerate(L):
        nxt[cf[b]] = i
        cf[b] += 1
    p, pre = nxt[orig], bytearray()
    for _ in range(n):
        pre.append(L[p])
        p = nxt[p]
    out, i = bytearray(), 0
    while i < len(pre):
        j = i
        while j < len(pre) and j - i < 4 and pre[j] == pre[i]:
            j += 1
        out += pre[i:j]
        if j - i == 4:
            out += bytes([pre[i]]) * pre[j]
            j += 1
        i = j
    return bytes(out)


def mtf_rle2(L, used):
    seq = {b: i for i, b in enumerate(used)}
    mtf, syms, run = list(range(len(used))), [], 0

    def flush():
        nonlocal run
        while run > 0:
            if run & 1:
                syms.append(0)
                run = (run - 1) >> 1
            else:
                syms.append(1)
                run = (run - 2) >> 1

    for b in L:
        k = mtf.index(seq[b])
        if k == 0:
            run += 1
            continue
        flush()
        mtf.insert(0, mtf.pop(k))
        syms.append(k + 1)
    flush()
    syms.append(len(used) + 1)
    return syms


def inverse_mtf(idx, used):
    mtf, L = list(range(len(used))), bytearray()
    for k in idx:
        v = mtf.pop(k)
        mtf.insert(0, v)
        L.append(used[v])
    return bytes(L)


def one_cycle(L, orig):
    n = len(L)
    cnt = [0] * 256
    for b in L:
        cnt[b] += 1
    cf, s = [], 0
    for c in range(256):
        cf.append(s)
        s += cnt[c]
    nxt = [0] * n
    for i, b in enumerate(L):
        nxt[cf[b]] = i
        cf[b] += 1
    p, k = nxt[orig], 1
    while p != orig:
        p = nxt[p]
        k += 1
    return k == n


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, k, x):
        self.v = (self.v << k) | (x & ((1 << k) - 1))
        self.n += k

    def bytes(self):
        pad = -self.n % 8
        return (self.v << pad).to_bytes((self.n + pad) // 8, "big")


def uniform_lengths(alpha):
    k = max(1, (alpha - 1).bit_length())
    return [k] * alpha


def codes(lengths):
    code, vec = [0] * len(lengths), 0
    for n in range(min(lengths), max(lengths) + 1):
        for i, ln in enumerate(lengths):
            if ln == n:
                code[i] = vec
                vec += 1
        vec <<= 1
    return code


def put_block(w, L, orig, syms=None, used=None, tables=None, selectors=None, randomised=0, block_crc=None):
    used = used if used is not None else sorted(set(L))
    syms = syms if syms is not None else mtf_rle2(L, used)
    alpha = len(used) + 2
    tables = tables or [uniform_lengths(alpha)] * 2
    ng = len(tables)
    nsel = (len(syms) + 49) // 50
    selectors = selectors or [0] * nsel
    w.put(48, 0x314159265359)
    w.put(32, crc(inverse(L, orig)) if block_crc is None else block_crc)
    w.put(1, randomised)
    w.put(24, orig)
    in16 = [any(b // 16 == i for b in used) for i in range(16)]
    for i in range(16):
        w.put(1, in16[i])
    for i in range(16):
        if in16[i]:
            for j in range(16):
                w.put(1, (i * 16 + j) in used)
    w.put(3, ng)
    w.put(15, len(selectors))
    pos = list(range(ng))
    for s in selectors:
        k = pos.index(s)
        pos.insert(0, pos.pop(k))
        for _ in range(k):
            w.put(1, 1)
        w.put(1, 0)
    for t in tables:
        cur = t[0]
        w.put(5, cur)
        for ln in t:
            while cur != ln:
                w.put(2, 0b10 if ln > cur else 0b11)
                cur += 1 if ln > cur else -1
            w.put(1, 0)
    cs = [codes(t) for t in tables]
    for i, s in enumerate(syms):
        t = selectors[i // 50]
        w.put(tables[t][s], cs[t][s])
    return inverse(L, orig)


def stream(blocks, level=9, stream_crc=None):
    """blocks: dicts of put_block arguments -> (stream bytes, decoded bytes)"""
    w = Bits()
    w.put(32, int.from_bytes(b"BZh" + bytes([0x30 + level]), "big"))
    comb, out = 0, b""
    for b in blocks:
        o = put_block(w, **b)
        c = b.get("block_crc", crc(o))
        comb = (((comb << 1) | (comb >> 31)) & 0xFFFFFFFF) ^ c
        out += o
    w.put(48, 0x177245385090)
    w.put(32, comb if stream_crc is None else stream_crc)
    return w.bytes(), out


def data_block(data):
    L, orig = bwt(rle1(data))
    return {"L": L, "orig": orig}
