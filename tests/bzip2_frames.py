"""A small bzip2 encoder for tests: streams that libbz2 accepts but its encoder never writes (a code of length 20, six
tables that switch every group, origPtr at either end, one byte value in use, block magic spelled by Huffman bits), a
catalogue of them (catalogue), of streams libbz2 refuses (invalid) and a seeded generator (generate).

Blocks are built from their BWT column L and origPtr (any L whose LF mapping the decoder walks), their symbol stream
(MTF / RLE2) and Huffman code lengths chosen by the caller; the block CRC is taken from the block's output as libbz2
computes it (nblock steps along the LF mapping from origPtr, then RLE1 undone).  put_block also writes blocks that have
no output: every field can be given as it should stand in the file.

One form asked of the catalogue cannot be written: "a code index past the alphabet".  In BZ2_hbCreateDecodeTables
limit[n] is the last code of length n and base[n] the first one minus the number of shorter codes, and the decode loop
leaves at the first n with zvec <= limit[n], where zvec is already >= the first code of that length (it was > limit[n - 1],
then doubled): zvec - base[n] lies between the count of shorter codes and the index of the last code of length n, inside
perm[0 .. alphaSize) whatever the lengths are, over-subscribed ones included.  libbz2's range check on that index and the
decoder's 0xFFFF entries of perm are both unreachable."""
import functools
import random
import zlib

MAGIC_BLOCK, MAGIC_END = 0x314159265359, 0x177245385090
NBLOCKS = (1, 2, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193, 12288, 20480)
PIECE = 4096  # the RLE1 piece of exg_bzip2.hip


def _crc_table():
    t = []
    for i in range(256):
        c = i << 24
        for _ in range(8):
            c = ((c << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if c & 0x80000000 else (c << 1) & 0xFFFFFFFF
        t.append(c)
    return t


_T = _crc_table()
_REV = bytes(int(format(i, "08b")[::-1], 2) for i in range(256))


def crc_bytewise(data):
    c = 0xFFFFFFFF
    for b in data:
        c = ((c << 8) & 0xFFFFFFFF) ^ _T[(c >> 24) ^ b]
    return c ^ 0xFFFFFFFF


def crc(data):
    """bzip2's CRC (MSB first) is zlib's (LSB first) over bit-reversed bytes, bit-reversed"""
    return int(format(zlib.crc32(bytes(data).translate(_REV)), "032b")[::-1], 2)


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
    s2 = bytes(s) * 2
    rots = sorted(range(n), key=lambda i: s2[i:i + n])
    return bytes(s[(i - 1) % n] for i in rots), rots.index(0)


def lf_next(L):
    """nxt[k] = the row of L that holds the k-th byte of the sorted column (stable)"""
    return sorted(range(len(L)), key=L.__getitem__)


def lf_walk(L, orig):
    """the text in front of RLE1 as libbz2 reads it from a BWT column: nblock steps from origPtr"""
    nxt = lf_next(L)
    p, pre = nxt[orig], bytearray()
    for _ in range(len(L)):
        pre.append(L[p])
        p = nxt[p]
    return bytes(pre)


def cycle_length(L, orig):
    nxt = lf_next(L)
    p, k = nxt[orig], 1
    while p != orig:
        p = nxt[p]
        k += 1
    return k


def unrle1(pre):
    """RLE1 undone; None when the text ends where a count byte is due (libbz2: a data error)"""
    out, i, n = bytearray(), 0, len(pre)
    while i < n:
        b, j = pre[i], i + 1
        while j < n and j - i < 4 and pre[j] == b:
            j += 1
        out += pre[i:j]
        if j - i == 4:
            if j == n:
                return None
            out += bytes([b]) * pre[j]
            j += 1
        i = j
    return bytes(out)


@functools.lru_cache(maxsize=32)
def inverse(L, orig):
    """libbz2's output for a BWT column: nblock steps from origPtr, then RLE1 undone (None: no valid output)"""
    return unrle1(lf_walk(L, orig))


def piece_states(pre, piece=PIECE):
    """the RLE1 state in which every piece of the text is entered: 0 free, 1..3 equal bytes so far, 4 a count byte is due"""
    r, prev, st = 0, None, []
    for i, x in enumerate(pre):
        if i % piece == 0:
            st.append(r)
        if r == 4:
            r = 0
        elif r and x == prev:
            r += 1
        else:
            r = 1
        prev = x
    return st


def run_syms(run):
    """RUNA / RUNB symbols of a run (bijective base 2, least significant first)"""
    syms = []
    while run > 0:
        if run & 1:
            syms.append(0)
            run = (run - 1) >> 1
        else:
            syms.append(1)
            run = (run - 2) >> 1
    return syms


def mtf_rle2(L, used):
    seq = {b: i for i, b in enumerate(used)}
    mtf, syms, run = list(range(len(used))), [], 0
    for b in L:
        k = mtf.index(seq[b])
        if k == 0:
            run += 1
            continue
        syms += run_syms(run)
        run = 0
        mtf.insert(0, mtf.pop(k))
        syms.append(k + 1)
    syms += run_syms(run)
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
    return cycle_length(L, orig) == len(L)


class Bits:
    """MSB-first bit writer: whole bytes go to a bytearray, at most 71 bits wait in an integer"""

    def __init__(self):
        self.buf, self.acc, self.k, self.n = bytearray(), 0, 0, 0

    def put(self, k, x):
        self.acc = (self.acc << k) | (x & ((1 << k) - 1))
        self.k += k
        self.n += k
        if self.k >= 64:
            r = self.k & 7
            self.buf += (self.acc >> r).to_bytes(self.k >> 3, "big")
            self.acc &= (1 << r) - 1
            self.k = r

    def put_bits(self, s):
        if s:
            self.put(len(s), int(s, 2))

    def bytes(self):
        pad = -self.k % 8
        return bytes(self.buf) + (self.acc << pad).to_bytes((self.k + pad) // 8, "big")


def uniform_lengths(alpha):
    k = max(1, (alpha - 1).bit_length())
    return [k] * alpha


def kraft_lengths(r, alpha, maxlen=20, deep=0.3):
    """random code lengths <= maxlen whose Kraft sum is exactly 1"""
    leaves = [0]
    while len(leaves) < alpha:
        can = [i for i, d in enumerate(leaves) if d < maxlen]
        i = max(can, key=leaves.__getitem__) if r.random() < deep else r.choice(can)
        d = leaves.pop(i)
        leaves += [d + 1, d + 1]
    r.shuffle(leaves)
    return leaves


def codes(lengths):
    code, vec = [0] * len(lengths), 0
    for n in range(min(lengths), max(lengths) + 1):
        for i, ln in enumerate(lengths):
            if ln == n:
                code[i] = vec
                vec += 1
        vec <<= 1
    return code


def delta_bits(lengths):
    """the delta code of a table's lengths as a string of bits"""
    cur = lengths[0]
    s = [format(cur, "05b")]
    for ln in lengths:
        while cur != ln:
            s.append("10" if ln > cur else "11")
            cur += 1 if ln > cur else -1
        s.append("0")
    return "".join(s)


def spelled_table(magic, alpha):
    """the delta-code bits of a table of alpha legal lengths that hold the 48 bits of `magic` behind the start value"""
    s = "01010" + format(magic, "048b")
    cur, nsym, i = 10, 0, 5
    while i < len(s):
        if s[i] == "0":
            nsym, i = nsym + 1, i + 1
            continue
        if i + 1 == len(s):
            s += "0"
        cur += 1 if s[i + 1] == "0" else -1
        assert 1 <= cur <= 20
        i += 2
    assert nsym <= alpha, (nsym, alpha)
    return s + "0" * (alpha - nsym)


def put_block(w, L=None, orig=0, syms=None, used=None, tables=None, selectors=None, randomised=0, block_crc=None, n_selectors=None,
              written=None, selector_bits=None, symmap=None, table_bits=None, n_groups=None, orig_field=None, magic=MAGIC_BLOCK):
    """One block into w; -> its output (None when it has none).
    L, orig: the BWT column (None: syms, used and block_crc say what is written); syms: symbols, or (bits, value) for raw
    bits; tables: code lengths that code the symbols; table_bits[t]: the bits sent for table t instead of its delta code;
    selectors: the table of every group of 50 (coding); written: how many of them are sent; n_selectors: the field;
    selector_bits: the bits sent for the selectors instead; symmap: (the 16 bits, [the 16-bit words sent]);
    n_groups, orig_field, magic: those fields as sent"""
    used = used if used is not None else sorted(set(L))
    syms = syms if syms is not None else mtf_rle2(L, used)
    alpha = len(used) + 2
    tables = tables or [uniform_lengths(alpha)] * 2
    ng = len(tables)
    selectors = list(selectors) if selectors is not None else [0] * ((len(syms) + 49) // 50)
    sent = selectors if written is None else selectors[:written]
    out = inverse(L, orig) if L is not None else None
    if block_crc is None:
        block_crc = crc(out) if out is not None else 0
    w.put(48, magic)
    w.put(32, block_crc)
    w.put(1, randomised)
    w.put(24, orig if orig_field is None else orig_field)
    if symmap is None:
        words = [sum(((i * 16 + j) in used) << (15 - j) for j in range(16)) for i in range(16)]
        symmap = (sum((words[i] != 0) << (15 - i) for i in range(16)), [x for x in words if x])
    w.put(16, symmap[0])
    for x in symmap[1]:
        w.put(16, x)
    w.put(3, ng if n_groups is None else n_groups)
    w.put(15, len(sent) if n_selectors is None else n_selectors)
    if selector_bits is not None:
        w.put_bits(selector_bits)
    else:
        pos = list(range(ng))
        for s in sent:
            k = pos.index(s)
            pos.insert(0, pos.pop(k))
            w.put(k + 1, (1 << (k + 1)) - 2)
    for t, lens in enumerate(tables):
        w.put_bits(table_bits[t] if table_bits and table_bits[t] is not None else delta_bits(lens))
    cs = [codes(t) for t in tables]
    for i, s in enumerate(syms):
        if isinstance(s, tuple):
            w.put(*s)
        else:
            t = selectors[i // 50]
            w.put(tables[t][s], cs[t][s])
    return out


def stream(blocks, level=9, stream_crc=None, info=None, header=None):
    """blocks: dicts of put_block arguments -> (stream bytes, decoded bytes); info (a dict) receives the bit offsets of the
    blocks, of the end-of-stream magic and the stream's length in bits before padding"""
    w = Bits()
    w.put_bits("".join(format(c, "08b") for c in (header if header is not None else b"BZh" + bytes([0x30 + level]))))
    comb, out, at = 0, b"", []
    for b in blocks:
        at.append(w.n)
        o = put_block(w, **b)
        c = b.get("block_crc")
        if c is None:
            c = crc(o) if o is not None else 0
        comb = (((comb << 1) | (comb >> 31)) & 0xFFFFFFFF) ^ c
        out += o or b""
    if info is not None:
        info.update(blocks=at, end=w.n, bits=w.n + 80)
    w.put(48, MAGIC_END)
    w.put(32, comb if stream_crc is None else stream_crc)
    return w.bytes(), out


def data_block(data):
    L, orig = bwt(rle1(data))
    return {"L": L, "orig": orig}


def block_from_pre(pre):
    """the block whose text in front of RLE1 is exactly `pre` (keep it under ~5000 bytes: bwt sorts rotations)"""
    L, orig = bwt(pre)
    assert lf_walk(L, orig) == bytes(pre)
    return {"L": L, "orig": orig}


# ---------------------------------------------------------------- columns
def random_column(r, n, values, runs=False):
    if not runs:
        return bytes(r.choices(values, k=n))
    out = bytearray()
    while len(out) < n:
        out += bytes([r.choice(values)]) * min(n - len(out), r.choice((1, 1, 1, 2, 3, 4, 5, 8, 30, 300)))
    return bytes(out)


def valid_column(seed, n, values, orig, runs=False):
    """a seeded random column that has an output at this origPtr"""
    for salt in range(200):
        L = random_column(random.Random("%s/%d" % (seed, salt)), n, values, runs)
        if inverse(L, orig) is not None:
            return L
    raise AssertionError(seed)


def valid_orig(L, start=0):
    for orig in list(range(start, len(L))) + list(range(start)):
        if inverse(L, orig) is not None:
            return orig
    raise AssertionError("no origPtr gives this column an output")


def values_of(seed, k):
    return [5, 250] if k == 2 else sorted(random.Random("values/%s" % seed).sample(range(256), k))


def filler(r, n, avoid):
    """n bytes without two equal neighbours and without the bytes of `avoid`"""
    pool = [b for b in range(32, 127) if b not in avoid]
    out = bytearray()
    while len(out) < n:
        b = r.choice(pool)
        if not out or out[-1] != b:
            out.append(b)
    return bytes(out)


def period5_columns():
    """name -> (L, origPtr): one byte value whose count byte equals it; the text in front of RLE1 has period 5"""
    return {"period5_byte%02x_n%d" % (b, n): (bytes([b]) * n, n // 3) for b in (0x41, 0x00, 0xFF) for n in (20480, 20481, 20482, 20483)}


def short_cycle_column(seed, n, values):
    """a column and an origPtr whose cycle is short and does not divide n"""
    for salt in range(200):
        L = random_column(random.Random("cycle/%s/%d" % (seed, salt)), n, values)
        nxt, seen = lf_next(L), [False] * n
        for s in range(n):
            if seen[s]:
                continue
            k, p = 0, s
            while not seen[p]:
                seen[p] = True
                p = nxt[p]
                k += 1
            if 3 < k < n // 3 and n % k and inverse(L, s) is not None:
                return L, s, k
    raise AssertionError(seed)


def lengths_9_to_12(r):
    """alpha 258, Kraft sum exactly 1: 29 codes of 7 bits, 191 of 8, 6 of 9, 8 of 10, 8 of 11, 16 of 12"""
    lens = [7] * 29 + [8] * 191 + [9] * 6 + [10] * 8 + [11] * 8 + [12] * 16
    assert len(lens) == 258 and sum(1 << (12 - x) for x in lens) == 1 << 12
    r.shuffle(lens)
    return lens


def ramp_lengths(alpha):
    ramp = list(range(1, 21)) + list(range(19, 0, -1))
    return [ramp[i % len(ramp)] for i in range(alpha)]


def spelled_block(r, magic, times, n=340):
    """a block of 256 byte values whose symbols 0..253 have 8-bit codes equal to themselves: its Huffman bits spell `magic`
    `times` times (the last time as its last six symbols in front of the end-of-block code)"""
    used, lens = list(range(256)), [8] * 254 + [9] * 4
    spell = [((magic >> s) & 0xFF) - 1 for s in (40, 32, 24, 16, 8, 0)]
    assert min(spell) >= 1
    for _ in range(200):
        idx = [r.randint(1, 200) for _ in range(n)]
        for k in range(times - 1):
            at = 7 + k * (n - 20) // times
            idx[at:at + 6] = spell
        idx[-6:] = spell
        L = inverse_mtf(idx, used)
        orig = r.randrange(n)
        if inverse(L, orig) is not None:
            return {"L": L, "orig": orig, "syms": [k + 1 for k in idx] + [257], "used": used, "tables": [lens, lens]}
    raise AssertionError("no such block")


def count_bits(data, magic):
    s = format(int.from_bytes(data, "big"), "0%db" % (8 * len(data)))
    pat, k, at = format(magic, "048b"), 0, -1
    while True:
        at = s.find(pat, at + 1)
        if at < 0:
            return k
        k += 1


# ---------------------------------------------------------------- the catalogue
TRAILING = "trailing_"  # entries whose stream ends in bytes that are no stream: nothing can follow them in one input


def with_tables(r, blk, ng, selectors="random", maxlen=20):
    used = blk.get("used") or sorted(set(blk["L"]))
    syms = blk.get("syms") or mtf_rle2(blk["L"], used)
    nsel = (len(syms) + 49) // 50
    sel = [r.randrange(ng) for _ in range(nsel)] if selectors == "random" else selectors(nsel)
    return dict(blk, used=used, syms=syms, tables=[kraft_lengths(r, len(used) + 2, maxlen) for _ in range(ng)], selectors=sel)


@functools.lru_cache(None)
def _build():
    cat, offsets = {}, {}

    def add(name, blocks, level=9, **kw):
        info = {}
        cat[name] = stream(blocks, level, info=info, **kw)
        offsets[name] = info["blocks"]
        return cat[name]

    def col(L, orig, **kw):
        return dict({"L": bytes(L), "orig": orig}, **kw)

    r = random.Random(20)
    tiny = lambda k: data_block(b"tiny block %d of the catalogue\n" % k)  # noqa: E731

    # ---- block geometry: every nblock with origPtr 0, 256, 512, the last multiple of 256, nblock - 1; 2 / 17 / 256 byte values
    for i, n in enumerate(NBLOCKS):
        origs = sorted({o for o in (0, 256, 512, (n - 1) // 256 * 256, n - 1) if o < n})
        while len(origs) < 3:
            origs.append(origs[-1])
        blocks = []
        for j, o in enumerate(origs):
            k = (2, 17, 256)[(i + j) % 3]
            blocks.append(col(valid_column("geom/%d/%d" % (n, j), n, values_of(n, k), o), o))
        add("geometry_nblock_%d" % n, blocks)

    # ---- period 5: the five pieces of 20480 bytes are entered in five different states
    for name, (L, o) in period5_columns().items():
        add(name, [tiny(len(cat)), col(L, o)])

    # ---- a run of four against the piece boundary: it starts at 4092 .. 4096, the count byte is 0, 1, 255 or the run's byte
    for count in (0, 1, 255, 0x41):
        blocks = []
        for start in range(PIECE - 4, PIECE + 1):
            rr = random.Random("boundary/%d/%d" % (count, start))
            pre = filler(rr, start, b"A") + b"AAAA" + bytes([count]) + filler(rr, 4200 - start - 5, b"A")
            assert piece_states(pre)[1] == max(1, PIECE - start) and pre[start + 4] == count
            blocks.append(block_from_pre(pre))
        add("run_at_piece_boundary_count_%d" % count, blocks)
    rr = random.Random("boundary/twice")
    for name, body in (("run_count0_run_count2", b"AAAA\x00AAAA\x02"), ("run_count_then_byte_equal_to_count", b"AAAA\x05\x05"),
                       ("run_count_then_byte_equal_to_run", b"AAAA\x03A")):
        add(name, [block_from_pre(b"xy" + body + b"z"), block_from_pre(filler(rr, PIECE - 6, b"A\x05\x03") + body + filler(rr, 90, b"A\x05\x03\x00\x02"))])

    # ---- origPtr's cycle is short and does not divide nblock (libbz2 repeats it; k_repeat)
    for n, k in ((1000, 4), (12289, 4)):
        L, o, cyc = short_cycle_column(n, n, values_of("cyc", k))
        assert n % cyc and cyc < n // 3
        add("cycle_%d_of_nblock_%d" % (cyc, n), [tiny(n), col(L, o)])

    # ---- tables
    abc = (b"abc" * 40)
    for ng in (2, 3, 4, 5, 6):
        small = col(abc[:39], valid_orig(abc[:39]))
        big = col(valid_column("groups/%d" % ng, 5000, list(range(256)), 777), 777)
        add("groups_%d_on_40_and_5000_symbols" % ng, [with_tables(r, small, ng), with_tables(r, big, ng)])
        assert len(mtf_rle2(small["L"], sorted(set(small["L"])))) == 40
    b17 = col(valid_column("b17", 600, values_of("b17", 17), 300), 300)
    a17 = 19
    assert len(set(b17["L"])) == 17
    add("unused_tables_with_odd_lengths", [dict(b17, tables=[uniform_lengths(a17), [1] * a17, [20] * a17, [1, 20] * 9 + [1], ramp_lengths(a17), [20, 19] * 9 + [1]])])
    b37 = col(valid_column("b37", 900, values_of("b37", 37), 5), 5)
    assert len(set(b37["L"])) == 37
    add("table_1_to_20_to_1", [dict(b37, tables=[ramp_lengths(39), uniform_lengths(39)], selectors=[1] * ((len(mtf_rle2(b37["L"], sorted(set(b37["L"])))) + 49) // 50))])
    b256 = col(valid_column("b256", 3000, list(range(256)), 1024), 1024, used=list(range(256)))
    s256 = mtf_rle2(b256["L"], list(range(256)))
    l912 = lengths_9_to_12(r)
    assert {9, 10, 11, 12} <= {l912[s] for s in s256}
    add("codes_of_9_10_11_12_bits_in_one_table", [dict(b256, tables=[l912, l912])])
    add("table_minlen_11", [dict(b17, tables=[[11] * a17] * 2), dict(b256, tables=[[11 + (i % 3) for i in range(258)]] * 2)])
    add("table_minlen_15", [dict(b17, tables=[[15] * a17] * 2)])
    add("table_all_lengths_20", [dict(b17, tables=[[20] * a17] * 2), dict(b256, tables=[[20] * 258] * 2)])
    b4 = col(valid_column("b4", 300, [65, 67, 71, 84], 0), 0)
    add("incomplete_codes", [dict(b4, tables=[[3] * 6, [3] * 6]), dict(b4, tables=[[20] * 6, [3] * 6]), dict(b4, tables=[[2, 3, 4, 5, 6, 7]] * 2)])
    # over-subscribed: 15 byte values in the column, 4 more in the symbol map that never occur: the symbols of MTF index
    # 15 .. 18 have 5-bit codes 32 .. 35, which no 5 bits spell; every symbol that occurs has a code that fits
    v15 = list(range(40, 55))
    bo = col(valid_column("over", 700, v15, 9), 9, used=v15 + [200, 201, 202, 203])
    over = [4] * 12 + [5] * 8 + [3]
    assert sum(2.0 ** -x for x in over) > 1 and max(mtf_rle2(bo["L"], bo["used"])[:-1]) <= 15
    add("oversubscribed_table_in_use", [dict(bo, tables=[over, over])])
    add("oversubscribed_table_unused", [dict(b17, tables=[uniform_lengths(a17), [1] * a17, [2] * a17])])

    # ---- selectors
    s17 = mtf_rle2(b17["L"], sorted(set(b17["L"])))
    need = (len(s17) + 49) // 50
    add("selectors_exactly_as_needed", [dict(b17, selectors=[k % 2 for k in range(need)])])
    add("selectors_one_surplus", [dict(b17, selectors=[k % 2 for k in range(need + 1)])])
    for k in (18002, 18003, 32767):
        tabs = [kraft_lengths(r, a17) for _ in range(3)]
        add("selectors_%d_written" % k, [tiny(k), dict(b17, tables=tabs, selectors=[r.randrange(3) for _ in range(k)])])
    for ng in (2, 6):
        big = col(valid_column("lastsel/%d" % ng, 5000, list(range(256)), 4864), 4864)
        add("selector_mtf_index_last_at_every_group_of_%d" % ng, [with_tables(r, big, ng, selectors=lambda nsel, ng=ng: [(ng - 1 - k) % ng for k in range(nsel)])])
    for k in (49, 50, 51, 100):
        L = (b"abc" * 40)[:k - 1]
        add("symbols_%d_with_end_of_block" % k, [tiny(k), with_tables(r, col(L, valid_orig(L, k // 2)), 3)])
        assert len(mtf_rle2(L, sorted(set(L)))) == k

    # ---- symbols
    L = b"\x07" * 20 + random_column(r, 200, [7, 8, 9])
    add("run_at_block_start", [col(L, valid_orig(L, 100))])
    runs = [1, 2, 3, 4] + [x for k in range(3, 17) for x in ((1 << k) - 1, 1 << k)]
    L = b"".join(bytes([1 + (i & 1)]) * (x + 1) for i, x in enumerate(runs))
    add("runs_of_1_2_3_4_and_powers_of_two_to_65536", [col(L, valid_orig(L, 5))])
    add("block_of_one_run", [col(b"Q" * 7, 3)])
    L = bytes(range(255, -1, -1))
    assert mtf_rle2(L, list(range(256)))[0] == 256
    add("mtf_index_255_all_256_values", [col(L, valid_orig(L, 255))])

    # ---- limits and the symbol map
    add("nblock_100000_at_level_1", [col(b"\x41" * 100000, 99999)], level=1)
    add("symbol_map_only_byte_0", [col(b"\x00" * 7, 0)])
    add("symbol_map_only_byte_255", [col(b"\xff" * 7, 6)])
    L = random_column(r, 100, list(range(0x40, 0x50)))
    add("symbol_map_one_sixteen", [col(L, valid_orig(L))])
    L = random_column(r, 700, list(range(256))) + bytes(range(256))
    add("symbol_map_all_256", [col(L, valid_orig(L, 256))])
    L = random_column(r, 100, [0x41, 0x42, 0xE0])
    add("symbol_map_sixteen_set_but_empty", [col(L, valid_orig(L), symmap=(0x0802 | 0x0100, [0x6000, 0, 0x8000]))])

    # ---- stream shape
    for level in range(1, 10):
        add("header_level_%d" % level, [tiny(level)], level=level)
    empty = lambda level: stream([], level)[0]  # noqa: E731
    a, b = stream([tiny(1), tiny(2)], 3), stream([tiny(3)], 7)
    cat["empty_stream_in_front"] = (empty(1) + a[0] + b[0], a[1] + b[1])
    cat["empty_stream_in_the_middle"] = (a[0] + empty(9) + empty(2) + b[0], a[1] + b[1])
    cat["empty_stream_at_the_end"] = (a[0] + b[0] + empty(5), a[1] + b[1])
    one, nine = stream([col(b"\x42" * 100000, 0)], 1), stream([col(b"\x43" * 100001, 50000), tiny(9)], 9)
    cat["level_1_then_level_9_with_nblock_100001"] = (a[0] + one[0] + nine[0], a[1] + one[1] + nine[1])
    cat["level_9_with_nblock_100001_then_level_1"] = (nine[0] + one[0], nine[1] + one[1])
    for name, tail in (("1_byte", b"\x00"), ("2_bytes", b"ZB"), ("3_bytes", b"BZ\x00"), ("16_bytes_no_header", b"BZh0 is no level"), ("64_zero_bytes", b"\0" * 64)):
        cat[TRAILING + name] = (a[0] + tail, a[1])

    # ---- false magics: spelled by Huffman bits, four times and more, in front of a real block
    for name, magic in (("block", MAGIC_BLOCK), ("end_of_stream", MAGIC_END)):
        s, out = add("false_%s_magic_five_times" % name, [spelled_block(r, magic, 5), tiny(0)])
        assert count_bits(s, magic) >= 5 + (2 if magic == MAGIC_BLOCK else 1)
    s, out = add("false_block_magic_in_front_of_the_end_magic", [tiny(4), spelled_block(r, MAGIC_BLOCK, 1)])
    assert count_bits(s, MAGIC_BLOCK) >= 3
    for name in cat:
        offsets.setdefault(name, [])
    return cat, offsets


def catalogue():
    """name -> (stream bytes, decoded bytes): every one a stream libbz2 accepts"""
    return _build()[0]


def block_offsets():
    """name -> the bit offsets of the stream's real blocks (single-stream entries)"""
    return _build()[1]


# ---------------------------------------------------------------- invalid streams
# bz2.decompress drops whatever fails behind a good first stream; the bzip2 program (bzip2.c, uncompressStream: only bytes
# that are no stream header are "trailing garbage") and the device refuse these
PYTHON_ACCEPTS = {"good_stream_then_header_and_garbage", "stream_crc_wrong_in_stream_2_of_3"}
BAD_BLOCK = {"block_crc_wrong_in_block_2_of_4": 2, "garbage_where_the_next_block_magic_is_due": 1}  # the block the message names
R_TRUNCATED, R_NOT_BZIP2 = "truncated", "not bzip2"


def truncation_stream():
    """-> (bytes of two streams, three blocks; the length of the first stream; the first stream's output)"""
    a = stream([data_block(b"@first block, stream one\nACGTTGCAAGGCTTAACCGGTTAGCATGCATCGATCGGATC\n+\nIIIIHHGGFFEEDDCCBBAA@@??>>==<<;;::9988776\n"),
                data_block(b"@second block 0123456789 of the same stream\nGATTACAGATTACACATTAG\n+\n!\"#$%&'()*+,-./01234\n")], 4)
    b = stream([data_block(b"@third block: stream two, level two\nTTGACCANNNNACGT\n+\nJJJJJIIIHHHGGFF\n")], 2)
    return a[0] + b[0], len(a[0]), a[1]


@functools.lru_cache(None)
def invalid():
    """name -> (stream bytes, the wording of reason_text (exg_bzip2.hip) expected in the message, or "truncated" / "not bzip2",
    the clause of libbz2's decompress.c that refuses it)"""
    inv = {}
    text = b"hello bzip2 world, this block is damaged\n"
    base = data_block(text)
    used = sorted(set(base["L"]))
    alpha, eob = len(used) + 2, len(used) + 1
    uni = uniform_lengths(alpha)

    def add(name, blocks, reason, clause, level=9, **kw):
        inv[name] = (stream(blocks, level, **kw)[0], reason, clause)

    raw = lambda **kw: dict({"L": None, "used": used, "block_crc": 0x12345678}, **kw)  # noqa: E731
    add("symbol_map_empty", [dict(base, symmap=(0, []))], "no byte values in use", "if (s->nInUse == 0) RETURN(BZ_DATA_ERROR)")
    for ng in (0, 1, 7):
        add("ngroups_%d" % ng, [dict(base, n_groups=ng)], "number of Huffman groups outside 2..6", "if (nGroups < 2 || nGroups > BZ_N_GROUPS) RETURN(BZ_DATA_ERROR)")
    add("nselectors_0", [dict(base, n_selectors=0, written=0)], "bad selector", "if (nSelectors < 1) RETURN(BZ_DATA_ERROR)")
    add("selector_unary_run_reaches_ngroups", [dict(base, selector_bits="11", written=0, n_selectors=1)], "bad selector", "if (j >= nGroups) RETURN(BZ_DATA_ERROR)")
    why = "Huffman code length outside 1..20"
    clause = "if (curr < 1 || curr > 20) RETURN(BZ_DATA_ERROR)"
    rest = "0" * alpha
    add("code_length_start_0", [dict(base, table_bits=["00000" + rest, None])], why, clause)
    add("code_length_start_21", [dict(base, table_bits=[None, "10101" + rest])], why, clause)
    add("code_length_delta_reaches_0", [dict(base, table_bits=["00010" + "0" + "11" + "11" + "10" + rest, None])], why, clause)
    add("code_length_delta_reaches_21_and_returns", [dict(base, table_bits=["10011" + "0" + "10" + "10" + "11" + rest, None])], why, clause)
    add("symbol_matches_no_code_by_20_bits", [raw(syms=[(20, 0xFFFFF), (20, 0)], tables=[[20] * alpha] * 2)], "bad Huffman code", "if (zn > 20 /* the longest code */) RETURN(BZ_DATA_ERROR)")
    add("symbols_past_the_last_selector", [raw(syms=[2, 3] * 30 + [eob], selectors=[0, 0], written=1)], "symbols run past the last selector",
        "if (groupNo >= nSelectors) RETURN(BZ_DATA_ERROR)")
    add("run_weight_reaches_2_21", [raw(syms=[0] * 22 + [eob])], "run length too large", "if (N >= 2*1024*1024) RETURN(BZ_DATA_ERROR)")
    big = "block larger than the stream's level allows"
    for level in (1, 2):
        n = level * 100000
        add("nblock_over_the_limit_by_a_run_level_%d" % level, [raw(syms=run_syms(n + 1) + [eob])], big, "if (nblock >= nblockMAX) RETURN(BZ_DATA_ERROR) (in the run)", level)
        add("nblock_over_the_limit_by_one_symbol_level_%d" % level, [raw(syms=run_syms(n) + [2, eob])], big, "if (nblock >= nblockMAX) RETURN(BZ_DATA_ERROR) (at the symbol)", level)
    add("end_of_block_first", [raw(syms=[eob])], "origPtr outside the block", "if (s->origPtr < 0 || s->origPtr >= nblock) RETURN(BZ_DATA_ERROR)")
    for name, field in (("equals_nblock", len(base["L"])), ("2_24_minus_1", (1 << 24) - 1)):
        add("origptr_" + name, [dict(base, orig_field=field)], "origPtr outside the block", "if (s->origPtr < 0 || s->origPtr >= nblock) RETURN(BZ_DATA_ERROR)")
    L, o = bwt(b"the fourth equal byte is last: AAAA")
    assert inverse(L, o) is None
    add("block_ends_where_a_count_is_due", [{"L": L, "orig": o}], "block ends where a run-length byte is due",
        "unRLE_obuf_to_output_*: nblock_used runs past save_nblock + 1 (BZ_DATA_ERROR from BZ2_bzDecompress)")
    four = [data_block(b"block %d of four\n" % k) for k in range(4)]
    good = [crc(inverse(b["L"], b["orig"])) for b in four]
    add("block_crc_wrong_in_block_0", [dict(four[0], block_crc=good[0] ^ 1)] + four[1:], "block CRC mismatch", "if (s->calculatedBlockCRC != s->storedBlockCRC) return BZ_DATA_ERROR")
    add("block_crc_wrong_in_block_2_of_4", four[:2] + [dict(four[2], block_crc=good[2] ^ 0x80000000)] + four[3:], "block CRC mismatch",
        "if (s->calculatedBlockCRC != s->storedBlockCRC) return BZ_DATA_ERROR")
    ok = stream(four[:2], 5)[0]
    inv["stream_crc_wrong_in_stream_2_of_3"] = (ok + stream(four[2:], 1, stream_crc=0xDEADBEEF)[0] + ok, "stream CRC mismatch",
                                                "if (s->calculatedCombinedCRC != s->storedCombinedCRC) return BZ_DATA_ERROR")
    # (libbz2 derandomises: it flips a bit of byte 618 first, so a block that long, never randomised, fails its CRC)
    add("randomised_block", [dict(data_block(text * 20), randomised=1)], "randomised", "BZ_RAND_UPD_MASK, then the block CRC: return BZ_DATA_ERROR")
    add("garbage_where_the_next_block_magic_is_due", [four[0], dict(four[1], magic=0x31415926535A)], "bad block magic", "if (uc != 0x59) RETURN(BZ_DATA_ERROR)")
    whole, cut_ok, _ = truncation_stream()
    for cut in range(1, len(whole)):
        if cut != cut_ok:
            inv["truncated_at_%d" % cut] = (whole[:cut], R_NOT_BZIP2 if cut < 4 else R_TRUNCATED, "BZ_UNEXPECTED_EOF")
    for name, head in (("BZh0", b"BZh0"), ("BZh_colon", b"BZh:"), ("BZg9", b"BZg9")):
        add("header_" + name, [four[0]], R_NOT_BZIP2, "RETURN(BZ_DATA_ERROR_MAGIC)", header=head)
    inv["good_stream_then_header_and_garbage"] = (ok + b"BZh9" + bytes(range(1, 41)), "bad block magic", "RETURN(BZ_DATA_ERROR) at the block magic; bz2.decompress drops it")
    return inv


# ---------------------------------------------------------------- the generator
R_RUN_AT_END = "block ends where a run-length byte is due"


def generate(seed):
    """A random column, heavy in long runs -> (stream bytes, decoded bytes, None), or (stream bytes, None, reason) when the
    column's text ends where a count byte is due: such a seed is an invalid case, not drawn again"""
    r = random.Random("generate/%d" % seed)
    n = r.choice(NBLOCKS)
    values = r.sample(range(256), r.choice((1, 2, 3, 4, 16, 17, 255, 256)))
    L = random_column(r, n, values, runs=True)
    how = r.choice(("first", "last", "random", "stride"))
    orig = {"first": 0, "last": n - 1, "random": r.randrange(n), "stride": r.randrange((n + 255) // 256) * 256}[how]
    blk = with_tables(r, {"L": L, "orig": orig}, r.randint(2, 6))
    lead = [data_block(bytes(r.choice(b"ACGTN\n") for _ in range(r.randint(1, 40))))] if r.random() < 0.7 else []
    out = inverse(L, orig)
    s, o = stream(lead + [blk], r.randint(1, 9))
    return (s, o, None) if out is not None else (s, None, R_RUN_AT_END)


# ---------------------------------------------------------------- a hand-built FASTQ file for the reader, and the reader's rounds
def fastq_text(n, seed):
    r = random.Random("fastq/%d" % seed)
    out = []
    for i in range(n):
        k = r.randint(60, 150)
        out.append("@read%d len=%d\n%s\n+\n%s\n" % (i, k, "".join(r.choice("ACGT") for _ in range(k)), "".join(chr(33 + r.randint(2, 40)) for _ in range(k))))
    return "".join(out).encode()


READER_PADS = ((11, 6080), (24, 10428), (37, 21936))  # (block, surplus selectors): see reader_file


@functools.lru_cache(None)
def _reader_blocks():
    text = fastq_text(330, 1)
    r = random.Random("reader")
    chunks, at = [], 0
    while at < len(text):
        k = r.randint(1700, 2300)
        chunks.append(text[at:at + k])
        at += k
    assert 36 <= len(chunks) <= 46
    blocks = []
    for i, c in enumerate(chunks):
        b = data_block(c)
        b["used"] = sorted(set(b["L"]))
        b["syms"] = mtf_rle2(b["L"], b["used"])
        alpha = len(b["used"]) + 2
        kind = i % 8
        if kind == 0:
            b = with_tables(r, b, 6)
        elif kind == 1:
            b["tables"] = [[11] * alpha] * 2
        elif kind == 2:
            b["tables"] = [uniform_lengths(alpha), ramp_lengths(alpha), [20] * alpha]
        elif kind == 3:
            b["tables"] = [uniform_lengths(alpha), [1] * alpha]
            if i in (3, 11):
                b["table_bits"] = [None, spelled_table(MAGIC_BLOCK if i == 3 else MAGIC_END, alpha)]
        elif kind == 4:
            b["tables"] = [[20] * alpha] * 2
        elif kind == 5:
            b = with_tables(r, b, 3, maxlen=12)
        elif kind == 6:
            b["tables"] = [[x + 1 for x in uniform_lengths(alpha)]] * 2  # incomplete
        b.setdefault("selectors", [0] * ((len(b["syms"]) + 49) // 50))
        blocks.append(b)
    return text, blocks


@functools.lru_cache(None)
def reader_file(pads=None):
    """About 40 blocks of about 2 KB of FASTQ text in three streams (levels 1, 2, 9) with an empty stream between the first
    two, odd tables, and the two magics spelled by the length bits of unused tables.  pads = ((block, k), ..): k surplus
    selectors behind that block's own, a bit each, shift everything behind them; READER_PADS puts a stream header, an end
    magic, a CRC and the padding behind it on window edges of the reader (test_bzip2_frames.py computes which).
    -> (file bytes, text, layout): layout = [("header", bit, bit + 32) | ("block", bit, end) | ("end", bit, bit + 48) |
    ("crc", bit, bit + 32) | ("pad", bit, end)] in file order"""
    text, blocks = _reader_blocks()
    blocks = list(blocks)
    for i, k in READER_PADS if pads is None else pads:
        blocks[i] = dict(blocks[i], selectors=list(blocks[i]["selectors"]) + [blocks[i]["selectors"][-1]] * k)
    cut1, cut2 = len(blocks) // 3, 2 * len(blocks) // 3
    parts = [(blocks[:cut1], 1), ([], 5), (blocks[cut1:cut2], 2), (blocks[cut2:], 9)]
    data, layout, out = b"", [], b""
    for blks, level in parts:
        info = {}
        s, o = stream(blks, level, info=info)
        base = 8 * len(data)
        layout.append(("header", base, base + 32))
        ends = info["blocks"][1:] + [info["end"]]
        layout += [("block", base + a, base + e) for a, e in zip(info["blocks"], ends)]
        layout += [("end", base + info["end"], base + info["end"] + 48), ("crc", base + info["end"] + 48, base + info["bits"]),
                   ("pad", base + info["bits"], base + 8 * len(s))]
        data += s
        out += o
    assert out == text
    assert count_bits(data, MAGIC_BLOCK) == len(blocks) + 1 and count_bits(data, MAGIC_END) == len(parts) + 1
    return data, text, layout


def magic_offsets(data):
    s = format(int.from_bytes(data, "big"), "0%db" % (8 * len(data)))
    found = []
    for magic in (MAGIC_BLOCK, MAGIC_END):
        pat, at = format(magic, "048b"), -1
        while True:
            at = s.find(pat, at + 1)
            if at < 0:
                break
            found.append(at)
    return sorted(found)


def rounds(data, layout, window, max_blocks=None):
    """The rounds of the reader's bzip2 producer (exg_rd_bzip2.cpp, k_chain) on a valid file, restated: the window begins at
    the carried bit's byte rounded down to 16 and holds window x grow bytes; a round takes the stream headers, blocks (at
    most max_blocks, among the first 2 max_blocks + 2 magics found in the window) and ends of stream that lie whole inside
    it; a round without progress doubles grow.  -> [{lo, end (bytes), grow, blocks, progress}]"""
    n = len(data)
    cands = magic_offsets(data)
    what = {a: (kind, e) for kind, a, e in layout if kind in ("block", "end")}
    bit, at_header, grow, out = 0, True, 1, []
    while True:
        lo = (bit >> 3) & ~15
        end = lo + min(window * grow, n - lo)
        final = end >= n
        inside = [c for c in cands if c >= bit and c + 48 <= 8 * end]
        decoded = inside if max_blocks is None else inside[:2 * max_blocks + 2]
        p, m, hdr, done = bit, 0, at_header, False
        while True:
            if hdr:
                b = p >> 3
                if b + 4 > end or data[b:b + 3] != b"BZh":
                    done = final or (b + 4 <= end)
                    break
                p, hdr = p + 32, False
                continue
            if (max_blocks is not None and m >= max_blocks) or p not in decoded:
                break
            kind, e = what[p]
            if kind == "end":
                if p + 80 > 8 * end:
                    break
                p, hdr = (p + 80 + 7) & ~7, True
                continue
            if e > 8 * end:
                break
            p, m = e, m + 1
        progress = bool(m) or p != bit or hdr != at_header
        out.append({"lo": lo, "end": end, "grow": grow, "blocks": m, "progress": progress})
        if m:
            grow = 1
        elif not progress:
            grow *= 2
        bit, at_header = p, hdr
        if done:
            return out
        assert progress or not final, "the model made no progress in the last window"


def straddled(layout, rs, n):
    """the kinds of structure that a window edge of these rounds cuts.  An edge is a whole byte, so the padding (less than a
    byte, in the CRC's last byte) counts as cut when the edge falls on either side of that byte"""
    kinds = set()
    for r in rs:
        e = 8 * r["end"]
        if r["end"] >= n:
            continue
        for kind, a, b in layout:
            if kind == "pad":
                if b > a and e in (a & ~7, b):
                    kinds.add(kind)
            elif a < e < b:
                kinds.add(kind)
    return kinds
