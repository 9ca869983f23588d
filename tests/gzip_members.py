"""A gzip (RFC 1952) / BGZF (SAM spec 4.1) member writer that takes orders: every field of a member is chosen by the caller.

gzip.compress and bgzip write one header form each.  This writer builds the rest by hand, the way tests/deflate_frames.py does for
the DEFLATE stream inside and tests/zstd_frames.py for zstd:

    member(payload, ...)    -> Member (bytes + what the writer knows about it: hdr_len, sized, bsize, payload)
    bgzf(data, block, ...)  -> canonical BGZF members (FLG = 4, XLEN = 6, 'BC' first) + the EOF block: THE BGZF writer of the tests
    valid() / invalid()     -> name -> Case; every case names the clause it exercises and carries feature tags
    REQUIRED_TAGS           -> what the catalogue must reach (asserted when the catalogue is built)

A Case holds the file (`data`), its members as the writer laid them out (`parts`), and what reading it gives: `text` — for a
valid case the whole decoded text, for an invalid one the text of the whole members in front of the error.  Three kinds of
invalid case differ from zlib's one-shot decoder on purpose (oracle/pyoracle.py decode_by_rule lists them; `differs` names which):

    bsize_binds   a 'BC' subfield with SLEN 2 states the member's size and the reader holds the member to it; zlib skips FEXTRA
                  unread and reads the file without error
    partial       the error lies inside a member: zlib hands out what it decoded of that member so far, the reader nothing of it
    streamed      a big member (chunked decoder) with a wrong trailer: its rows come before the error, as from a streaming
                  decoder; one-shot zlib gives nothing of it

tests/test_gzip_members.py proves the writer against zlib (decode_by_rule) before tests/test_gzip_members_gpu.py judges the
device reader."""
import random
import struct
import zlib

import deflate_frames as df

FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16
BC = (b"BC", None)            # in a subfield list: the BGZF subfield, its BSIZE filled in by member()


def raw_deflate(payload, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return co.compress(payload) + co.flush()


class Member(bytes):
    """the bytes of one member + the writer's account of it"""
    hdr_len = 0          # bytes in front of the DEFLATE stream
    sized = False        # a 'BC' subfield with SLEN = 2 inside XLEN: the index takes its size from BSIZE
    bsize = None         # the BSIZE written (None: no BC subfield)
    isize = 0            # the ISIZE field as written
    payload = b""


def member(payload, *, id1=0x1F, id2=0x8B, cm=8, flg=None, flg_or=0, mtime=0, xfl=0, os=255, extra=None, xlen=None, fname=None,
           fcomment=None, fhcrc=None, body=None, level=6, slack=b"", crc=None, isize=None, bsize=None, bsize_delta=0):
    """extra: list of (two id bytes, data) subfields, BC among them for the BGZF one (None: no FEXTRA; []: XLEN = 0); xlen: the raw
    XLEN field when it should not be the subfields' size; fname / fcomment: bytes without their NUL (None: none);
    fhcrc: True = the right CRC16, an int = that value; flg: the whole FLG byte instead of the one the fields imply, flg_or: bits
    set on top of it; body: the raw DEFLATE stream instead of zlib's; slack: bytes between the stream and the trailer;
    crc / isize / bsize: the fields instead of the right values (bsize_delta: added to the right BSIZE)"""
    payload = bytes(payload)
    body = raw_deflate(payload, level) if body is None else bytes(body)
    f = 0
    if extra is not None:
        f |= FEXTRA
    if fname is not None:
        f |= FNAME
    if fcomment is not None:
        f |= FCOMMENT
    if fhcrc is not None:
        f |= FHCRC
    f = (f if flg is None else flg) | flg_or
    subs = b"".join(si + struct.pack("<H", 2 if d is None else len(d)) + (b"\0\0" if d is None else d) for si, d in (extra or []))
    opt = b""
    if extra is not None:
        opt += struct.pack("<H", len(subs) if xlen is None else xlen) + subs
    if fname is not None:
        opt += fname + b"\0"
    if fcomment is not None:
        opt += fcomment + b"\0"
    hdr_len = 10 + len(opt) + (2 if fhcrc is not None else 0)
    total = hdr_len + len(body) + len(slack) + 8
    has_bc = any(d is None for _, d in (extra or []))
    bs = None
    if has_bc:
        bs = (total - 1 + bsize_delta) if bsize is None else bsize
        subs = b"".join(si + struct.pack("<H", 2 if d is None else len(d)) + (struct.pack("<H", bs & 0xFFFF) if d is None else d)
                        for si, d in extra)
        opt = struct.pack("<H", len(subs) if xlen is None else xlen) + subs + opt[2 + len(subs):]
    head = bytes([id1, id2, cm, f]) + struct.pack("<IBB", mtime, xfl, os) + opt
    if fhcrc is not None:
        head += struct.pack("<H", (zlib.crc32(head) & 0xFFFF) if fhcrc is True else fhcrc)
    assert len(head) == hdr_len
    isz = len(payload) & 0xFFFFFFFF if isize is None else isize
    m = Member(head + body + slack + struct.pack("<II", zlib.crc32(payload) if crc is None else crc, isz))
    m.hdr_len, m.bsize, m.isize, m.payload = hdr_len, bs, isz, payload
    m.sized = has_bc and (xlen is None or xlen >= len(subs))
    return m


def bgzf_member(payload, level=6, **kw):
    """one canonical BGZF member (what bgzip / htslib write)"""
    return member(payload, extra=[BC], level=level, **kw)


EOF_BLOCK = bgzf_member(b"")
assert EOF_BLOCK == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_members(data, block=65280, level=6, eof=True):
    data = bytes(data)
    return [bgzf_member(data[i:i + block], level) for i in range(0, len(data), block)] + ([EOF_BLOCK] if eof else [])


def bgzf(data, block=65280, level=6, eof=True):
    """`data` as canonical BGZF members of `block` inflated bytes each, with the empty EOF block behind them"""
    return b"".join(bgzf_members(data, block, level, eof))


# ---- payloads -------------------------------------------------------------------------------------------------------------------
FQ = b"@r1 first\nACGT\n+\n!!!!\n@r2\nGGA\n+\nIII\n@r3 x y\nT\n+\n#\n"          # three records, 51 bytes
FQ2 = b"@s1\nTTAG\n+\nFFFF\n@s2 d\nC\n+\n5\n"
TINY_A, TINY_B, TINY_C = b"@a\nAC\n+\n!!\n@b\nG", b"T\n+\n##\n@c\nT\n", b"+\nI\n@d\nA\n+\n~\n"
VCF = (b"##fileformat=VCFv4.2\n##contig=<ID=1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
       b"1\t5\trs1\tA\tC\t3.5\tPASS\t.\n1\t9\t.\tG\tT,A\t.\t.\t.\n")
FA = b">s1 d\nACGT\nAC\n>s2\nGG\n"


def fastq_of_size(n, seed, line=150, alphabet=None):
    """a FASTQ text of exactly n bytes (n >= 40): records with `line` bases (15 letters) and random qualities (94 symbols unless
    `alphabet` says otherwise), the last one sized to fit"""
    rng = random.Random(seed)
    qual = alphabet or bytes(range(33, 127))
    out, k = bytearray(), 0
    while len(out) < n:
        left = n - len(out)
        name = b"@q%d" % k
        fixed = len(name) + 5                     # the newline behind the name, "\n+\n", the last newline
        ln = line
        if left < fixed + 2 * line + 40:          # the last record: what is left, the name taking up the odd byte
            ln = (left - fixed) // 2
            name += b"x" * (left - fixed - 2 * ln)
        assert ln >= 1
        seq = bytes(rng.choice(b"ACGTNRYKMSWBDHV") for _ in range(ln))
        out += name + b"\n" + seq + b"\n+\n" + bytes(rng.choice(qual) for _ in range(ln)) + b"\n"
        k += 1
    assert len(out) == n, (len(out), n)
    return bytes(out)


class Case:
    def __init__(self, name, parts, text, clause, tags, differs=None, refused_by_index=False, pure_bgzf=False, env=None,
                 reader=None):
        self.name, self.parts, self.text, self.clause, self.tags = name, [p for p in parts], bytes(text), clause, set(tags)
        self.data = b"".join(self.parts)
        self.differs, self.refused_by_index, self.pure_bgzf = differs, refused_by_index, pure_bgzf
        self.env, self.reader = dict(env or {}), dict(reader or {})
        self.valid = True


def phase_tail(rec_no, a, b):
    """the last record of a text whose final DEFLATE block ends at bit phase (2 + 4 a + 5 b) % 8: -> (text in front of the final
    block, the final block's bytes, the text it adds).  The block is fixed-Huffman: a matches (3, 1) of 12 bits, b matches
    (11, 1) of 13 bits, the literal newline, end-of-block: 3 + 12 a + 13 b + 8 + 7 bits from a byte boundary"""
    n = 4 + 3 * a + 11 * b
    front = b"@z%d\n" % rec_no + b"A" * n + b"\n+\nIIII"
    blk = df.Stream([df.Fixed([(3, 1)] * a + [(11, 1)] * b + [10], final=True)])
    raw, info = df._encode(blk)
    assert info["end_bit"] % 8 == (2 + 4 * a + 5 * b) % 8
    return front, raw, b"I" * (3 * a + 11 * b) + b"\n"


PHASES = {(2 + 4 * a + 5 * b) % 8: (a, b) for b in range(4) for a in range(2)}


def phased_body(text, phase, level=6):
    """-> (raw DEFLATE, payload): `text` by zlib up to a sync flush (byte aligned), then the hand-built final block"""
    a, b = PHASES[phase]
    front, blk, tail = phase_tail(phase, a, b)
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    raw = co.compress(text + front) + co.flush(zlib.Z_SYNC_FLUSH) + blk
    return raw, text + front + tail


_BIG = {}


def big_text():
    """~230 KB of FASTQ whose level-9 DEFLATE stream is >= 128 KiB: a plain member of it takes the chunked decoder"""
    if "t" not in _BIG:
        _BIG["t"] = fastq_of_size(230_000, seed=7)
        assert len(raw_deflate(_BIG["t"], 9)) >= (128 << 10) + 2048
    return _BIG["t"]


REQUIRED_TAGS = frozenset(
    ["hdr:ftext", "hdr:mtime_xfl_os_ff", "hdr:xlen0", "hdr:non_bc_subfield", "hdr:xlen65535", "hdr:fname_empty", "hdr:fname_latin1_300",
     "hdr:longer_than_70000"] + ["hdr:combo%02d" % c for c in range(16)]
    + ["bc:canonical", "bc:second", "bc:then_other", "bc:xlen240", "bc:xlen241", "bc:xlen246", "bc:slen_not_2", "bc:with_fname", "bc:with_fhcrc",
       "bc:twice"]
    + ["empty:eof_first", "empty:eof_middle", "empty:eof_twice", "empty:eof_only", "empty:eof_absent", "empty:plain_alone", "empty:plain_between"]
    + ["size:isize1", "size:isize65280", "size:isize65535", "size:isize65536", "size:member65536", "size:isize65537_bc"]
    + ["cut:one_byte_members", "cut:every_byte_of_a_record", "cut:window_256k", "cut:window_256k_small_segments", "cut:plain_x300",
       "cut:plain_bgzf_plain"]
    + ["big:plain", "big:fextra", "big:fname", "big:fcomment", "big:fhcrc"]
    + ["phase:%s%d" % (p, k) for p in ("bgzf", "small", "big") for k in range(8)]
    + ["bad:id1", "bad:id2", "bad:cm7", "bad:cm9", "bad:flg_bit5", "bad:flg_bit6", "bad:flg_bit7", "bad:fhcrc", "bad:xlen_past_eof",
       "bad:fname_open", "bad:fcomment_open", "bad:cut_plain", "bad:cut_bgzf"]
    + ["bad:crc_byte%d_%s" % (k, p) for k in range(4) for p in ("bgzf", "small")] + ["bad:crc_big"]
    + ["bad:isize_%s_%s" % (w, p) for w in ("minus1", "plus1", "zero", "ffffffff") for p in ("bgzf", "small", "big")]
    + ["bad:bsize_minus1", "bad:bsize_plus1", "bad:bsize_below_header", "bad:bsize_past_eof", "bad:bsize_next_member", "bad:slack"]
    + ["bad:tail_%s_%s" % (t, p) for t in ("zero1", "zero17", "zero18", "magic", "text") for p in ("bgzf", "plain")])

_VALID = _INVALID = None


def _check(cases):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return {c.name: c for c in cases}


def valid():
    """name -> Case whose rows are the rows of case.text"""
    global _VALID
    if _VALID is None:
        _VALID = _check(_build_valid())
    return _VALID


def invalid():
    """name -> Case that ends in an error behind the rows of case.text"""
    global _INVALID
    if _INVALID is None:
        _INVALID = _check(_build_invalid())
        for c in _INVALID.values():
            c.valid = False
        missing = REQUIRED_TAGS - set().union(*(c.tags for c in list(valid().values()) + list(_INVALID.values())))
        assert not missing, sorted(missing)
    return _INVALID


def _build_valid():
    c = []
    add = lambda *a, **kw: c.append(Case(*a, **kw))   # noqa: E731
    X = (b"XX", b"\1\2\3")
    # ---- header forms (RFC 1952 2.3)
    add("hdr_mtime_xfl_os_ff", [member(FQ, mtime=0xFFFFFFFF, xfl=0xFF, os=0xFF)], FQ, "2.3: MTIME, XFL, OS are not interpreted", ["hdr:mtime_xfl_os_ff"])
    add("hdr_ftext", [member(FQ, flg_or=FTEXT, mtime=0xFFFFFFFF, xfl=0xFF, os=0xFF)], FQ, "2.3.1: FTEXT is a hint", ["hdr:ftext"])
    for combo in range(16):
        kw = {}
        if combo & 1:
            kw["extra"] = [X]
        if combo & 2:
            kw["fname"] = b"reads.fastq"
        if combo & 4:
            kw["fcomment"] = b"a comment"
        if combo & 8:
            kw["fhcrc"] = True
        add("hdr_combo_%02d" % combo, [member(FQ, **kw), member(FQ2)], FQ + FQ2, "2.3.1: FEXTRA / FNAME / FCOMMENT / FHCRC in any combination",
            ["hdr:combo%02d" % combo] + (["hdr:non_bc_subfield"] if combo == 1 else []))
    add("hdr_xlen_0", [member(FQ, extra=[]), member(FQ2)], FQ + FQ2, "2.3.1: XLEN = 0", ["hdr:xlen0"])
    add("hdr_xlen_65535", [member(FQ, extra=[(b"XX", b"\x1f\x8b\x08" * 21843 + b"\0\0")]), member(FQ2)], FQ + FQ2, "2.3.1: XLEN is 16 bits", ["hdr:xlen65535"])
    add("hdr_fname_empty", [member(FQ, fname=b""), member(FQ2)], FQ + FQ2, "2.3.1: FNAME is zero-terminated: may be empty", ["hdr:fname_empty"])
    add("hdr_fname_latin1_300", [member(FQ, fname=bytes(range(0xA0, 0xFF)) * 3 + b"\xe9" * 15), member(FQ2)], FQ + FQ2, "2.3.1: FNAME is ISO 8859-1, any length",
        ["hdr:fname_latin1_300"])
    long_hdr = member(FQ, extra=[(b"XX", b"y" * 65531)], fname=b"n" * 3000, fcomment=b"c" * 3000, fhcrc=True)
    assert long_hdr.hdr_len > 70000
    add("hdr_longer_than_70000", [long_hdr, member(FQ2)], FQ + FQ2, "2.3.1: no field of the header bounds its length", ["hdr:longer_than_70000"])
    # ---- where the BC subfield stands (SAM spec 4.1: "BC" with SLEN 2, among other subfields)
    pad = lambda n: (b"PD", b"\0" * (n - 10))          # noqa: E731  (pads XLEN to n beside a BC subfield)
    add("bc_canonical", [bgzf_member(FQ), bgzf_member(FQ2), EOF_BLOCK], FQ + FQ2, "SAM 4.1: FLG 4, XLEN 6, BC first", ["bc:canonical"], pure_bgzf=True)
    add("bc_second", [member(FQ, extra=[X, BC]), bgzf_member(FQ2), EOF_BLOCK], FQ + FQ2, "SAM 4.1: other subfields may precede BC", ["bc:second"], pure_bgzf=True)
    add("bc_then_other", [member(FQ, extra=[BC, X]), bgzf_member(FQ2), EOF_BLOCK], FQ + FQ2, "SAM 4.1: other subfields may follow BC", ["bc:then_other"], pure_bgzf=True)
    for n in (240, 241, 246):   # the BGZF walk takes XLEN <= 240; longer ones are read as plain members held to their BSIZE
        add("bc_xlen_%d" % n, [bgzf_member(FQ), member(FQ2, extra=[BC, pad(n)]), bgzf_member(FQ), EOF_BLOCK], FQ + FQ2 + FQ, "SAM 4.1: XLEN is not bounded",
            ["bc:xlen%d" % n], pure_bgzf=n == 240)
    add("bc_slen_3", [member(FQ, extra=[(b"BC", b"\x10\0\0")]), member(FQ2)], FQ + FQ2, "SAM 4.1: BC has SLEN 2: another SLEN is another subfield", ["bc:slen_not_2"])
    add("bc_with_fname", [member(FQ, extra=[BC], fname=b"x.fastq"), bgzf_member(FQ2)], FQ + FQ2, "RFC 1952: a member with FEXTRA and FNAME", ["bc:with_fname"])
    add("bc_with_fhcrc", [member(FQ, extra=[BC], fhcrc=True), bgzf_member(FQ2)], FQ + FQ2, "RFC 1952: a member with FEXTRA and FHCRC", ["bc:with_fhcrc"])
    # two BC subfields: the LAST one with SLEN 2 states the size (both walks overwrite as they go); the first here is wrong
    two = member(FQ, extra=[(b"BC", b"\x05\0"), BC])
    add("bc_twice_last_wins", [two, bgzf_member(FQ2), EOF_BLOCK], FQ + FQ2, "SAM 4.1 names one BC subfield; of two the last is taken", ["bc:twice"], pure_bgzf=True)
    # ---- empty members
    add("eof_first", [EOF_BLOCK, bgzf_member(FQ), bgzf_member(FQ2)], FQ + FQ2, "SAM 4.1.2: an empty block anywhere", ["empty:eof_first"], pure_bgzf=True)
    add("eof_middle", [bgzf_member(FQ), EOF_BLOCK, bgzf_member(FQ2), EOF_BLOCK], FQ + FQ2, "SAM 4.1.2: an empty block anywhere", ["empty:eof_middle"], pure_bgzf=True)
    add("eof_twice", [bgzf_member(FQ), EOF_BLOCK, EOF_BLOCK], FQ, "SAM 4.1.2", ["empty:eof_twice"], pure_bgzf=True)
    add("eof_only", [EOF_BLOCK], b"", "SAM 4.1.2: an empty file is the EOF block alone", ["empty:eof_only"], pure_bgzf=True)
    add("eof_absent", [bgzf_member(FQ), bgzf_member(FQ2)], FQ + FQ2, "SAM 4.1.2: the EOF block is optional to a reader", ["empty:eof_absent"], pure_bgzf=True)
    e = member(b"")
    assert len(e) == 20
    add("plain_empty_alone", [e], b"", "RFC 1952: a member may be empty (20 bytes)", ["empty:plain_alone"])
    add("plain_empty_between", [member(FQ), e, e, member(FQ2), e], FQ + FQ2, "RFC 1952 2.2: members follow one another", ["empty:plain_between"])
    # ---- sizes (SAM 4.1: a block inflates to at most 64 KiB, BSIZE is 16 bits)
    for n in (1, 65280, 65535, 65536):
        t = fastq_of_size(n + 100, seed=n)      # the member of n bytes begins and ends in the middle of a record
        add("bgzf_isize_%d" % n, [bgzf_member(t[:37]), bgzf_member(t[37:37 + n], level=9), bgzf_member(t[37 + n:]), EOF_BLOCK], t,
            "SAM 4.1: ISIZE 0 .. 65536", ["size:isize%d" % n], pure_bgzf=True)
    t = fastq_of_size(65505, seed=3)
    m = bgzf_member(t, body=df.encode(df.Stream([df.Stored(t, final=True)])))
    assert len(m) == 65536 and m.bsize == 65535
    add("bgzf_member_of_65536_bytes", [m, bgzf_member(FQ), EOF_BLOCK], t + FQ, "SAM 4.1: BSIZE = 65535", ["size:member65536"], pure_bgzf=True)
    t = fastq_of_size(65537, seed=4, alphabet=b"FI")
    add("isize_65537_with_bc", [bgzf_member(FQ), bgzf_member(t), bgzf_member(FQ2), EOF_BLOCK], FQ + t + FQ2, "RFC 1952: valid gzip, beyond a BGZF block",
        ["size:isize65537_bc"])
    # ---- boundaries
    forty = b"@name\n" + b"ACGTACGTACGTACG" + b"\n+\n" + b"IIIIIIIIIIIIIII" + b"\n"
    assert len(forty) == 40
    add("forty_one_byte_members", [bgzf_member(forty[i:i + 1]) for i in range(40)] + [EOF_BLOCK], forty, "RFC 1952 2.2: a record may span members",
        ["cut:one_byte_members"], pure_bgzf=True)
    rec = b"@r d\nACGTA\n+\n!#%')\n"
    text = b"".join(rec.replace(b"@r", b"@r%02d" % i) for i in range(len(rec) + 4))
    cuts, at = [0], 0
    for i in range(len(rec) + 4):
        cuts.append(at + 1 + i)      # record i is cut behind its byte i (the record is len(rec) + 2 bytes long)
        at += len(rec) + 2
    cuts.append(len(text))
    add("cut_at_every_byte_of_a_record", [bgzf_member(text[a:b]) for a, b in zip(cuts, cuts[1:])] + [EOF_BLOCK], text,
        "RFC 1952 2.2: a member boundary may fall on any byte of a record", ["cut:every_byte_of_a_record"], pure_bgzf=True)
    t = fastq_of_size(600_000, seed=5)
    blocks = bgzf_members(t, 65280, level=0)
    sizes = [len(b) for b in blocks]
    assert sum(sizes[:4]) < (256 << 10) < sum(sizes[:5])          # the fifth member straddles the end of the 256 KiB window
    add("straddles_256k_window", blocks, t, "the compressed window's end falls inside a member", ["cut:window_256k"], pure_bgzf=True)
    add("straddles_256k_window_small_segments", blocks, t, "... with a few members per segment", ["cut:window_256k_small_segments"], pure_bgzf=True,
        env={"EXG_STREAM_ROUND_OUT": "1"}, reader={"device_batch_bytes": 128 << 10})
    text = b"".join(b"@p%d\nAC\n+\n!!\n" % i for i in range(300))
    recs = [b"@p%d\nAC\n+\n!!\n" % i for i in range(300)]
    add("three_hundred_tiny_plain_members", [member(r, level=1 + i % 9) for i, r in enumerate(recs)], text, "RFC 1952 2.2: members follow one another",
        ["cut:plain_x300"])
    add("plain_bgzf_plain", [member(FQ, fname=b"a"), bgzf_member(FQ2), bgzf_member(TINY_A), EOF_BLOCK, member(TINY_B + TINY_C)], FQ + FQ2 + TINY_A + TINY_B + TINY_C,
        "RFC 1952 2.2: members of any form follow one another", ["cut:plain_bgzf_plain"])
    big = big_text()
    for tag, kw in (("plain", {}), ("fextra", {"extra": [X]}), ("fname", {"fname": b"big.fastq"}), ("fcomment", {"fcomment": b"c"}), ("fhcrc", {"fhcrc": True})):
        add("big_member_%s" % tag, [member(big, level=9, **kw), member(FQ)], big + FQ, "a member of >= 128 KiB takes the chunked decoder; a small one follows",
            ["big:" + tag])
    # ---- where the DEFLATE stream ends in its last byte: the trailer begins at the next byte boundary (RFC 1952 2.3)
    for ph in range(8):
        raw, payload = phased_body(FQ, ph)
        add("phase_%d_bgzf" % ph, [bgzf_member(FQ2), bgzf_member(payload, body=raw), bgzf_member(FQ2), EOF_BLOCK], FQ2 + payload + FQ2,
            "the final block ends at bit %d of its last byte" % ph, ["phase:bgzf%d" % ph], pure_bgzf=True)
        add("phase_%d_small" % ph, [member(payload, body=raw), member(FQ2)], payload + FQ2, "the final block ends at bit %d of its last byte" % ph,
            ["phase:small%d" % ph])
        raw, payload = phased_body(big, ph, level=9)
        assert len(raw) >= (128 << 10) + 1024
        add("phase_%d_big" % ph, [member(payload, body=raw), member(FQ2)], payload + FQ2, "the final block ends at bit %d of its last byte" % ph,
            ["phase:big%d" % ph])
    return c


def _build_invalid():
    c = []
    add = lambda *a, **kw: c.append(Case(*a, **kw))   # noqa: E731
    good = member(FQ)
    # ---- headers zlib refuses (the index refuses them too)
    for tag, kw, clause in (("id1", {"id1": 0x1E}, "2.3.1: ID1 = 31"), ("id2", {"id2": 0x8A}, "2.3.1: ID2 = 139"), ("cm7", {"cm": 7}, "2.3.1: CM = 8"),
                            ("cm9", {"cm": 9}, "2.3.1: CM = 8"), ("flg_bit5", {"flg_or": 32}, "2.3.1: reserved FLG bits must be zero"),
                            ("flg_bit6", {"flg_or": 64}, "2.3.1: reserved FLG bits must be zero"), ("flg_bit7", {"flg_or": 128}, "2.3.1: reserved FLG bits must be zero"),
                            ("fhcrc", {"fhcrc": 0x1234, "fname": b"n"}, "2.3.1: CRC16 of the header")):
        bad = member(FQ2, **kw)
        assert tag != "fhcrc" or (zlib.crc32(bad[:bad.hdr_len - 2]) & 0xFFFF) != 0x1234
        add("bad_%s" % tag, [good, bad, member(FQ)], FQ, clause, ["bad:" + tag], refused_by_index=True)
    m = member(FQ2, extra=[(b"XX", b"abc")], xlen=5000)
    add("bad_xlen_past_eof", [good, m], FQ, "2.3.1: XLEN bytes of extra field follow", ["bad:xlen_past_eof"], refused_by_index=True)
    m = member(FQ2, fname=b"name")
    add("bad_fname_open", [good, bytes(m).replace(b"name\0", b"name!").replace(b"\0", b"\1")[:40]], FQ, "2.3.1: FNAME is zero-terminated", ["bad:fname_open"],
        refused_by_index=True)
    m = member(FQ2, fcomment=b"cmnt")
    add("bad_fcomment_open", [good, bytes(m).replace(b"cmnt\0", b"cmnt!").replace(b"\0", b"\1")[:40]], FQ, "2.3.1: FCOMMENT is zero-terminated",
        ["bad:fcomment_open"], refused_by_index=True)
    # ---- every prefix of a two-member plain file and of a three-member BGZF file
    for kind, parts in (("plain", [member(TINY_A), member(TINY_B + TINY_C, fname=b"t")]), ("bgzf", [bgzf_member(TINY_A), bgzf_member(TINY_B), bgzf_member(TINY_C)])):
        whole = b"".join(parts)
        assert len(whole) <= 160, len(whole)
        ends, at = [], 0
        for p in parts:
            at += len(p)
            ends.append(at)
        for k in range(1, len(whole)):
            if k in ends:
                continue                      # (a cut between members leaves a valid file)
            n_whole = sum(1 for e in ends if e <= k)
            start = ends[n_whole - 1] if n_whole else 0
            inside = k - start > parts[n_whole].hdr_len          # the cut lies behind the header: zlib has begun to decode
            rest = Member(whole[start:k])                         # what is left of the member the cut falls in
            rest.hdr_len = parts[n_whole].hdr_len
            add("cut_%s_at_%03d" % (kind, k), parts[:n_whole] + [rest], b"".join(p.payload for p in parts[:n_whole]), "2.2: a member ends with its trailer",
                ["bad:cut_" + kind], differs="partial" if inside else None, refused_by_index=kind == "bgzf" or k - start < 18)
    # ---- trailers
    bg = lambda **kw: [bgzf_member(FQ), bgzf_member(FQ2, **kw), bgzf_member(FQ), EOF_BLOCK]      # noqa: E731
    sm = lambda **kw: [member(FQ), member(FQ2, **kw), member(FQ)]                                # noqa: E731
    big = big_text()
    bigm = lambda **kw: [member(FQ), member(big, level=9, **kw), member(FQ2)]                    # noqa: E731
    crc2 = zlib.crc32(FQ2)
    for k in range(4):
        add("crc_byte_%d_bgzf" % k, bg(crc=crc2 ^ (1 << (8 * k))), FQ, "2.3.1: CRC32 of the uncompressed data", ["bad:crc_byte%d_bgzf" % k])
        add("crc_byte_%d_small" % k, sm(crc=crc2 ^ (0x80 << (8 * k))), FQ, "2.3.1: CRC32 of the uncompressed data", ["bad:crc_byte%d_small" % k])
    add("crc_big", bigm(crc=zlib.crc32(big) ^ 0x00010000), FQ + big, "2.3.1: CRC32 of the uncompressed data", ["bad:crc_big"], differs="streamed")
    for tag, f in (("minus1", lambda n: n - 1), ("plus1", lambda n: n + 1), ("zero", lambda n: 0), ("ffffffff", lambda n: 0xFFFFFFFF)):
        add("isize_%s_bgzf" % tag, bg(isize=f(len(FQ2))), FQ, "2.3.1: ISIZE = the uncompressed size mod 2^32", ["bad:isize_%s_bgzf" % tag])
        add("isize_%s_small" % tag, sm(isize=f(len(FQ2))), FQ, "2.3.1: ISIZE = the uncompressed size mod 2^32", ["bad:isize_%s_small" % tag])
        add("isize_%s_big" % tag, bigm(isize=f(len(big))), FQ + big, "2.3.1: ISIZE = the uncompressed size mod 2^32", ["bad:isize_%s_big" % tag], differs="streamed")
    # ---- BSIZE (SAM 4.1: total block size minus 1).  zlib does not read it
    add("bsize_minus1", bg(bsize_delta=-1), FQ, "SAM 4.1: BSIZE = block size - 1", ["bad:bsize_minus1"], differs="bsize_binds")
    add("bsize_plus1", bg(bsize_delta=1), FQ, "SAM 4.1: BSIZE = block size - 1", ["bad:bsize_plus1"], differs="bsize_binds")
    add("bsize_below_header", bg(bsize=18 + 8 - 2), FQ, "SAM 4.1: a block holds its header and trailer", ["bad:bsize_below_header"], differs="bsize_binds")
    add("bsize_past_eof", [bgzf_member(FQ), bgzf_member(FQ2, bsize=4000)], FQ, "SAM 4.1: BSIZE = block size - 1", ["bad:bsize_past_eof"], differs="bsize_binds")
    a, b = bgzf_member(FQ2), bgzf_member(FQ2.replace(b"TTAG", b"CCAG"))          # the same ISIZE, another CRC-32
    a2 = bgzf_member(FQ2, bsize=len(a) + len(b) - 1)
    assert len(a.payload) == len(b.payload)
    add("bsize_takes_in_the_next_member", [bgzf_member(FQ), a2, b, EOF_BLOCK], FQ, "SAM 4.1: BSIZE = block size - 1", ["bad:bsize_next_member"], differs="bsize_binds")
    add("slack_in_front_of_the_trailer", bg(slack=b"\0\0"), FQ, "2.3: the trailer follows the compressed blocks", ["bad:slack"])
    # ---- bytes behind the last member
    for tag, tail in (("zero1", b"\0"), ("zero17", b"\0" * 17), ("zero18", b"\0" * 18), ("magic", b"\x1f\x8b"), ("text", b"@x\nAC\n+\n!!\nmore text, no gzip\n")):
        add("tail_%s_bgzf" % tag, [bgzf_member(FQ), bgzf_member(FQ2), EOF_BLOCK, tail], FQ + FQ2, "2.2: a file is a series of members", ["bad:tail_%s_bgzf" % tag],
            refused_by_index=True)
        add("tail_%s_plain" % tag, [member(FQ), member(FQ2), tail], FQ + FQ2, "2.2: a file is a series of members", ["bad:tail_%s_plain" % tag], refused_by_index=True)
    return c


_GROUPS = (("cut_plain_at", "cuts_plain"), ("cut_bgzf_at", "cuts_bgzf"), ("hdr", "headers"), ("bc", "headers"), ("big", "big"), ("phase", "phases"),
           ("bad", "headers"), ("crc", "trailers"), ("isize_65537", "framing"), ("isize", "trailers"), ("bsize", "trailers"), ("slack", "trailers"),
           ("tail", "tails"), ("", "framing"))


def groups():
    """the catalogue in groups of up to a hundred-odd cases (a test item each): "valid_..." / "invalid_..." -> [Case]"""
    g = {}
    for c in list(valid().values()) + list(invalid().values()):
        key = next(grp for prefix, grp in _GROUPS if c.name.startswith(prefix))
        g.setdefault(("valid_" if c.valid else "invalid_") + key, []).append(c)
    return g


GROUP_NAMES = ("valid_headers", "valid_framing", "valid_big", "valid_phases", "invalid_headers", "invalid_cuts_plain", "invalid_cuts_bgzf",
               "invalid_trailers", "invalid_tails")
