"""BGZF + tabix for the region tests (helper, not collected): an independent Python implementation that is the ORACLE of
vcf_query — a bgzip writer with a chosen amount of text per member, a tabix index writer and reader, the region grammar and the
chunk planner of exg_tabix.hpp, the mapping from chunks to member ranges, the row rule of exg_vcf_region.hpp and a brute-force
rows_in_region.  Nothing here shares code with the library; only zlib is used, for the raw DEFLATE streams.

The index writer follows the tabix paper's scheme (min_shift 14, depth 5) the way htslib does: a record goes to the smallest bin
that holds [beg, end), consecutive records of one bin extend its last chunk, the linear index keeps the smallest virtual offset of
the records that overlap each 16 KiB window and an empty window takes the offset of the next one, and every reference carries the
metadata pseudo-bin 37450."""
import random
import struct
import zlib

PSEUDO_BIN = 37450
MAX_POS = 1 << 29
UNBOUNDED = (1 << 63) - 1
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


# ---- BGZF ---------------------------------------------------------------------------------------------------------------
def bgzf_member(data):
    assert len(data) <= 65536
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    if len(body) + 26 > 65536:  # (incompressible: stored blocks)
        c = zlib.compressobj(0, zlib.DEFLATED, -15)
        body = c.compress(data) + c.flush()
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25)
    return head + body + struct.pack("<II", zlib.crc32(data), len(data))


def bgzip(text, member_bytes, eof=True, cuts=()):
    """-> (file bytes, [(compressed offset, text offset, text length)] of the data members): `member_bytes` of text a member, cut
    wherever that falls (lines straddle the seams); cuts: text offsets at which a new member begins whatever the size says"""
    out, members, pos = bytearray(), [], 0
    while pos < len(text):
        stop = min([pos + member_bytes] + [c for c in cuts if c > pos])
        piece = text[pos:stop]
        members.append((len(out), pos, len(piece)))
        out += bgzf_member(piece)
        pos += len(piece)
    if eof:
        out += EOF_MEMBER
    return bytes(out), members


def bgunzip(data):
    """the inflated bytes of a BGZF file, member by member (every size and CRC checked)"""
    out, pos = bytearray(), 0
    while pos < len(data):
        assert data[pos:pos + 4] == b"\x1f\x8b\x08\x04" and data[pos + 12:pos + 14] == b"BC"
        xlen, = struct.unpack_from("<H", data, pos + 10)
        bsize, = struct.unpack_from("<H", data, pos + 16)
        end = pos + bsize + 1
        piece = zlib.decompress(data[pos + 12 + xlen:end - 8], -15)
        crc, isize = struct.unpack_from("<II", data, end - 8)
        assert zlib.crc32(piece) == crc and len(piece) == isize
        out += piece
        pos = end
    return bytes(out)


def member_offsets(data):
    """[(compressed offset, inflated size)] of every member of a BGZF file"""
    out, pos = [], 0
    while pos < len(data):
        bsize, = struct.unpack_from("<H", data, pos + 16)
        isize, = struct.unpack_from("<I", data, pos + bsize + 1 - 4)
        out.append((pos, isize))
        pos += bsize + 1
    return out


def voffset_of(members, text_off):
    """the virtual offset of byte text_off of the text (the member that holds it; the end of the text: behind the last member)"""
    for c, t0, n in members:
        if t0 <= text_off < t0 + n:
            return (c << 16) | (text_off - t0)
    c, t0, n = members[-1]
    assert text_off == t0 + n
    return (c << 16) | n


# ---- the row rule -------------------------------------------------------------------------------------------------------
def info_end(info):
    """the integer of the first END key of an INFO text, or None (absent, or counts as absent)"""
    for item in info.split(b";"):
        if item == b"END" or item.startswith(b"END="):
            v = item[4:]
            return int(v) if item != b"END" and v.isdigit() and len(v) <= 18 and v.isascii() else None
    return None


def row_end(pos, ref, info):
    e = info_end(info)
    return e if e is not None else pos + len(ref) - 1


def keeps(chrom, pos, ref, info, name, start, end):
    if chrom != name or pos > end:
        return False
    if pos >= start:
        return True
    return row_end(pos, ref, info) >= start


def data_lines(text):
    """[(text offset, line without its newline)] of the lines that are not header lines"""
    out, pos = [], 0
    for line in text.split(b"\n"):
        if line and not line.startswith(b"#"):
            out.append((pos, line))
        pos += len(line) + 1
    return out


def fields_of(line):
    f = line.split(b"\t")
    return f[0], int(f[1]), f[3], f[7]


def rows_in_region(rows, region):
    """brute force: the rows [(chrom, pos, ref, info, ...)] a region (name, start, end) keeps"""
    name, start, end = region
    return [r for r in rows if keeps(r[0], r[1], r[2], r[3], name, start, end)]


# ---- the index ----------------------------------------------------------------------------------------------------------
def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


def build_index(text, members):
    """the index of VCF text cut into `members` (bgzip's list): {names, refs: [{bins: {bin: [(beg, end)]}, ioff: [...]}]}"""
    names, refs = [], []
    lines = data_lines(text)
    for k, (off, line) in enumerate(lines):
        chrom, pos, ref, info = fields_of(line)
        if chrom not in names:
            names.append(chrom)
            refs.append({"bins": {}, "ioff": [], "n": 0, "lo": None, "hi": 0})
        r = refs[names.index(chrom)]
        beg, end = pos - 1, max(row_end(pos, ref, info), pos)
        v0 = voffset_of(members, off)
        nxt = off + len(line) + 1
        v1 = voffset_of(members, min(nxt, len(text)))
        b = reg2bin(beg, end)
        chunks = r["bins"].setdefault(b, [])
        if chunks and chunks[-1][1] == v0 and r.get("last_bin") == b:
            chunks[-1] = (chunks[-1][0], v1)
        else:
            chunks.append((v0, v1))
        r["last_bin"] = b
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            while len(r["ioff"]) <= w:
                r["ioff"].append(None)
            if r["ioff"][w] is None:
                r["ioff"][w] = v0
        r["n"] += 1
        r["lo"] = v0 if r["lo"] is None else r["lo"]
        r["hi"] = v1
    for r in refs:
        for w in range(len(r["ioff"]) - 2, -1, -1):
            if r["ioff"][w] is None:
                r["ioff"][w] = r["ioff"][w + 1]
        r.pop("last_bin", None)
    return {"names": names, "refs": refs}


def serialize_index(idx, n_no_coor=0, fmt=2):
    names = b"".join(n + b"\0" for n in idx["names"])
    out = bytearray(b"TBI\1" + struct.pack("<8i", len(idx["names"]), fmt, 1, 2, 0, ord("#"), 0, len(names)) + names)
    for r in idx["refs"]:
        out += struct.pack("<i", len(r["bins"]) + 1)
        for b in sorted(r["bins"]):
            out += struct.pack("<Ii", b, len(r["bins"][b]))
            for c in r["bins"][b]:
                out += struct.pack("<QQ", *c)
        out += struct.pack("<Ii", PSEUDO_BIN, 2) + struct.pack("<QQQQ", r["lo"] or 0, r["hi"], r["n"], 0)
        out += struct.pack("<i", len(r["ioff"])) + b"".join(struct.pack("<Q", v) for v in r["ioff"])
    if n_no_coor is not None:
        out += struct.pack("<Q", n_no_coor)
    return bytes(out)


def read_index(d):
    """the inflated bytes of a .tbi -> the same shape build_index makes (the pseudo-bin kept apart, under "meta")"""
    assert d[:4] == b"TBI\1"
    n_ref, fmt, col_seq, col_beg, col_end, meta, skip, l_nm = struct.unpack_from("<8i", d, 4)
    names = d[36:36 + l_nm].split(b"\0")[:-1]
    assert len(names) == n_ref
    p, refs = 36 + l_nm, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", d, p)
        p += 4
        r = {"bins": {}, "ioff": [], "meta": None}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", d, p)
            p += 8
            chunks = [struct.unpack_from("<QQ", d, p + 16 * k) for k in range(n_chunk)]
            p += 16 * n_chunk
            if b == PSEUDO_BIN:
                r["meta"] = chunks
            else:
                r["bins"][b] = chunks
        n_intv, = struct.unpack_from("<i", d, p)
        r["ioff"] = list(struct.unpack_from("<%dQ" % n_intv, d, p + 4))
        p += 4 + 8 * n_intv
        refs.append(r)
    assert len(d) - p in (0, 8)
    return {"names": names, "refs": refs, "format": fmt, "n_no_coor": struct.unpack_from("<Q", d, p)[0] if len(d) - p == 8 else None}


# ---- the region grammar and the planner -----------------------------------------------------------------------------------
class RegionError(ValueError):
    pass


def _interval(s):
    a, dash, b = s.partition(b"-")
    ok = lambda t: t.isdigit() and t.isascii() and len(t) <= 18  # noqa: E731
    if not ok(a) or int(a) < 1:
        return None
    if not dash:
        return int(a), UNBOUNDED
    return (int(a), int(b)) if ok(b) and int(b) >= int(a) else None


def parse_region(names, text):
    """-> (name, start, end), 1-based closed; RegionError for the empty string or a name the index does not hold"""
    if not text:
        raise RegionError(text)
    if text in names:
        return text, 1, UNBOUNDED
    head, colon, tail = text.rpartition(b":")
    iv = _interval(tail) if colon else None
    if iv and head in names:
        return head, iv[0], iv[1]
    raise RegionError(text)


def plan(idx, region):
    """the chunks (begin, end) to read for (name, start, end): collected from reg2bins, cut by the linear index, sorted, merged when
    next.begin <= cur.end"""
    name, start, end = region
    r = idx["refs"][idx["names"].index(name)]
    beg = min(start - 1, MAX_POS - 1)
    e = max(min(end, MAX_POS), beg + 1)
    ioff = r["ioff"]
    min_off = ioff[min(beg >> 14, len(ioff) - 1)] if ioff else 0
    chunks = sorted(c for b in set(reg2bins(beg, e)) if b != PSEUDO_BIN for c in r["bins"].get(b, []) if c[1] > min_off)
    out = []
    for c in chunks:
        if out and c[0] <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], c[1]))
        else:
            out.append(c)
    return out


def member_ranges(chunks, offsets):
    """chunks -> [(first member, one past the last member, skip)] as indices into `offsets` (member_offsets of the file): a chunk
    covers the members from begin >> 16 through end >> 16, the last only when end & 0xFFFF > 0; overlapping or adjacent ranges merge"""
    where = {c: i for i, (c, _) in enumerate(offsets)}  # (an end at the end of the file: behind the last member)
    out = []
    for b, e in chunks:
        first, last = where[b >> 16], where.get(e >> 16, len(offsets))
        if e & 0xFFFF:
            last += 1
        if out and first <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], last), out[-1][2])
        elif last > first:
            out.append((first, last, b & 0xFFFF))
    return out


def header_members(text, members):
    """the leading members a reader inflates, one at a time, until a line that is not a header line begins inside them"""
    end = 0
    for line in text.split(b"\n"):
        if not line.startswith(b"#"):
            break
        end += len(line) + 1
    for i, (_, t0, n) in enumerate(members):
        if end < t0 + n:
            return i + 1
    return len(members)


# ---- VCF text -------------------------------------------------------------------------------------------------------------
HEADER = (b"##fileformat=VCFv4.2\n##contig=<ID=1>\n##contig=<ID=10>\n##contig=<ID=chrX:1>\n"
          b'##INFO=<ID=DP,Number=1,Type=Integer,Description="d">\n##INFO=<ID=END,Number=1,Type=Integer,Description="e">\n'
          b'##INFO=<ID=SVEND,Number=1,Type=Integer,Description="s">\n##INFO=<ID=SVTYPE,Number=1,Type=String,Description="t">\n'
          b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")


def vcf_line(chrom, pos, ref=b"A", alt=b"C", qual=b"30", info=b"DP=7", ident=b"."):
    return b"\t".join([chrom, str(pos).encode(), ident, ref, alt, qual, b"PASS", info]) + b"\n"


def synth_vcf(seed, n_lines=2000, contigs=(b"1", b"10", b"chrX:1"), span=1 << 20, sv=True):
    """sorted VCF text: per contig positions spread over `span`, with deletions, END= records, SVEND decoys, and — sv — one long
    early structural variant per contig (a high-level bin far from the local chunks)"""
    rng = random.Random(seed)
    out = [HEADER]
    per = n_lines // len(contigs)
    for chrom in contigs:
        positions = sorted(rng.randrange(1, span) for _ in range(per))
        if sv:
            positions[0] = min(positions[0], 50)
        for k, pos in enumerate(positions):
            roll = rng.random()
            if sv and k == 0:
                out.append(vcf_line(chrom, pos, alt=b"<DEL>", info=b"SVTYPE=DEL;END=%d" % (pos + span * 3 // 4)))
            elif roll < 0.05:
                out.append(vcf_line(chrom, pos, ref=b"A" + b"CGT" * rng.randrange(1, 120), alt=b"A"))
            elif roll < 0.10:
                out.append(vcf_line(chrom, pos, alt=b"<DEL>", info=b"DP=3;END=%d" % (pos + rng.randrange(1, 40000))))
            elif roll < 0.13:
                out.append(vcf_line(chrom, pos, info=b"SVEND=%d;DP=1" % (pos + 100000)))
            elif roll < 0.15:
                out.append(vcf_line(chrom, pos, info=rng.choice([b"END", b"END=.", b"DP=2;END", b"."])))
            else:
                out.append(vcf_line(chrom, pos, qual=str(rng.randrange(1, 99)).encode(), info=b"DP=%d" % rng.randrange(1, 500)))
    return b"".join(out)


def write_indexed(path, text, member_bytes, cuts=()):
    """text -> path (BGZF) + path.tbi; -> (members, idx)"""
    data, members = bgzip(text, member_bytes, cuts=cuts)
    idx = build_index(text, members)
    with open(path, "wb") as f:
        f.write(data)
    with open(path + ".tbi", "wb") as f:
        f.write(bgzip(serialize_index(idx), 65280)[0])
    return members, idx


def rows_of(text):
    """[(chrom, pos, ref, info, line)] of the data lines"""
    return [fields_of(line) + (line,) for _, line in data_lines(text)]


def random_regions(rng, idx, n, span=1 << 20):
    out = []
    for _ in range(n):
        name = rng.choice(idx["names"])
        kind = rng.random()
        if kind < 0.1:
            out.append((name, 1, UNBOUNDED))
        elif kind < 0.3:  # at 16 384-bp boundaries
            k = rng.randrange(0, span >> 14)
            s = 16384 * k + rng.choice([0, 1]) or 1
            out.append((name, s, s + rng.choice([0, 1, 16383, 16384, 40000])))
        elif kind < 0.4:  # behind the last linear window
            out.append((name, span + rng.randrange(1, 1 << 20), UNBOUNDED))
        else:
            s = rng.randrange(1, span)
            out.append((name, s, s + rng.randrange(0, 60000)))
    return out


def region_text(region):
    name, start, end = region
    if (start, end) == (1, UNBOUNDED):
        return name
    return name + b":%d" % start + (b"" if end == UNBOUNDED else b"-%d" % end)


SPREAD_MEMBER_BYTES = 1024


def spread_file(windows=64, per_window=40):
    """-> (text, members, idx, a one-window region): one contig, `per_window` records in each of `windows` 16 KiB windows, 1 KiB of
    text a member — far more than 64 data members, of which a one-window region needs a handful"""
    rng = random.Random(64)
    lines = [HEADER]
    for w in range(windows):
        for pos in sorted(rng.sample(range(16384 * w + 1, 16384 * (w + 1) + 1), per_window)):
            lines.append(vcf_line(b"1", pos, info=b"DP=%d" % rng.randrange(1, 99)))
    text = b"".join(lines)
    _, members = bgzip(text, SPREAD_MEMBER_BYTES)
    return text, members, build_index(text, members), (b"1", 16384 * 30 + 1, 16384 * 31)


def build_index_snps(chrom, positions, line_offsets, text_len, members):
    """build_index for one contig of single-base records, vectorised (tools/region_bench.py: millions of lines): positions and
    line_offsets are numpy int64 arrays in file order, members bgzip's list for members of one text size"""
    import numpy as np
    t0 = np.array([m[1] for m in members], np.int64)
    c0 = np.array([m[0] for m in members], np.int64)
    size = np.array([m[2] for m in members], np.int64)

    def voff(off):
        k = np.minimum(np.searchsorted(t0, off, side="right") - 1, len(members) - 1)
        k = np.where(off >= t0[k] + size[k], len(members) - 1, k)      # (the end of the text: behind the last member)
        return (c0[k] << 16) | (off - t0[k])
    v0 = voff(line_offsets)
    v1 = voff(np.append(line_offsets[1:], text_len))
    win = (positions - 1) >> 14
    first = np.flatnonzero(np.append(True, win[1:] != win[:-1]))          # runs of one window = runs of one bin (level 5)
    last = np.append(first[1:] - 1, len(win) - 1)
    bins = {}
    for w, a, b in zip(win[first].tolist(), v0[first].tolist(), v1[last].tolist()):
        bins.setdefault(4681 + w, []).append((a, b))
    ioff = [None] * (int(win[-1]) + 1)
    for w, a in zip(win[first].tolist(), v0[first].tolist()):
        if ioff[w] is None:
            ioff[w] = a
    for w in range(len(ioff) - 2, -1, -1):
        if ioff[w] is None:
            ioff[w] = ioff[w + 1]
    return {"names": [chrom], "refs": [{"bins": bins, "ioff": ioff, "n": len(positions), "lo": int(v0[0]), "hi": int(v1[-1])}]}
