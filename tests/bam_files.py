"""BAM files for the tests (helper, not collected): a WRITER that builds headers, records and BGZF members by hand — members
cut at any decoded offset (mid-record, mid-block_size), stored blocks, empty members, a pre-compressed run of members
repeated N times for large files — and an independent READER (gzip + struct) that is the oracle of the BAM tests: the ten
columns of read_bam_file_records as INTEGRATION.md states them, rows as tuples, NULL as None.

SAM v1 section 4.2 is the format; nothing here shares code with the library."""
import gzip
import struct
import zlib

CIGAR_OPS = b"MIDNSHP=X"
SEQ_CODES = b"=ACMGRSVTWYHKDBN"
_SEQ_INDEX = {c: i for i, c in enumerate(SEQ_CODES)}

# record errors, numbered like include/exon_gpu.h (EXG_PE_BAM_*)
E_BLOCK_SIZE, E_TRUNCATED, E_READ_NAME, E_REFERENCE_ID, E_FIELD_LENGTHS, E_CIGAR_OP, E_QUALITY = 15, 16, 17, 18, 19, 20, 21


# ---------------------------------------------------------------- writer
def header(refs=(), text=b""):
    """refs: [(name bytes, length)]"""
    out = [b"BAM\1", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, length in refs:
        out += [struct.pack("<i", len(name) + 1), name, b"\0", struct.pack("<i", length)]
    return b"".join(out)


def pack_seq(seq):
    codes = [_SEQ_INDEX[c] for c in seq]
    if len(codes) & 1:
        codes.append(0)
    return bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))


def _op(op):
    if isinstance(op, int):
        return op
    return CIGAR_OPS.index(op.encode() if isinstance(op, str) else op)


def record(name=b"r", flag=0, ref=-1, pos=-1, mapq=255, cigar=(), next_ref=-1, next_pos=-1, tlen=0, seq=b"", qual=None, aux=b"",
           bin_=0, l_read_name=None, l_seq=None, n_cigar=None, block_size=None, raw_name=None, raw_cigar=None):
    """One alignment record.  cigar: [(length, op)] with op a character of MIDNSHP=X or a number; qual: raw Phred bytes (None =
    absent, 0xFF).  The trailing keyword arguments overwrite single fields with lies (the error tests)."""
    name_bytes = raw_name if raw_name is not None else name + b"\0"
    cig = raw_cigar if raw_cigar is not None else b"".join(struct.pack("<I", (ln << 4) | _op(op)) for ln, op in cigar)
    n_ops = len(cig) // 4
    if qual is None:
        qual = b"\xff" * len(seq)
    body = b"".join([
        struct.pack("<iiBBHHHiiii", ref, pos, len(name_bytes) if l_read_name is None else l_read_name, mapq, bin_,
                    n_ops if n_cigar is None else n_cigar, flag, len(seq) if l_seq is None else l_seq, next_ref, next_pos, tlen),
        name_bytes, cig, pack_seq(seq), qual, aux])
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def aux_z(tag, value):
    return tag + b"Z" + value + b"\0"


def aux_b_u8(tag, values):
    return tag + b"BC" + struct.pack("<i", len(values)) + bytes(values)


def bgzf_member(data, level=6, stored=False):
    assert len(data) <= 0xFFFF
    if stored:
        deflated = b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data
    else:
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        deflated = c.compress(data) + c.flush()
    bsize = 12 + 6 + len(deflated) + 8 - 1
    assert bsize <= 0xFFFF, "member too large: cut it smaller"
    return (b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize) + deflated +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


BGZF_EOF = bgzf_member(b"")


def bgzf(data, cuts=None, member_bytes=0xFF00, level=6, stored=False, eof=True):
    """data as BGZF members that end at the decoded offsets `cuts` (sorted; pieces longer than member_bytes are cut
    further), or every member_bytes."""
    edges = sorted(set([0, len(data)] + [c for c in (cuts or []) if 0 < c < len(data)]))
    out = []
    for lo, hi in zip(edges, edges[1:]):
        for s in range(lo, hi, member_bytes):
            out.append(bgzf_member(data[s:min(hi, s + member_bytes)], level, stored or level == 0))
    if eof:
        out.append(BGZF_EOF)
    return b"".join(out)


def write_repeated(path, head, run, n, level=1, member_bytes=0xFF00):
    """A large file cheaply: the members of `head` (header + whatever) once, then the members of `run` — whole records —
    compressed once and written n times, then the EOF member.  -> decoded size"""
    h = bgzf(head, eof=False, level=level, member_bytes=member_bytes)
    m = bgzf(run, eof=False, level=level, member_bytes=member_bytes)
    with open(path, "wb") as f:
        f.write(h)
        for _ in range(n):
            f.write(m)
        f.write(BGZF_EOF)
    return len(head) + n * len(run)


# ---------------------------------------------------------------- reader (the oracle)
class Parsed:
    def __init__(self):
        self.refs, self.rows, self.error, self.data_offset = [], [], None, 0


def _digits(n):
    return str(n).encode()


def parse_decoded(raw):
    """decoded bytes of a BAM file -> Parsed: refs [(name, length)], rows (tuples of the ten columns), error = None or
    (record ordinal, E_*) for the first bad record (rows holds the records in front of it)."""
    out = Parsed()
    if raw[:4] != b"BAM\1":
        raise ValueError("not a BAM file")
    l_text, = struct.unpack_from("<i", raw, 4)
    pos = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, pos)
    pos += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, pos)
        name = raw[pos + 4:pos + 4 + l_name - 1]
        length, = struct.unpack_from("<i", raw, pos + 4 + l_name)
        out.refs.append((name, length))
        pos += 8 + l_name
    out.data_offset = pos
    n = len(raw)
    ordinal = 0

    def ref_name(i):
        return None if i < 0 else out.refs[i][0]

    while pos < n:
        def bad(code):
            out.error = (ordinal, code)
            return out
        if pos + 4 > n:
            return bad(E_TRUNCATED)
        bs, = struct.unpack_from("<I", raw, pos)
        if bs < 32:
            return bad(E_BLOCK_SIZE)
        if pos + 4 + bs > n:
            return bad(E_TRUNCATED)
        ref, p, l_name, mapq, _bin, n_cig, flag, l_seq, nref, _npos, _tlen = struct.unpack_from("<iiBBHHHiiii", raw, pos + 4)
        if l_name == 0:
            return bad(E_READ_NAME)
        if l_seq < 0 or 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
            return bad(E_FIELD_LENGTHS)
        q = pos + 36
        if raw[q + l_name - 1] != 0:
            return bad(E_READ_NAME)
        if not (-1 <= ref < n_ref and -1 <= nref < n_ref):
            return bad(E_REFERENCE_ID)
        name = raw[q:q + l_name - 1]
        q += l_name
        ops = struct.unpack_from("<%dI" % n_cig, raw, q)
        q += 4 * n_cig
        if any((w & 15) > 8 for w in ops):
            return bad(E_CIGAR_OP)
        cigar = b"".join(_digits(w >> 4) + CIGAR_OPS[w & 15:(w & 15) + 1] for w in ops)
        span = sum(w >> 4 for w in ops if (w & 15) in (0, 2, 3, 7, 8))
        packed = raw[q:q + (l_seq + 1) // 2]
        q += (l_seq + 1) // 2
        seq = bytes(SEQ_CODES[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq)) if l_seq < 64 else \
            packed.hex().encode().translate(bytes.maketrans(b"0123456789abcdef", SEQ_CODES))[:l_seq]
        qual = raw[q:q + l_seq]
        if qual == b"\xff" * l_seq:
            quality = b""
        else:
            if max(qual) > 93:
                return bad(E_QUALITY)
            quality = qual.translate(_PLUS33)
        start = p + 1 if p >= 0 else None
        end = None
        if start is not None:
            e = start + span - 1
            end = e if 1 <= e <= 0x7FFFFFFF else None
        out.rows.append((name, flag, ref_name(ref), start, end, None if mapq == 255 else _digits(mapq), cigar, ref_name(nref), seq, quality))
        ordinal += 1
        pos += 4 + bs
    return out


_PLUS33 = bytes((i + 33) & 0xFF for i in range(256))


def parse(path):
    with open(path, "rb") as f:
        return parse_decoded(gzip.decompress(f.read()))


NAMES = ["name", "flag", "reference", "start", "end", "mapping_quality", "cigar", "mate_reference", "sequence", "quality_score"]
TYPES = ["VARCHAR", "INTEGER", "VARCHAR", "INTEGER", "INTEGER", "VARCHAR", "VARCHAR", "VARCHAR", "VARCHAR", "VARCHAR"]


# ---------------------------------------------------------------- generators
def illumina_pairs(n_pairs, refs, seed=1, read_len=150, aux=True):
    """2 * n_pairs records of paired 150 bp reads, as a short-read aligner writes them: names of an instrument run, 150M (a
    few with indels / soft clips), mapq 0..60, an unmapped pair now and then, NM / MD / RG aux fields.  -> list of records"""
    import random
    rng = random.Random(seed)
    out = []
    for i in range(n_pairs):
        name = b"A00%03d:%d:HXXXXXX:%d:%d:%d:%d" % (rng.randrange(1000), rng.randrange(400), rng.randrange(1, 5), rng.randrange(1101, 2679),
                                                  rng.randrange(1000, 32000), rng.randrange(1000, 37000))
        unmapped = rng.random() < 0.02
        ref = -1 if unmapped else rng.randrange(len(refs))
        pos = -1 if unmapped else rng.randrange(0, 200_000_000)
        for mate in (0, 1):
            seq = rng.randbytes(read_len).translate(_TO_BASES)
            qual = rng.randbytes(read_len).translate(_TO_QUAL)
            shape = rng.random()
            if unmapped:
                cigar = ()
            elif shape < 0.9:
                cigar = ((read_len, "M"),)
            elif shape < 0.95:
                k = rng.randrange(1, 40)
                cigar = ((k, "S"), (read_len - k, "M"))
            else:
                a = rng.randrange(10, 100)
                cigar = ((a, "M"), (2, "D"), (read_len - a - 3, "M"), (3, "I"))
            flag = (0x1 | (0x40 if mate == 0 else 0x80) | (0xC if unmapped else 0x2) | (0x10 if rng.random() < 0.5 and not unmapped else 0))
            extra = b""
            if aux:
                extra = b"NMC" + bytes([rng.randrange(5)]) + aux_z(b"MD", b"%d" % read_len) + aux_z(b"RG", b"grp%d" % rng.randrange(4))
            out.append(record(name, flag, ref, pos + mate * 200 if pos >= 0 else -1, 255 if unmapped else rng.choice((0, 1, 27, 40, 60)), cigar, ref,
                              pos + (1 - mate) * 200 if pos >= 0 else -1, 0 if unmapped else (350 if mate == 0 else -350), seq, qual, extra))
    return out


_TO_BASES = bytes(b"ACGT"[i & 3] for i in range(256))
_TO_QUAL = bytes(2 + i % 40 for i in range(256))
