"""SAM text for the tests (helper, not collected): a WRITER — alignment lines of every shape (mapped, unmapped, `=` and `*`
mates, absent SEQ / QUAL, with and without aux fields, leading zeros, CRLF, an unterminated last line, long reads), a header,
and the same records bam_files.record() packs, as text — and an independent READER that is the oracle of the SAM tests: the
ten columns of read_sam_file_records as INTEGRATION.md states them, rows as tuples, NULL as None, the first error as
(record ordinal, code, byte offset of its line).

Nothing here shares code with the library.  The rules marked [R] are recalled from exon 0.2.x over noodles-sam, which are not
in the reference tree; tests/test_sam_host.py names each of them so that a real exon build can falsify it."""
import random

NAMES = ["name", "flag", "reference", "start", "end", "mapping_quality", "cigar", "mate_reference", "sequence", "quality_score"]
TYPES = ["VARCHAR", "INTEGER", "VARCHAR", "INTEGER", "INTEGER", "VARCHAR", "VARCHAR", "VARCHAR", "VARCHAR", "VARCHAR"]
INT_COLS = (1, 3, 4)
NULLABLE = (2, 3, 4, 5, 7)

# parse errors, numbered like include/exon_gpu.h (EXG_PE_*)
E_INVALID_UTF8 = 4
E_FIELD_COUNT, E_EMPTY_FIELD, E_HEADER_LINE, E_FLAG, E_POSITION, E_MAPQ, E_CIGAR, E_LENGTHS = 35, 36, 37, 38, 39, 40, 41, 42

I31 = (1 << 31) - 1
CIGAR_LEN_MAX = (1 << 28) - 1
REF_OPS, OTHER_OPS = b"MDN=X", b"ISHP"


# ---------------------------------------------------------------- reader (the oracle)
class SamError(Exception):
    def __init__(self, code):
        Exception.__init__(self, code)
        self.code = code


def _number(text, most, code):
    """one or more ASCII digits, no sign and no other byte; at most `most`"""
    if not text:
        raise SamError(E_EMPTY_FIELD)
    if any(not 48 <= c <= 57 for c in text):
        raise SamError(code)
    v = int(text)
    if v > most:
        raise SamError(code)
    return v


def _span(cigar):
    """reference bases of a CIGAR text (not `*`): M, D, N, = and X consume them"""
    span, digits, ops = 0, b"", 0
    for c in cigar:
        ch = bytes([c])
        if ch.isdigit():
            digits += ch
            continue
        if not digits or ch not in (b"M", b"I", b"D", b"N", b"S", b"H", b"P", b"=", b"X") or int(digits) > CIGAR_LEN_MAX:
            raise SamError(E_CIGAR)
        if ch in (b"M", b"D", b"N", b"=", b"X"):
            span += int(digits)
        digits, ops = b"", ops + 1
    if digits or not ops:
        raise SamError(E_CIGAR)
    return span


def parse_line(line):
    """one line (terminator and its CR stripped) -> the row; raises SamError.  The field count first, then the fields left to
    right, UTF-8 last"""
    f = line.split(b"\t")
    if len(f) < 11:
        raise SamError(E_FIELD_COUNT)
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    if not qname:
        raise SamError(E_EMPTY_FIELD)
    if qname[:1] == b"@":
        raise SamError(E_HEADER_LINE)
    flag_v = _number(flag, 65535, E_FLAG)
    if not rname:
        raise SamError(E_EMPTY_FIELD)
    pos_v = _number(pos, I31, E_POSITION)
    mapq_v = _number(mapq, 255, E_MAPQ)
    if not cigar:
        raise SamError(E_EMPTY_FIELD)
    span = 0 if cigar == b"*" else _span(cigar)
    if not rnext or not pnext or not tlen or not seq or not qual:
        raise SamError(E_EMPTY_FIELD)
    if seq != b"*" and qual != b"*" and len(seq) != len(qual):
        raise SamError(E_LENGTHS)
    try:
        line.decode("utf-8")
    except UnicodeDecodeError:
        raise SamError(E_INVALID_UTF8)
    reference = None if rname == b"*" else rname
    start = pos_v if pos_v else None
    end = None
    if start is not None and 1 <= start + span - 1 <= I31:
        end = start + span - 1
    return (qname, flag_v, reference, start, end, None if mapq_v == 255 else b"%d" % mapq_v, b"" if cigar == b"*" else cigar,
            reference if rnext == b"=" else None if rnext == b"*" else rnext, b"" if seq == b"*" else seq, b"" if qual == b"*" else qual)


def lines_of(data, base=0):
    """[(offset, line bytes)]: a line ends at LF, one CR in front of it is stripped; an unterminated last line is a line"""
    out, pos = [], base
    while pos < len(data):
        nl = data.find(b"\n", pos)
        if nl < 0:
            out.append((pos, data[pos:]))
            break
        end = nl - 1 if nl > pos and data[nl - 1:nl] == b"\r" else nl
        out.append((pos, data[pos:end]))
        pos = nl + 1
    return out


def header_end(data):
    """the header: the maximal run of lines at the start whose first byte is '@'"""
    pos = 0
    while pos < len(data) and data[pos:pos + 1] == b"@":
        nl = data.find(b"\n", pos)
        pos = len(data) if nl < 0 else nl + 1
    return pos


def read(data, base=0):
    """alignment lines from data[base:] -> (rows in front of the first failing line, None | (record ordinal, code, byte offset
    of the line in data))"""
    rows = []
    for off, line in lines_of(data, base):
        try:
            rows.append(parse_line(line))
        except SamError as e:
            return rows, (len(rows), e.code, off)
    return rows, None


def read_file(data):
    """a whole file: the header is skipped unread"""
    return read(data, header_end(data))


# ---------------------------------------------------------------- writer
REFS = [(b"chr1", 248956422), (b"chr2", 242193529), (b"chrX", 156040895), (b"chrUn_KI270742v1", 186739)]


def header(refs=REFS, extra=()):
    out = [b"@HD\tVN:1.6\tSO:coordinate\n"] + [b"@SQ\tSN:%s\tLN:%d\n" % r for r in refs] + [b"@PG\tID:writer\tPN:sam_files\n"]
    return b"".join(out + list(extra))


def line(rng, read_len=None, name=None, aux=None):
    """a valid alignment line (no terminator): 60 to 450 bytes unless `read_len` or `name` make it longer"""
    n = rng.choice((0, 1, 10, 36, 100, 150, 151)) if read_len is None else read_len
    qname = name if name is not None else b"A00%03d:%d:HXX:%d:%d:%d" % (rng.randrange(1000), rng.randrange(400), rng.randrange(1, 5),
                                                                      rng.randrange(1101, 2679), rng.randrange(1000, 37000))
    unmapped = rng.random() < 0.1
    ref = b"*" if unmapped else rng.choice(REFS)[0]
    pos = 0 if unmapped else rng.randrange(1, 150_000_000)
    mapq = b"255" if unmapped else rng.choice((b"0", b"1", b"27", b"60", b"007", b"000", b"254"))
    seq = bytes(rng.choice(b"ACGTN") for _ in range(n)) if n else b"*"
    qual = b"*" if (n == 0 or rng.random() < 0.1) else bytes(rng.randrange(33, 127) for _ in range(n))
    if n == 0 and rng.random() < 0.5:
        qual = bytes(rng.randrange(34, 127) for _ in range(rng.choice((1, 2, 30))))   # SEQ absent, QUAL present
    if unmapped or n == 0:
        cigar = b"*"
    else:
        shape = rng.random()
        if shape < 0.6:
            cigar = b"%dM" % n
        elif shape < 0.8 and n > 4:
            k = rng.randrange(1, n - 2)
            cigar = b"%dS%dM" % (k, n - k)
        elif n > 8:
            a = rng.randrange(1, n - 6)
            cigar = b"%dM2D%d=1X3I%dH5P7N" % (a, n - a - 4, rng.randrange(1, 50))
        else:
            cigar = b"%dX" % n
    rnext = rng.choice((b"=", b"*", rng.choice(REFS)[0]))
    f = [qname, b"%d" % rng.randrange(0, 4096), ref, b"%d" % pos, mapq, cigar, rnext, b"%d" % rng.randrange(0, 150_000_000),
         b"%d" % rng.randrange(-500, 500), seq, qual]
    if aux is None:
        aux = rng.random() < 0.6
    if aux:
        f += [b"NM:i:%d" % rng.randrange(5), b"MD:Z:%d" % max(n, 1), b"RG:Z:grp%d" % rng.randrange(4)][:rng.randrange(1, 4)]
        if qual == b"*" and n >= 10:
            # QUAL absent, SEQ present: the first aux field ends exactly len(SEQ) bytes behind QUAL's first byte, at a tab or at the
            # line's end — where a scan that finds QUAL's end by SEQ's length would look
            f[11] = b"XQ:Z:" + b"q" * (n - 7)
            assert len(b"*\t" + f[11]) == n
    return b"\t".join(f)


def mixed(rng, n_lines, crlf_every=0, final_newline=True, **kw):
    out = []
    for i in range(n_lines):
        out.append(line(rng, **kw))
        out.append(b"\r\n" if crlf_every and (i + 1) % crlf_every == 0 else b"\n")
    if not final_newline and out:
        out[-1] = b""
    return b"".join(out)


def fill_to(rng, data, size, **kw):
    """`data` with valid lines appended until it is at least `size` bytes long (ends with LF)"""
    parts, n = [data], len(data)
    while n < size:
        ln = line(rng, **kw) + b"\n"
        parts.append(ln)
        n += len(ln)
    return b"".join(parts)


def from_bam_fields(refs, name=b"r", flag=0, ref=-1, pos=-1, mapq=255, cigar=(), next_ref=-1, next_pos=-1, tlen=0, seq=b"", qual=None,
                    aux_text=()):
    """the arguments of bam_files.record() (refs: the BAM header's [(name, length)]; qual: raw Phred bytes or None) as the line
    `samtools view` prints for that record"""
    rnext = b"*" if next_ref < 0 else b"=" if next_ref == ref else refs[next_ref][0]
    f = [name, b"%d" % flag, refs[ref][0] if ref >= 0 else b"*", b"%d" % (pos + 1), b"%d" % mapq,
         b"".join(b"%d%s" % (ln, op.encode() if isinstance(op, str) else op) for ln, op in cigar) or b"*", rnext, b"%d" % (next_pos + 1),
         b"%d" % tlen, seq or b"*", b"*" if qual is None or not seq else bytes(q + 33 for q in qual)]
    return b"\t".join(f + list(aux_text))


def rng(seed):
    return random.Random(seed)
