"""GTF text for the tests (helper, not collected): an independent READER that is the oracle of the GTF tests — the nine columns
of read_gtf as INTEGRATION.md states them, rows as tuples, NULL as None, `attributes` as the list of (key, value) pairs in file
order, the first error as (row ordinal among ALL lines, code, byte offset of its line) — and a WRITER of Ensembl-shaped lines.

Nothing here shares code with the library.  Only the fixture row and the count 77 are the reference's
(test_gtf_scan.test:6-22); every other rule is INTEGRATION.md's, [RECALLED] or [DECIDED] there, and tests/test_gtf_host.py names
each of them.

The scan numbers rows by lines, so read() returns, beside the rows of the feature lines, `keep`: one bool per line in front of
the first failing one (False: a `#` line).  score is a float32: its value comes from the C library's strtof through ctypes (not
from a double that is cast), behind a check of the literal's grammar, and is carried as the float's bit pattern."""
import ctypes
import ctypes.util
import random
import re
import struct

NAMES = ["seqname", "source", "type", "start", "end", "score", "strand", "frame", "attributes"]
TYPES = ["VARCHAR", "VARCHAR", "VARCHAR", "BIGINT", "BIGINT", "FLOAT", "VARCHAR", "VARCHAR", "MAP(VARCHAR, VARCHAR)"]
NULLABLE = (5, 6, 7)

# parse errors, numbered like include/exon_gpu.h (EXG_PE_*)
E_INVALID_UTF8 = 4
E_FIELD_COUNT, E_EMPTY_FIELD, E_POSITION, E_SCORE, E_STRAND, E_FRAME, E_ATTRIBUTES = 57, 58, 59, 60, 61, 62, 63

I63 = (1 << 63) - 1

_libc = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6")
_libc.strtof.restype = ctypes.c_float
_libc.strtof.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p)]
# f32::from_str: [+-] (digits [. digits*] | . digits) [e [+-] digits] | inf | infinity | nan, any case
_FLOAT = re.compile(rb"[+-]?(?:(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|[iI][nN][fF](?:[iI][nN][iI][tT][yY])?|[nN][aA][nN])\Z")


class GtfError(Exception):
    def __init__(self, code, offset=None):
        Exception.__init__(self, code, offset)
        self.code, self.offset = code, offset


def f32_bits(text):
    """the bit pattern of the float32 nearest to the literal (round to nearest even), or None when it is not one"""
    if not _FLOAT.match(text):
        return None
    bits = struct.unpack("<I", struct.pack("<f", _libc.strtof(text, None)))[0]
    if (bits & 0x7FFFFFFF) > 0x7F800000:          # nan: one quiet NaN, no sign
        return 0x7FC00000
    return bits


def bits_f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def parse_attributes(s):
    """the ninth field -> [(key, value)] in file order; raises GtfError(E_ATTRIBUTES, offset) where a left-to-right parser stops.
    Entries are separated by `;`; blank segments are skipped; an entry is `key SP+ value`; a value is `"..."` (any byte but `"`
    inside) or a run of bytes that are neither space, `;` nor `"`; a `"` stands nowhere but around a value."""
    i, n, out = 0, len(s), []
    while True:
        while i < n and s[i] in b" ;":
            i += 1
        if i >= n:
            return out
        k0 = i
        while i < n and s[i] not in b' ;"':
            i += 1
        if i < n and s[i] == 0x22:                      # a quote in (or in front of) a key
            raise GtfError(E_ATTRIBUTES, i)
        key = s[k0:i]
        while i < n and s[i] == 0x20:
            i += 1
        if i >= n or s[i] == 0x3B:                      # an entry without a value
            raise GtfError(E_ATTRIBUTES, i)
        if s[i] == 0x22:
            j = s.find(b'"', i + 1)
            if j < 0:                                   # an unterminated quote: where it opens
                raise GtfError(E_ATTRIBUTES, i)
            value, i = s[i + 1:j], j + 1
            if i < n and s[i] not in b" ;":             # bytes behind the closing quote
                raise GtfError(E_ATTRIBUTES, i)
        else:
            v0 = i
            while i < n and s[i] not in b' ;"':
                i += 1
            if i < n and s[i] == 0x22:                  # a quote inside an unquoted value
                raise GtfError(E_ATTRIBUTES, i)
            value = s[v0:i]
        out.append((key, value))
        while i < n and s[i] == 0x20:
            i += 1
        if i < n and s[i] != 0x3B:                      # a third token in the entry
            raise GtfError(E_ATTRIBUTES, i)


def _position(text):
    if not text or any(not 48 <= c <= 57 for c in text):
        raise GtfError(E_POSITION)
    v = int(text)
    if not 1 <= v <= I63:
        raise GtfError(E_POSITION)
    return v


def parse_line(line, attributes=True):
    """one line (terminator and its CR stripped) -> the row, or None for a `#` line; raises GtfError.  The field count first,
    then the fields left to right, UTF-8 behind them, the attributes' grammar last (attributes=False: the raw ninth field)"""
    if line[:1] == b"#":
        try:
            line.decode("utf-8")
        except UnicodeDecodeError:
            raise GtfError(E_INVALID_UTF8)
        return None
    f = line.split(b"\t", 8)
    if len(f) < 9:
        raise GtfError(E_FIELD_COUNT)
    seqname, source, typ, start, end, score, strand, frame, attrs = f
    if not seqname or not typ:
        raise GtfError(E_EMPTY_FIELD)
    start_v, end_v = _position(start), _position(end)
    score_v = None
    if score != b".":
        score_v = f32_bits(score)
        if score_v is None:
            raise GtfError(E_SCORE)
    if strand not in (b"+", b"-", b"?", b"."):
        raise GtfError(E_STRAND)
    if frame not in (b"0", b"1", b"2", b"."):
        raise GtfError(E_FRAME)
    try:
        line.decode("utf-8")
    except UnicodeDecodeError:
        raise GtfError(E_INVALID_UTF8)
    return (seqname, source, typ, start_v, end_v, score_v, None if strand == b"." else strand, None if frame == b"." else frame,
            parse_attributes(attrs) if attributes else attrs)


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


def read(data, attributes=True):
    """-> (rows of the feature lines in front of the first failing line, keep = [line is a feature] for the lines in front of
    it, None | (ordinal of the failing line among all lines, code, byte offset of the line, offset in its ninth field or None))"""
    rows, keep = [], []
    for off, line in lines_of(data):
        try:
            row = parse_line(line, attributes)
        except GtfError as e:
            return rows, keep, (len(keep), e.code, off, e.offset)
        keep.append(row is not None)
        if row is not None:
            rows.append(row)
    return rows, keep, None


def user_row(row):
    """a row as the reader hands it out: score as a Python float"""
    return row[:5] + (None if row[5] is None else bits_f32(row[5]),) + row[6:]


# ---------------------------------------------------------------- writer
SEQNAMES = [b"chr1", b"chr2", b"chrX", b"KI270742.1", b"1"]
SOURCES = [b"ensembl_havana", b"havana", b"processed_transcript", b"."]
FEATURES = [b"gene", b"transcript", b"exon", b"CDS", b"start_codon", b"five_prime_utr"]
SCORES = [b".", b".", b".", b"0", b"1000", b"0.5", b"13.25", b"-1.5e-3", b"1e10", b"7.", b".5", b"+3", b"inf"]


def attributes(rng, n_entries=None, tags=None):
    """Ensembl / GENCODE shaped: quoted ids, an unquoted exon_number or level, repeated `tag` keys, `;` and spaces inside quotes"""
    n = rng.randrange(2, 9) if n_entries is None else n_entries
    ent = [b'gene_id "ENSG%011d"' % rng.randrange(10 ** 9), b'transcript_id "ENST%011d"' % rng.randrange(10 ** 9),
           b"exon_number %d" % rng.randrange(1, 40), b'gene_name "%s"' % rng.choice((b"DDX11L1", b"WASH7P", b"MIR1302-11", b"A")),
           b'gene_biotype "%s"' % rng.choice((b"pseudogene", b"protein_coding", b"lincRNA")), b"level %d" % rng.randrange(1, 4),
           b'note "5; prime end, see Ensembl"', b'empty ""'][:n]
    for _ in range(rng.randrange(0, 3) if tags is None else tags):
        ent.append(b'tag "%s"' % rng.choice((b"basic", b"CCDS", b"appris_principal_1")))
    sep = rng.choice((b"; ", b";", b";  "))
    return sep.join(ent) + rng.choice((b";", b"", b"; ", b" ;"))


def line(rng, attrs=None, seqname=None):
    start = rng.randrange(1, 248_000_000)
    f = [seqname if seqname is not None else rng.choice(SEQNAMES), rng.choice(SOURCES), rng.choice(FEATURES), b"%d" % start,
         b"%d" % (start + rng.randrange(0, 100_000)), rng.choice(SCORES), rng.choice((b"+", b"-", b".", b"?")), rng.choice((b".", b"0", b"1", b"2")),
         attributes(rng) if attrs is None else attrs]
    return b"\t".join(f)


def mixed(rng, n_lines, crlf_every=0, comment_every=0, final_newline=True, **kw):
    """n_lines lines; every comment_every-th is a `#` line"""
    out = []
    for i in range(n_lines):
        out.append(b"#!genome-build GRCh38.p%d" % i if comment_every and (i + 1) % comment_every == 0 else line(rng, **kw))
        out.append(b"\r\n" if crlf_every and (i + 1) % crlf_every == 0 else b"\n")
    if not final_newline and out:
        out[-1] = b""
    return b"".join(out)


def fill_to(rng, data, size, **kw):
    """`data` with valid feature lines appended until it is at least `size` bytes long (ends with LF)"""
    parts, n = [data], len(data)
    while n < size:
        ln = line(rng, **kw) + b"\n"
        parts.append(ln)
        n += len(ln)
    return b"".join(parts)


def rng(seed):
    return random.Random(seed)
