"""BED text for the tests (helper, not collected): a WRITER — lines of every field count, a per-line mix of field counts,
CRLF, an unterminated last line, oversized names and block lists, and lies for the error cases — and an independent
READER that is the oracle of the BED tests: the twelve columns of read_bed_file as INTEGRATION.md states them, rows as
tuples, NULL as None, the first error as (record ordinal, code, byte offset of its line).

Nothing here shares code with the library.  The rules marked [R] are recalled from exon 0.2.6 over noodles-bed 0.10.0, which
are not in the reference tree; tests/test_bed_host.py names each of them so that a real exon build can falsify it."""
import random

NAMES = ["reference_sequence_name", "start", "end", "name", "score", "strand", "thick_start", "thick_end", "color",
         "block_count", "block_sizes", "block_starts"]
INT_COLS = (1, 2, 4, 6, 7, 9)
FIELD_COUNTS = (3, 4, 5, 6, 7, 8, 9, 12)

# parse errors, numbered like include/exon_gpu.h (EXG_PE_*)
E_INVALID_UTF8 = 4
E_FIELD_COUNT, E_REFERENCE_NAME, E_POSITION, E_SCORE, E_STRAND, E_COLOR, E_BLOCKS = 22, 23, 24, 25, 26, 27, 28

I63 = (1 << 63) - 1


# ---------------------------------------------------------------- reader (the oracle)
class BedError(Exception):
    def __init__(self, code):
        Exception.__init__(self, code)
        self.code = code


def _uint(text, most, code):
    """Rust's usize::from_str: an optional single '+', then one or more ASCII digits; at most `most`"""
    digits = text[1:] if text[:1] == b"+" else text
    if not digits or any(not 48 <= c <= 57 for c in digits):
        raise BedError(code)
    v = int(digits)
    if v > most:
        raise BedError(code)
    return v


def _blocks(text, count):
    """the text of the first `count` comma-separated items (each an integer)"""
    if count == 0:
        return b""
    items = text.split(b",")
    if len(items) < count:
        raise BedError(E_BLOCKS)
    for it in items[:count]:
        _uint(it, I63, E_BLOCKS)
    return b",".join(items[:count])


def parse_line(line):
    """one line (terminator and its CR stripped) -> the row; raises BedError"""
    f = line.split(b"\t")
    n = len(f)
    if n not in FIELD_COUNTS:
        raise BedError(E_FIELD_COUNT)
    row = [None] * 12
    if not f[0]:
        raise BedError(E_REFERENCE_NAME)
    row[0] = f[0]
    row[1] = _uint(f[1], I63 - 1, E_POSITION) + 1
    row[2] = _uint(f[2], I63, E_POSITION)
    if row[2] < 1:
        raise BedError(E_POSITION)
    if n >= 4 and f[3] != b".":
        row[3] = f[3]
    if n >= 5 and f[4] != b"0":
        row[4] = _uint(f[4], 1000, E_SCORE)
        if row[4] < 1:
            raise BedError(E_SCORE)
    if n >= 6:
        if f[5] in (b"+", b"-"):
            row[5] = f[5]
        elif f[5] != b".":
            raise BedError(E_STRAND)
    if n >= 7:
        row[6] = _uint(f[6], I63 - 1, E_POSITION) + 1
    if n >= 8:
        row[7] = _uint(f[7], I63, E_POSITION)
        if row[7] < 1:
            raise BedError(E_POSITION)
    if n >= 9 and f[8] != b"0":
        parts = f[8].split(b",")
        if len(parts) != 3:
            raise BedError(E_COLOR)
        for p in parts:
            _uint(p, 255, E_COLOR)
        row[8] = f[8]
    if n == 12:
        row[9] = _uint(f[9], I63, E_POSITION)
        row[10] = _blocks(f[10], row[9])
        row[11] = _blocks(f[11], row[9])
    try:
        line.decode("utf-8")
    except UnicodeDecodeError:
        raise BedError(E_INVALID_UTF8)
    return tuple(row)


def lines_of(data):
    """[(offset, line bytes)]: a line ends at LF, one CR in front of it is stripped; an unterminated last line is a line"""
    out, pos = [], 0
    while pos < len(data):
        nl = data.find(b"\n", pos)
        if nl < 0:
            out.append((pos, data[pos:]))
            break
        end = nl - 1 if nl > pos and data[nl - 1:nl] == b"\r" else nl
        out.append((pos, data[pos:end]))
        pos = nl + 1
    return out


def read(data):
    """-> (rows in front of the first failing line, None | (record ordinal, code, byte offset of the line))"""
    rows = []
    for off, line in lines_of(data):
        try:
            rows.append(parse_line(line))
        except BedError as e:
            return rows, (len(rows), e.code, off)
    return rows, None


# ---------------------------------------------------------------- writer
def line(rng, n_fields, name=None, n_blocks=None, extra_blocks=0, trailing_comma=False):
    """a valid line (no terminator) of n_fields fields: 25 to 90 bytes unless `name` or `n_blocks` make it longer"""
    start = rng.randrange(100_000_000, 250_000_000)
    end = start + rng.randrange(1, 100_000)
    f = [rng.choice([b"chr10", b"chr11", b"chr17", b"chr22", b"chrUn1"]), b"%d" % start, b"%d" % end]
    if n_fields >= 4:
        f.append(name if name is not None else rng.choice([b".", b"f%d" % rng.randrange(10 ** rng.randrange(1, 6))]))
    if n_fields >= 5:
        f.append(rng.choice([b"0", b"%d" % rng.randrange(1, 1001), b"1000", b"1"]))
    if n_fields >= 6:
        f.append(rng.choice([b"+", b"-", b"."]))
    if n_fields >= 7:
        f.append(b"%d" % rng.randrange(start, end))
    if n_fields >= 8:
        f.append(b"%d" % end)
    if n_fields >= 9:
        f.append(rng.choice([b"0", b"255,0,0", b"0,0,255", b"12,34,56", b"+1,02,3"]))
    if n_fields == 12:
        k = rng.randrange(0, 3) if n_blocks is None else n_blocks
        f.append(b"%d" % k)
        for _ in range(2):
            items = [b"%d" % rng.randrange(0, 1000 if n_blocks is None else 100_000) for _ in range(k + extra_blocks)]
            f.append(b",".join(items) + (b"," if trailing_comma or (n_blocks is None and items and rng.random() < 0.3) else b""))
    assert len(f) == n_fields
    return b"\t".join(f)


def mixed(rng, n_lines, crlf_every=0, final_newline=True, counts=FIELD_COUNTS):
    """n_lines lines whose field counts cycle through `counts` in a shuffled order; a CRLF on every crlf_every-th line"""
    out = []
    for i in range(n_lines):
        out.append(line(rng, counts[rng.randrange(len(counts))]))
        out.append(b"\r\n" if crlf_every and (i + 1) % crlf_every == 0 else b"\n")
    if not final_newline and out:
        out[-1] = b""
    return b"".join(out)


def fill_to(rng, data, size, counts=FIELD_COUNTS):
    """`data` with valid lines appended until it is at least `size` bytes long (ends with LF)"""
    parts, n = [data], len(data)
    while n < size:
        ln = line(rng, counts[rng.randrange(len(counts))]) + b"\n"
        parts.append(ln)
        n += len(ln)
    return b"".join(parts)


def rng(seed):
    return random.Random(seed)
