"""An independent restatement of the CIGAR scalars' rules ("CIGAR scalars"; the reference's
sam_functions/module.cpp:32-131 and rust/src/sam_functions.rs:114-200) for the tests: a regular expression says what is valid, a
left-to-right loop says where an invalid row is reported.  Nothing here is shared with the library or ported from its kernels."""
import re

MAX_LEN = (1 << 28) - 1
OPS = b"MIDNSHP=X"
PE_INVALID, PE_RANGE = 44, 45
INVALID_TEXT, RANGE_TEXT = b"Invalid CIGAR string", b"CIGAR insertions exceed the sequence"

_VALID = re.compile(rb"(?:[0-9]+[MIDNSHP=X])+\Z")
_OP = re.compile(rb"([0-9]+)([MIDNSHP=X])")
_DIGITS = re.compile(rb"[0-9]*")


class CigarError(Exception):
    def __init__(self, code, offset=0):
        super().__init__(code, offset)
        self.code, self.offset = code, offset


def absent(s):
    return s in (b"", b"*")


def error_offset(s):
    """where a left-to-right parser stops in an invalid row; None for a valid (or absent) one"""
    if absent(s):
        return None
    i, n = 0, len(s)
    while i < n:
        digits = _DIGITS.match(s, i).group()
        value = 0
        for k, d in enumerate(digits):
            value = value * 10 + (d - 48)
            if value > MAX_LEN:
                return i + k                  # the digit at which the value first exceeds the bound
        j = i + len(digits)
        if j == n:
            return n                          # digits up to the end of the row
        if not digits or s[j] not in OPS:
            return j                          # a letter without digits, or a byte that is neither
        i = j + 1
    return None


def parse(s):
    """-> [(letter as str, length)]"""
    off = error_offset(s)
    if off is not None:
        raise CigarError(PE_INVALID, off)
    if absent(s):
        return []
    assert _VALID.match(s)
    ops = [(m.group(2).decode(), int(m.group(1).lstrip(b"0") or b"0")) for m in _OP.finditer(s)]      # (leading zeros: any number)
    assert all(v <= MAX_LEN for _, v in ops)
    return ops


def letters(s):
    """what total_ops counts: every operation letter, those of a failing row too"""
    return sum(s.count(bytes([c])) for c in OPS)


def extract(sequence, cigar):
    """-> (start, end, slice)"""
    ops = parse(cigar)
    start = ops[0][1] if ops and ops[0][0] == "I" else 0
    end = len(sequence) - (ops[-1][1] if ops and ops[-1][0] == "I" else 0)
    if start > end or len(sequence) > (1 << 31) - 1:
        raise CigarError(PE_RANGE)
    return start, end, sequence[start:end]


def first_error(cigars, sequences=None):
    """(row, CigarError) of the lowest failing row (None rows are empty strings), or None"""
    for r, s in enumerate(cigars):
        try:
            if sequences is None:
                parse(s or b"")
            else:
                extract(sequences[r] or b"", s or b"")
        except CigarError as e:
            return r, e
    return None


def error_message(row, e):
    if e.code == PE_INVALID:
        return INVALID_TEXT + b" in row %d at byte %d" % (row, e.offset)
    return RANGE_TEXT + b" in row %d" % row
