"""The oracle of the gff_parse_attributes tests: the reference's function (exon/src/exon/gff_functions/module.cpp:29-84 over
DuckDB v0.8.1's StringUtil::Split(string, string) and StringUtil::Trim) restated on bytes, extended to say where it fails.

    parse(field) -> [(key, value), ...]            or raises AttributeError_ with .offset, .length, .segment
    spans(field) -> [(key_start, key_len, value_start, value_len), ...]   the same entries as slices of the field

An error is reported as the offset in the field of the failing segment's first byte behind its trim (of the segment's first byte
when the trim leaves nothing) and the trimmed segment's length; the text is the reference's."""
import random

WS = b" \t\n\v\f\r"


class AttributeError_(ValueError):
    def __init__(self, segment, offset):
        self.segment, self.offset, self.length = segment, offset, len(segment)
        super().__init__(error_text(segment))


def error_text(segment):
    return "Invalid attribute: '" + segment.decode("latin-1") + "' expected 'key=value;key2=value2'"


def split_nonempty(b, sep, at=0):
    """the non-empty pieces of b between sep bytes, each with its offset (+ at)"""
    out, start = [], 0
    for i in range(len(b) + 1):
        if i == len(b) or b[i:i + 1] == sep:
            if i > start:
                out.append((at + start, b[start:i]))
            start = i + 1
    return out


def spans(field):
    out = []
    for off, seg in split_nonempty(field, b";") or [(0, field)]:
        t = seg.strip(WS)
        t_off = off + (len(seg) - len(seg.lstrip(WS))) if t else off
        kv = split_nonempty(t, b"=", t_off) or [(t_off, t)]
        if len(kv) != 2:
            raise AttributeError_(t, t_off)
        out.append((kv[0][0], len(kv[0][1]), kv[1][0], len(kv[1][1])))
    return out


def parse(field):
    return [(field[k:k + kn], field[v:v + vn]) for k, kn, v, vn in spans(field)]


def outcome(field):
    """("ok", entries) or ("error", offset, length)"""
    try:
        return ("ok", parse(field))
    except AttributeError_ as e:
        return ("error", e.offset, e.length)


# ---- the fuzz both test files share -----------------------------------------------------------------------------------------
#: the share of generated fields that must parse, so that a fuzz cannot pass on errors alone
VALID_SHARE = 1 / 3
ALPHABET = [b"a", b"b", b"=", b";", b" ", b"\t", b"\r", b"\xe9"]


def fuzz_field(rng):
    """lengths 0 .. 200 over `a b = ; space tab CR` and one byte >= 0x80.  Seven fields in ten are built from well-formed entries
    with blanks around them and stray separators (most of those parse), the others are free draws (hardly any of those does)."""
    n = rng.randrange(201)
    if rng.random() < 0.3:
        return b"".join(rng.choice(ALPHABET) for _ in range(n))
    out = b""
    while True:
        word = lambda: b"".join(rng.choice([b"a", b"b", b"\xe9", b"a", b"b", b" "]) for _ in range(rng.randrange(1, 18))).strip(WS) or b"a"
        eq = b"=" * rng.choice([1, 1, 1, 1, 2])
        ent = rng.choice([b"", b"", b" ", b"\t "]) + rng.choice([b"", b"", b"", b"="]) + word() + eq + word() + rng.choice([b"", b"", b"", b"="])
        ent += rng.choice([b"", b"", b" ", b"\r", b"  \t"]) + rng.choice([b";", b";", b";;", b" ;"])
        if rng.random() < 0.02:
            ent = rng.choice([b"a;", b"=;", b"a=b=a;", b" ;", b"a= =b;"])
        if len(out) + len(ent) > n:
            break
        out += ent
    if out.endswith(b";") and rng.random() < 0.5:
        out = out[:-1]
    return out


def fuzz_fields(seed, count):
    rng = random.Random(seed)
    return [fuzz_field(rng) for _ in range(count)]
