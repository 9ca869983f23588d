"""BCF 2.2 for the tests: a writer (records described by typed fields -> bytes, BGZF framing from bam_files) and an independent
renderer (BCF bytes -> the VCF lines they stand for, VCF 4.3 spec section 6.3 as INTEGRATION.md states the rules).  Nothing here
shares code with csrc: the renderer is the second statement of the rules that the device transcoder (exg_bcf.hip) is held to.

Typed values are built with ints(), floats(), chars(), flag(); MISSING and EOV stand for the two reserved values of a type.
"""
import re
import struct

import numpy as np

import bam_files as BAM

MISSING, EOV = "missing", "end-of-vector"
INT_MISSING = {1: -128, 2: -32768, 3: -2147483648}
F_MISSING, F_EOV = 0x7F800001, 0x7F800002
ESIZE = {0: 0, 1: 1, 2: 2, 3: 4, 5: 4, 7: 1}
PACK = {1: "<b", 2: "<h", 3: "<i"}

# EXG_PE_BCF_* (include/exon_gpu.h)
E_RECORD_LENGTH, E_TRUNCATED, E_TYPE, E_RESERVED, E_OVERRUN, E_CHROM, E_DICT, E_NO_ALLELE, E_SAMPLE_COUNT = range(47, 56)


class BcfError(Exception):
    def __init__(self, code):
        Exception.__init__(self, f"BCF record error {code}")
        self.code = code


# ---- writer ---------------------------------------------------------------------------------------------------------------------
def typed_int(v, width=None):
    """a typed integer scalar (a key, a long form's length): the narrowest type that holds v, or `width` (1, 2, 3)"""
    t = width or (1 if -120 <= v <= 127 else 2 if -32760 <= v <= 32767 else 3)
    return bytes([0x10 | t]) + struct.pack(PACK[t], v)


def descriptor(type_, count, long_form=False):
    if count < 15 and not long_form:
        return bytes([(count << 4) | type_])
    return bytes([0xF0 | type_]) + typed_int(count)


def ints(values, width=None, long_form=False, pad_to=None):
    """an integer vector: values are ints, MISSING or EOV; the narrowest type that holds them (reserved values excluded), or
    `width`; pad_to: padded with EOV to that many elements.  -> (type, count, data)"""
    nums = [v for v in values if isinstance(v, int)]
    lo, hi = (min(nums), max(nums)) if nums else (0, 0)
    t = width or (1 if lo >= -120 and hi <= 127 else 2 if lo >= -32760 and hi <= 32767 else 3)
    vals = list(values) + [EOV] * max(0, (pad_to or 0) - len(values))
    raw = [INT_MISSING[t] if v is MISSING else INT_MISSING[t] + 1 if v is EOV else v for v in vals]
    return t, len(vals), b"".join(struct.pack(PACK[t], v) for v in raw), long_form


def floats(values, long_form=False, pad_to=None):
    """a float vector: values are Python floats, ("bits", u32), MISSING or EOV"""
    vals = list(values) + [EOV] * max(0, (pad_to or 0) - len(values))
    out = []
    for v in vals:
        if v is MISSING:
            out.append(struct.pack("<I", F_MISSING))
        elif v is EOV:
            out.append(struct.pack("<I", F_EOV))
        elif isinstance(v, tuple):
            out.append(struct.pack("<I", v[1]))
        else:
            out.append(np.float32(v).tobytes())
    return 5, len(vals), b"".join(out), long_form


def chars(text, pad_to=None, long_form=False):
    data = text + b"\0" * max(0, (pad_to or 0) - len(text))
    return 7, len(data), data, long_form


def flag():
    return 0, 0, b"", False


def raw_value(type_, count, data, long_form=False):
    return type_, count, data, long_form


def enc(value):
    t, n, data, long_form = value
    return descriptor(t, n, long_form) + data


def record(chrom=0, pos=0, rlen=1, qual=MISSING, id_=b"", alleles=(b"A",), filters=None, info=(), fmt=(), n_sample=0, n_allele=None,
           l_shared=None, l_indiv=None, filter_value=None, n_sample_field=None):
    """One record.  qual: a float, ("bits", u32) or MISSING; filters: None / [] (no value) or dictionary indices; info: [(key,
    value)]; fmt: [(key, [per-sample value, ...])] — the per-sample values of one field must share type and count (use pad_to).
    n_allele / l_shared / l_indiv / filter_value / n_sample_field override what is written (for malformed records)."""
    q = struct.pack("<I", F_MISSING) if qual is MISSING else struct.pack("<I", qual[1]) if isinstance(qual, tuple) else np.float32(qual).tobytes()
    shared = [enc(chars(id_))] + [enc(chars(a)) for a in alleles]
    if filter_value is not None:
        shared.append(enc(filter_value))
    else:
        shared.append(enc(ints(filters)) if filters else enc(flag()))
    for key, value in info:
        shared.append((typed_int(key) if isinstance(key, int) else key) + enc(value))
    indiv = []
    for key, per_sample in fmt:
        assert len(per_sample) == n_sample and len({(v[0], v[1]) for v in per_sample}) == 1, "one type and count per FORMAT field"
        t, n, _, long_form = per_sample[0]
        indiv.append((typed_int(key) if isinstance(key, int) else key) + descriptor(t, n, long_form) + b"".join(v[2] for v in per_sample))
    shared, indiv = b"".join(shared), b"".join(indiv)
    na = len(alleles) if n_allele is None else n_allele
    ns = n_sample if n_sample_field is None else n_sample_field
    fixed = struct.pack("<iii", chrom, pos, rlen) + q + struct.pack("<II", (na << 16) | len(info), (len(fmt) << 24) | ns)
    return struct.pack("<II", 24 + len(shared) if l_shared is None else l_shared, len(indiv) if l_indiv is None else l_indiv) + fixed + shared + indiv


def header_text(contigs=("1", "2"), filters=(), infos=(), formats=(), samples=(), idx=False, extra=()):
    """a VCF header as a BCF file holds it.  infos / formats: [(id, number, type)].  idx: write IDX= attributes (PASS 0, then in
    order of first appearance)."""
    order = ["PASS"]
    for i in list(filters) + [x[0] for x in infos] + [x[0] for x in formats]:
        if i not in order:
            order.append(i)
    at = lambda i: f",IDX={order.index(i)}" if idx else ""
    lines = ["##fileformat=VCFv4.2", f'##FILTER=<ID=PASS,Description="All filters passed"{at("PASS")}>']
    lines += [f'##FILTER=<ID={f},Description="filter {f}"{at(f)}>' for f in filters if f != "PASS"]
    lines += [f'##contig=<ID={c},length=1000000{f",IDX={k}" if idx else ""}>' for k, c in enumerate(contigs)]
    lines += [f'##INFO=<ID={i},Number={n},Type={t},Description="info, {i}"{at(i)}>' for i, n, t in infos]
    lines += [f'##FORMAT=<ID={i},Number={n},Type={t},Description="format {i}"{at(i)}>' for i, n, t in formats]
    lines += list(extra)
    cols = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO" + ("\tFORMAT\t" + "\t".join(samples) if samples else "")
    return ("\n".join(lines + [cols]) + "\n").encode()


def file_header(text, minor=2, terminate=True):
    t = text + (b"\0" if terminate else b"")
    return b"BCF\2" + bytes([minor]) + struct.pack("<I", len(t)) + t


def dictionaries(text):
    """(strings, contigs, n_samples) of a header text: lists indexed by dictionary index (None: no such index)"""
    strings, contigs, n_samples = {"PASS": 0}, {}, 0
    for line in text.decode().split("\n"):
        m = re.match(r"##(FILTER|INFO|FORMAT|contig)=<(.*)>\s*$", line)
        if m:
            d = contigs if m.group(1) == "contig" else strings
            attrs = dict(re.findall(r'(\w+)=("(?:[^"\\]|\\.)*"|[^,>]*)', m.group(2)))
            if "ID" not in attrs or attrs["ID"] in d:
                continue
            d[attrs["ID"]] = int(attrs["IDX"]) if "IDX" in attrs else (max(d.values()) + 1 if d else 0)
        elif line.startswith("#CHROM"):
            n_samples = max(0, len(line.split("\t")) - 9)
    def table(d):
        out = [None] * (max(d.values()) + 1 if d else 0)
        for k, v in d.items():
            out[v] = k.encode()
        return out
    return table(strings), table(contigs), n_samples


def bgzf_file(text, records, member_bytes=0xFF00, level=6, **kw):
    return BAM.bgzf(file_header(text, **kw) + b"".join(records), member_bytes=member_bytes, level=level)


# ---- renderer -------------------------------------------------------------------------------------------------------------------
def _typed_int(b, o, lim):
    if o + 1 > lim:
        raise BcfError(E_OVERRUN)
    t = b[o] & 15
    if b[o] >> 4 != 1 or t not in (1, 2, 3):
        raise BcfError(E_TYPE)
    if o + 1 + ESIZE[t] > lim:
        raise BcfError(E_OVERRUN)
    return struct.unpack_from(PACK[t], b, o + 1)[0], o + 1 + ESIZE[t]


def _descriptor(b, o, lim):
    if o + 1 > lim:
        raise BcfError(E_OVERRUN)
    t, n = b[o] & 15, b[o] >> 4
    o += 1
    if t not in ESIZE:
        raise BcfError(E_TYPE)
    if n == 15:
        n, o = _typed_int(b, o, lim)
        if n < 0:
            raise BcfError(E_TYPE)
    return t, n, o


def _value(b, o, lim):
    t, n, o = _descriptor(b, o, lim)
    if o + n * ESIZE[t] > lim:
        raise BcfError(E_OVERRUN)
    return t, n, o, o + n * ESIZE[t]


def fmt_float(bits):
    """nine significant digits of the float: any spelling that reads back to the same float32 is as good (lines_equal)"""
    f = np.array([bits], np.uint32).view(np.float32)[0]
    if np.isnan(f):
        return b"nan"
    if np.isinf(f):
        return b"-inf" if f < 0 else b"inf"
    return ("%.9g" % float(f)).encode()


def _int_kind(v, t):
    d = v - INT_MISSING[t]
    return MISSING if d == 0 else EOV if d == 1 else "reserved" if d < 8 else None


def _elements(b, t, n, o):
    """the texts of a numeric vector's elements up to the first end-of-vector"""
    out = []
    for i in range(n):
        if t == 5:
            bits = struct.unpack_from("<I", b, o + 4 * i)[0]
            if bits == F_EOV:
                break
            out.append(b"." if bits == F_MISSING else fmt_float(bits))
        else:
            v = struct.unpack_from(PACK[t], b, o + ESIZE[t] * i)[0]
            k = _int_kind(v, t)
            if k is EOV:
                break
            if k == "reserved":
                raise BcfError(E_RESERVED)
            out.append(b"." if k is MISSING else str(v).encode())
    return out


def render_value(b, t, n, o):
    if t == 0:          # no data whatever the count says
        return b"."
    if t == 7:
        s = bytes(b[o:o + n]).split(b"\0")[0]
        return s or b"."
    return b",".join(_elements(b, t, n, o)) or b"."


def render_gt(b, t, n, o):
    out = b""
    k = 0
    for i in range(n):
        v = struct.unpack_from(PACK[t], b, o + ESIZE[t] * i)[0]
        kind = _int_kind(v, t)
        if kind is EOV:
            break
        if kind == "reserved" or (kind is None and v < 0):
            raise BcfError(E_RESERVED)
        if k:
            out += b"|" if kind is None and v & 1 else b"/"
        out += b"." if kind is MISSING or v >> 1 == 0 else str((v >> 1) - 1).encode()
        k += 1
    return out or b"."


def render_record(b, s, strings, contigs, n_samples):
    """the VCF line (without its LF) of the complete record at b[s:]"""
    ls, li, chrom, pos, _rlen, qual, nai, nfs = struct.unpack_from("<IIiiiIII", b, s)
    n_allele, n_info, n_fmt, n_sample = nai >> 16, nai & 0xFFFF, nfs >> 24, nfs & 0xFFFFFF
    lim_s, lim_i = s + 8 + ls, s + 8 + ls + li
    name = lambda idx: strings[idx] if 0 <= idx < len(strings) and strings[idx] is not None else None
    if not (0 <= chrom < len(contigs)) or contigs[chrom] is None:
        raise BcfError(E_CHROM)
    if n_allele == 0:
        raise BcfError(E_NO_ALLELE)
    if n_sample != n_samples:
        raise BcfError(E_SAMPLE_COUNT)
    cols = [contigs[chrom], str(pos + 1).encode()]
    o = s + 32
    strs = []
    for _ in range(1 + n_allele):
        t, n, d, o = _value(b, o, lim_s)
        if t not in (0, 7):
            raise BcfError(E_TYPE)
        strs.append(render_value(b, t, n, d))
    cols += [strs[0], strs[1], b",".join(strs[2:]) or b"."]
    cols.append(b"." if qual in (F_MISSING, F_EOV) else fmt_float(qual))
    t, n, d, o = _value(b, o, lim_s)
    if t > 3:
        raise BcfError(E_TYPE)
    names = []
    for i in range(n if t else 0):
        k = name(struct.unpack_from(PACK[t], b, d + ESIZE[t] * i)[0])
        if k is None:
            raise BcfError(E_DICT)
        names.append(k)
    cols.append(b";".join(names) or b".")
    entries = []
    for _ in range(n_info):
        key, o = _typed_int(b, o, lim_s)
        if name(key) is None:
            raise BcfError(E_DICT)
        t, n, d, o = _value(b, o, lim_s)
        entries.append(name(key) if t == 0 else name(key) + b"=" + render_value(b, t, n, d))
    cols.append(b";".join(entries) or b".")
    if n_fmt and n_sample:
        o = lim_s
        fields = []
        for _ in range(n_fmt):
            key, o = _typed_int(b, o, lim_i)
            if name(key) is None:
                raise BcfError(E_DICT)
            t, n, o = _descriptor(b, o, lim_i)
            if o + n_sample * n * ESIZE[t] > lim_i:
                raise BcfError(E_OVERRUN)
            fields.append((name(key), t, n, o))
            o += n_sample * n * ESIZE[t]
        cols.append(b":".join(f[0] for f in fields))
        for k in range(n_sample):
            cols.append(b":".join(render_gt(b, t, n, d + k * n * ESIZE[t]) if nm == b"GT" and t in (1, 2, 3) else
                                  render_value(b, t, n, d + k * n * ESIZE[t]) for nm, t, n, d in fields))
    return b"\t".join(cols)


class Rendered:
    """the serial chain over record bytes: lines of the complete records in front of the first error, error = None or (record
    ordinal, code, offset), consumed = the offset behind the last rendered record, offsets[k] = where record k begins"""

    def __init__(self, b, strings, contigs, n_samples, eof=True):
        b = memoryview(bytes(b))
        self.lines, self.offsets, self.error, s = [], [], None, 0
        while s < len(b):
            code = None
            if s + 8 > len(b):
                code = E_TRUNCATED
            else:
                ls, li = struct.unpack_from("<II", b, s)
                if ls < 24:
                    code = E_RECORD_LENGTH
                elif s + 8 + ls + li > len(b):
                    code = E_TRUNCATED
            if code is None:
                try:
                    line = render_record(b, s, strings, contigs, n_samples)
                except BcfError as e:
                    code = e.code
            if code is not None:
                if code != E_TRUNCATED or eof:
                    self.error = (len(self.lines), code, s)
                break
            self.lines.append(line)
            self.offsets.append(s)
            s += 8 + ls + li
        self.consumed = s
        self.text = b"".join(ln + b"\n" for ln in self.lines)


def render_file(raw):
    """decoded bytes of a BCF file -> (header text, Rendered)"""
    assert raw[:5] == b"BCF\2\2"
    l_text = struct.unpack_from("<I", raw, 5)[0]
    text = raw[9:9 + l_text].split(b"\0")[0]
    strings, contigs, n_samples = dictionaries(text)
    return text, Rendered(raw[9 + l_text:], strings, contigs, n_samples)


# ---- comparing lines: byte for byte, except that a number may be spelled differently when it is the same float32 ------------------
_SEP = re.compile(rb"([\t;:,=/|\n])")


def _same_token(a, b):
    if a == b:
        return True
    try:
        with np.errstate(all="ignore"):
            fa, fb = np.float32(a.decode()), np.float32(b.decode())
    except (ValueError, UnicodeDecodeError):
        return False
    if not re.fullmatch(rb"[-+0-9.eEinfa]+", a) or not re.fullmatch(rb"[-+0-9.eEinfa]+", b):
        return False
    return fa.tobytes() == fb.tobytes() or (np.isnan(fa) and np.isnan(fb))


def text_equal(a, b):
    """None when the two texts are equal in that sense, else a description of the first difference"""
    if a == b:
        return None
    ta, tb = _SEP.split(a), _SEP.split(b)
    for i, (x, y) in enumerate(zip(ta, tb)):
        if not _same_token(x, y):
            return f"token {i}: {x[:60]!r} != {y[:60]!r} (line {a[:a.find(x)].count(10) if x in a else '?'})"
    if len(ta) != len(tb):
        return f"{len(ta)} tokens != {len(tb)} tokens"
    return None
