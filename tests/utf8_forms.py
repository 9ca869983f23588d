"""UTF-8 forms for the validators of the text scans: a catalogue of well- and ill-formed byte strings judged by Python's strict
decoder alone, the forms placed at seams, builders that put a form into a chosen field of a chosen record of each text format
(optionally with a chosen byte on a chosen absolute offset), and the reference verdict on such an input.

Not collected: tests/test_utf8_forms.py checks this module on the CPU, tests/test_utf8_gpu.py drives the device with it."""
from collections import namedtuple

import bed_files as B
import gtf_files as G
import sam_files as S

E_INVALID_UTF8 = 4
HALF, SUPER, WINDOW = 16384, 32768, 1024       # the single-pass scans' staging unit, their super-tile, the window in front of it
FORMATS = ("fastq", "fasta", "vcf", "bed", "sam", "gtf")
VCF_HDR = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def strict(b):
    """Python's strict decoder: the only judge of `well_formed`"""
    try:
        bytes(b).decode("utf-8", "strict")
        return True
    except UnicodeDecodeError:
        return False


# ---------------------------------------------------------------- the catalogue
LEADS = (0x7F, 0x80, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xEF, 0xF0, 0xF4, 0xF5, 0xF7, 0xF8, 0xFF)
SECOND = {0xC2: (0x7F, 0x80, 0xBF, 0xC0), 0xDF: (0x7F, 0x80, 0xBF, 0xC0),
          0xE0: (0x9F, 0xA0, 0xBF, 0xC0),
          0xE1: (0x7F, 0x80, 0xBF, 0xC0), 0xEC: (0x7F, 0x80, 0xBF, 0xC0), 0xEE: (0x7F, 0x80, 0xBF, 0xC0), 0xEF: (0x7F, 0x80, 0xBF, 0xC0),
          0xED: (0x7F, 0x80, 0x9F, 0xA0),
          0xF0: (0x8F, 0x90, 0xBF, 0xC0),
          0xF1: (0x7F, 0x80, 0xBF, 0xC0), 0xF3: (0x7F, 0x80, 0xBF, 0xC0),
          0xF4: (0x7F, 0x80, 0x8F, 0x90)}
EDGE4 = (0x7F, 0x80, 0xBF, 0xC0)
EXTREMES = (b"\xc2\x80", b"\xdf\xbf", b"\xe0\xa0\x80", b"\xed\x9f\xbf", b"\xee\x80\x80", b"\xef\xbf\xbf", b"\xf0\x90\x80\x80", b"\xf4\x8f\xbf\xbf")
CHARS = (b"\xc3\xa9", b"\xe2\x82\xac", b"\xf0\x9f\x98\x80")


def implied_length(lead):
    """bytes the lead announces (1 where it announces none: ASCII, a continuation, FE / FF)"""
    return 1 if lead < 0xC0 else 2 if lead < 0xE0 else 3 if lead < 0xF0 else 4 if lead < 0xF8 else 5 if lead < 0xFC else 1


def valid_tail(lead):
    """continuation bytes that are inside every window of `lead`"""
    n = implied_length(lead) - 1
    first = {0xE0: 0xA0, 0xF0: 0x90}.get(lead, 0x80)
    return bytes([first] + [0x80] * (n - 1)) if n else b""


def _second_forms():
    return [bytes([lead, c1]) + valid_tail(lead)[1:] for lead, window in SECOND.items() for c1 in window]


def catalogue():
    """[(bytes, well_formed)]: every lead class, every continuation window's edges, every truncation, the extreme scalars"""
    forms = [bytes([lead]) + valid_tail(lead) for lead in LEADS]
    forms += _second_forms()
    for lead in (0xE0, 0xE1, 0xED, 0xEF, 0xF0, 0xF1, 0xF4):
        t = valid_tail(lead)
        forms += [bytes([lead, t[0], c2]) + t[2:] for c2 in EDGE4]
    for lead in (0xF0, 0xF1, 0xF4):
        t = valid_tail(lead)
        forms += [bytes([lead, t[0], t[1], c3]) for c3 in EDGE4]
    for ch in CHARS + EXTREMES:
        forms += [ch[:k] for k in range(1, len(ch))]
    forms += list(EXTREMES + CHARS)
    out, seen = [], set()
    for f in forms:
        if f not in seen:
            seen.add(f)
            out.append((f, strict(f)))
    assert len(out) >= 90 and sum(1 for _, ok in out if not ok) >= 60, (len(out), sum(1 for _, ok in out if not ok))
    return out


def boundary_subset():
    """the 2-, 3- and 4-byte forms whose SECOND byte sits on an edge of its window, and the extreme scalars"""
    keep = set(_second_forms()) | set(EXTREMES)
    out = [(f, ok) for f, ok in catalogue() if f in keep]
    assert len(out) == len(keep)
    return out


# (form, the form is the last bytes of its field): a well-formed and an ill-formed one per length, a surrogate, a cut prefix
SeamForm = namedtuple("SeamForm", "form ends_field")
SEAM_FORMS = (SeamForm(b"\xc3\xa9", False), SeamForm(b"\xe2\x82\xac", False), SeamForm(b"\xf0\x9f\x98\x80", False),
              SeamForm(b"\xc3\x41", False), SeamForm(b"\xe2\x82\x41", False), SeamForm(b"\xf0\x9f\x98\x41", False),
              SeamForm(b"\xed\xa0\x80", False), SeamForm(b"\xe2\x82", True))
FUSED_SEAMS = (16, 1024, 4096, 15360, 16384, 31744, 32768, 49152, 65536)     # chunk, chunk row, ..., window, half and super-tile starts
FASTA_SEAMS = (16, 1024, 4096, 8192, 16384, 24576, 32768, 65536)


def placements(sf):
    """j = 0..L: the form's first byte at S - j — wholly behind the seam, every split, wholly in front of it"""
    out = list(range(len(sf.form) + 1))
    assert len(out) == len(sf.form) + 1
    return out


# ---------------------------------------------------------------- records of each format
# record(i, text, field, broken) -> (the record with its terminator, offset of `text` in it).  `text` stands in `field`, everything
# else is ASCII; `broken` gives the record a structural error that does not touch `text`.
TEXT = object()


def _join(parts, text):
    off, toff = 0, None
    out = []
    for p in parts:
        if p is TEXT:
            assert toff is None
            toff, p = off, text
        out.append(p)
        off += len(p)
    assert toff is not None
    return b"".join(out), toff


def _pick(field, name, default):
    return TEXT if field == name else default


def _fastq(i, text, field, broken):
    n = len(text) if field in ("sequence", "quality") else 10
    seq = TEXT if field == "sequence" else b"A" * n
    qual = TEXT if field == "quality" else b"I" * n
    return _join([b"@", _pick(field, "name", b"r%06d" % i), b" ", _pick(field, "description", b"d"), b"\n", seq, b"\n",
                  b"-" if broken else b"+", _pick(field, "plus", b""), b"\n", qual, b"\n"], text)


def _fasta(i, text, field, broken):
    assert not (broken and field == "id")
    ident = b"" if broken else _pick(field, "id", b"s%06d" % i)          # an empty id: the definition's name is missing
    return _join([b">", ident, b" ", _pick(field, "description", b"d"), b"\n", _pick(field, "sequence", b"ACGTACGTACGT"), b"\n"], text)


def _vcf(i, text, field, broken):
    pos = b"x%06d" % i if broken else b"%07d" % (1000000 + i)
    return _join([b"1\t", pos, b"\t", _pick(field, "id", b"."), b"\tA\tC\t.\t", _pick(field, "filter", b"."), b"\t", _pick(field, "info", b"S=1"),
                  b"\n"], text)


def _bed(i, text, field, broken):
    start = b"x%06d" % i if broken else b"%07d" % (1000000 + i)
    return _join([_pick(field, "chrom", b"chr1"), b"\t", start, b"\t%07d\t" % (2000000 + i), _pick(field, "name", b"n"), b"\n"], text)


def _sam(i, text, field, broken):
    n = len(text) if field == "quality" else 4
    return _join([_pick(field, "name", b"r%06d" % i), b"\t", b"x" if broken else b"0", b"\t", _pick(field, "reference", b"chr1"),
                  b"\t100\t60\t", _pick(field, "cigar", b"*"), b"\t*\t0\t0\t", b"A" * n, b"\t", _pick(field, "quality", b"I" * n), b"\tCO:Z:",
                  _pick(field, "aux", b"c"), b"\n"], text)


def _gtf(i, text, field, broken):
    return _join([_pick(field, "seqname", b"chr1"), b"\t", _pick(field, "source", b"src"), b"\t", _pick(field, "type", b"exon"),
                  b"\t%07d\t%07d\t.\t" % (1000000 + i, 2000000 + i), b"*" if broken else b"+", b"\t.\tgene_id ",
                  _pick(field, "attributes", b"g"), b"\n"], text)


Format = namedtuple("Format", "record free early fields unvalidated last")
# free: the free-text field the builders pad and place forms in (it ends at the record's first line end or at its last);
# early: a field that begins within the record's first 12 bytes; fields: validated string fields; last: the input's last field
FMT = {"fastq": Format(_fastq, "description", "name", ("name", "description", "sequence", "quality"), ("plus",), "quality"),
       "fasta": Format(_fasta, "description", "id", ("id", "description", "sequence"), (), "sequence"),
       "vcf": Format(_vcf, "info", "id", ("id", "filter", "info"), (), "info"),
       "bed": Format(_bed, "name", "chrom", ("chrom", "name"), (), "name"),
       "sam": Format(_sam, "aux", "name", ("name", "reference", "quality", "aux"), (), "aux"),
       "gtf": Format(_gtf, "attributes", "seqname", ("seqname", "source", "type", "attributes"), (), "attributes")}
STD = 96                                       # bytes of free text in an ordinary padding record


def record(fmt, i, text, field=None, broken=False):
    f = FMT[fmt]
    return f.record(i, bytes(text), field or f.free, broken)


def _pad(fmt, out, n_rec, target):
    """ordinary records until `out` is exactly `target` bytes long -> the number of records then"""
    base = len(record(fmt, 0, b"x")[0]) - 1
    while target - len(out) >= 2 * (base + STD):
        out += record(fmt, n_rec, b"p" * STD)[0]
        n_rec += 1
    gap = target - len(out)
    if gap == 0:
        return n_rec
    if gap >= 2 * (base + 1):
        first = gap // 2
        out += record(fmt, n_rec, b"p" * (first - base))[0]
        n_rec += 1
        gap -= first
    assert gap >= base + 1, (fmt, target, gap, "no room for a padding record in front of this offset")
    out += record(fmt, n_rec, b"p" * (gap - base))[0]
    assert len(out) == target
    return n_rec + 1


Site = namedtuple("Site", "text k offset field broken", defaults=(None, False))
# text[k] lands on data[offset]; field None: the format's free-text field


def build(fmt, sites, size=2 * SUPER + 2048, final_newline=True, stop=False):
    """an input of `fmt` of at least `size` bytes that holds each site's text in a record of its own, text[k] on the site's absolute
    offset; earlier records' free text is padded to get there.  stop: the last site's record is the input's last.
    -> (data, [the record index of each site])"""
    out, n_rec, idx = bytearray(), 0, []
    for s in sorted(sites, key=lambda s: s.offset):
        rec, toff = record(fmt, 0, s.text, s.field, s.broken)
        start = s.offset - s.k - toff
        assert start >= len(out), (fmt, s.offset, start, len(out), "sites too close, or the offset lies in front of the field")
        n_rec = _pad(fmt, out, n_rec, start)
        rec, toff = record(fmt, n_rec, s.text, s.field, s.broken)
        out += rec
        assert out[s.offset] == s.text[s.k] and bytes(out[start + toff:start + toff + len(s.text)]) == s.text
        idx.append(n_rec)
        n_rec += 1
    if not stop:
        while len(out) < size:
            out += record(fmt, n_rec, b"p" * STD)[0]
            n_rec += 1
    data = bytes(out)
    order = sorted(range(len(sites)), key=lambda j: sites[j].offset)
    by_site = [None] * len(sites)
    for rank, j in enumerate(order):
        by_site[j] = idx[rank]
    return (data if final_newline else data[:-1]), by_site


def in_field(form, pre=20, post=8, ends_field=False):
    """(text, k): `form` with ASCII around it, k = the offset of its first byte"""
    return b"x" * pre + form + (b"" if ends_field else b"y" * post), pre


def seam_site(fmt, sf, seam, j, field=None):
    """the seam form with its first byte on seam - j; at the seam 16 it stands in the first record's `early` field"""
    if seam - j < 64:
        field = FMT[fmt].early
        text, k = in_field(sf.form, pre=seam - j - record(fmt, 0, b"x", field)[1], ends_field=sf.ends_field)
    else:
        text, k = in_field(sf.form, ends_field=sf.ends_field)
    return Site(text, k, seam - j, field)


def is_ascii_but(data, spans):
    """every byte outside [a, b) of `spans` is ASCII"""
    keep = bytearray(data)
    for a, b in spans:
        keep[a:b] = b"\0" * (b - a)
    return max(keep, default=0) < 0x80


# ---------------------------------------------------------------- the reference verdict
def _lines(data):
    out = data.split(b"\n")
    if out and out[-1] == b"":
        out.pop()
    return [ln[:-1] if ln.endswith(b"\r") else ln for ln in out]


def validated_fields(fmt, data, limit=None):
    """per record, the byte strings the reference turns into Utf8 values (records in front of `limit` only: they are known to be
    structurally sound, so lines group into records as written)"""
    lines = _lines(data)
    out = []
    if fmt == "fastq":
        for r in range(0, len(lines) - 3, 4):
            name, _, desc = lines[r][1:].partition(b" ")
            out.append([name, desc, lines[r + 1], lines[r + 3]])
    elif fmt == "fasta":
        for ln in lines:
            if ln[:1] == b">":
                out.append([ln[1:], b""])              # the definition line is read into a String whole, the sequence joined
            elif out:
                out[-1][1] += ln
    else:
        out = [[ln] for ln in lines]
    return out if limit is None else out[:limit]


def first_ill_formed(fmt, data, limit=None):
    for r, fields in enumerate(validated_fields(fmt, data, limit)):
        if not all(strict(f) for f in fields):
            return r
    return None


Verdict = namedtuple("Verdict", "code record offset n_rows ref")


def expect(fmt, data):
    """the format's existing reference on `data` (VCF: behind VCF_HDR, offsets counted without it), checked against Python's strict
    decoder: a UTF-8 error names the first record whose validated fields do not all decode, any other outcome has no such record
    in front of it"""
    from oracle import pyoracle
    if fmt in ("fastq", "fasta", "vcf"):
        if fmt == "vcf":
            ref = pyoracle.vcf_parse(VCF_HDR + data, payload_base=VCF_BASE - len(VCF_HDR))
        else:
            ref = pyoracle.fastq_parse(data, payload_base=FASTQ_BASE) if fmt == "fastq" else pyoracle.fasta_parse(data)
        off = ref.error_offset - (len(VCF_HDR) if fmt == "vcf" and ref.error_code else 0)
        v = Verdict(ref.error_code, ref.error_record if ref.error_code else None, off if ref.error_code else None, ref.n_rows, ref)
    else:
        got = {"bed": B.read, "sam": S.read}[fmt](data) if fmt != "gtf" else G.read(data, attributes=False)
        rows, err = got[0], got[-1]
        n = len(got[1]) if fmt == "gtf" else len(rows)
        v = Verdict(err[1], err[0], err[2], n, got) if err else Verdict(0, None, None, n, got)
    if v.code == E_INVALID_UTF8:
        assert first_ill_formed(fmt, data, v.record + 1) == v.record == v.n_rows, (fmt, v[:4])
    else:
        assert first_ill_formed(fmt, data, v.record if v.code else None) is None, (fmt, v[:4])
    return v


# ---------------------------------------------------------------- dense, well-formed files for the readers
ALPHABET = tuple(c.encode() for c in "é€😀ß中𝄞")          # 2, 3, 4, 2, 3 and 4 bytes
VCF_INFO_HDR = (b'##fileformat=VCFv4.2\n##INFO=<ID=S,Number=1,Type=String,Description="s">\n'
                b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")


def chars(n, seed):
    return b"".join(ALPHABET[(seed + i + i // 7) % 6] for i in range(n))


def file_head(fmt):
    return {"vcf": VCF_INFO_HDR, "sam": S.header()}.get(fmt, b"")


def _dense_record(fmt, i):
    u = chars
    if fmt == "fastq":           # (a shift of 3 in the alphabet keeps every character's length: sequence and quality are as long)
        return b"@" + u(6, i) + b" " + u(16 + i % 9, i + 1) + b"\n" + u(30 + i % 13, i + 2) + b"\n+\n" + u(30 + i % 13, i + 5) + b"\n"
    if fmt == "fasta":
        return b">" + u(5, i) + b" " + u(12 + i % 7, i + 1) + b"\n" + u(24, i + 2) + b"\n" + u(17 + i % 5, i + 4) + b"\n"
    if fmt == "vcf":
        return b"1\t%d\t" % (1000 + i) + u(4, i) + b"\tA\tC\t.\t.\tS=" + u(30 + i % 11, i + 1) + b"\n"
    if fmt == "bed":
        return b"chr1\t%d\t%d\t" % (1000 + i, 2000 + i) + u(28 + i % 9, i) + b"\n"
    if fmt == "sam":
        return u(8, i) + b"\t0\tchr1\t100\t60\t*\t*\t0\t0\t*\t*\tCO:Z:" + u(30 + i % 7, i + 1) + b"\tXS:Z:" + u(5, i + 2) + b"\n"
    return b"chr1\tsrc\texon\t%d\t%d\t.\t+\t.\t" % (1000 + i, 2000 + i) + b'gene_id "' + u(20, i) + b'"; note "' + u(20 + i % 5, i + 1) + b'";\n'


def dense(fmt, size=3 * SUPER + 5000):
    """a whole file of `fmt` (header included) of more than three super-tiles, more than half of its bytes in 2-, 3- and 4-byte
    characters: names, descriptions, sequences, qualities, ids, INFO strings, optional fields, attributes"""
    out, i = bytearray(file_head(fmt)), 0
    while len(out) < size:
        out += _dense_record(fmt, i)
        i += 1
    data = bytes(out)
    assert strict(data) and 2 * sum(b >= 0x80 for b in data) > len(data) and len(data) > 3 * SUPER
    return data


FASTQ_BASE = 0x7F0000000000     # the payload bases of test_fastq_gpu.py and test_vcf_gpu.py: the oracle's string_t views point there
VCF_BASE = 0x7E0000000000
