"""Fuzz inputs for the BED, SAM, BAM and BCF scans (helper, not collected): pure Python, no device, fixed seeds.

A case is addressed by (format, seed) and is a short list of inputs ("mutants", addressed by their index): case(fmt, seed);
reference(fmt, data) runs one input through the format's independent reader and returns an Outcome.  The GPU tests
(test_fuzz_records_gpu.py) hold the device to that reference; test_fuzz_records_host.py holds the INPUTS to what makes them
worth running — every record error of a format occurs, enough inputs are clean, enough errors have rows in front of them, and
no reference raises — so that the GPU tests cannot quietly test nothing.

Mutators.  BED and SAM are text: test_fuzz_gpu.mutate (separators into data and back, CRs, non-UTF-8, deletions, truncation) on
a base of a seed-dependent number of lines, plus a field mutator that swaps one field of one line for a token from a list of
near-misses (byte noise rarely writes `256,0,0` into a colour).  BAM and BCF are binary: a byte mutator (overwrite, bit flip,
delete 1-7, insert 1-4, truncate) and a field mutator that replaces one record of the base by one built through the writer's
own override parameters — a record that is consistent but wrong, with one fault or with two faults in different fields, in
either order."""
import functools
import random
import struct

import numpy as np

import bam_files as BAM
import bcf_files as BCF
import bed_files as BED
import sam_files as SAM

FORMATS = ("bed", "sam", "bam", "bcf")
SEEDS = range(48)
TILE = 32768


class Outcome:
    """what the reference says of one input: rows (BCF: lines) in front of the first error, error = None or (record ordinal,
    code, byte offset or None where the reference has none), consumed = where the scan stops"""

    def __init__(self, rows, error, consumed, extra=None):
        self.rows, self.error, self.consumed, self.extra = rows, error, consumed, extra

    @property
    def code(self):
        return self.error[1] if self.error else 0


def mutate(data, rng, n_mut):
    """test_fuzz_gpu.mutate: separators into data and back, CRs, non-UTF-8 bytes, deletions, truncation"""
    import test_fuzz_gpu
    return test_fuzz_gpu.mutate(data, rng, n_mut)


def mutate_binary(data, rng, n_mut):
    """overwrite a byte, flip a bit, delete 1-7 bytes, insert 1-4 random bytes, truncate (rarely: a truncated stream has one
    outcome)"""
    b = bytearray(data)
    for _ in range(n_mut):
        if not b:
            break
        kind = int(rng.integers(0, 17))
        pos = int(rng.integers(0, len(b)))
        if kind < 5:
            b[pos] = int(rng.integers(0, 256))
        elif kind < 10:
            b[pos] ^= 1 << int(rng.integers(0, 8))
        elif kind < 13:
            del b[pos:pos + int(rng.integers(1, 8))]
        elif kind < 16:
            b[pos:pos] = bytes(int(x) for x in rng.integers(0, 256, int(rng.integers(1, 5))))
        else:
            del b[max(pos, 1):]
    return bytes(b)


# ---------------------------------------------------------------- BED and SAM
BED_TOKENS = {0: [b""], 1: [b"x", b"-1", b"9" * 20, b""], 2: [b"0", b"1e3", b"%d" % 2 ** 63], 3: [b"", b"."], 4: [b".", b"1001", b"-5", b"00"],
              5: [b"*", b"", b"+-"], 6: [b"", b"x"], 7: [b"0", b"y"], 8: [b"256,0,0", b"1,2", b"1,2,3,4", b"", b"a,b,c"],
              9: [b"3", b"x", b"70"], 10: [b"1", b"a,b,c", b""], 11: [b"", b"1,x,3"]}
SAM_TOKENS = {0: [b"", b"@q", b"@"], 1: [b"65536", b"-1", b"+1", b"", b"x"], 2: [b"", b"*"], 3: [b"2147483648", b"-1", b"", b"1.5"],
              4: [b"256", b"-1", b"", b"q"], 5: [b"", b"M", b"10", b"10Q", b"268435456M", b"*"], 6: [b"", b"="], 7: [b""], 8: [b""],
              9: [b"", b"ACGT", b"*"], 10: [b"", b"II", b"*"]}


def mutate_field(data, rng, tokens, drop_fields_to):
    """one field of one line swapped for a near-miss, or the line cut to a field count the format does not take"""
    lines = data.split(b"\n")
    i = int(rng.integers(0, len(lines)))
    f = lines[i].split(b"\t")
    if int(rng.integers(0, 8)) == 0:
        f = f[:drop_fields_to]
    else:
        k = int(rng.integers(0, len(f)))
        if k in tokens:
            f[k] = tokens[k][int(rng.integers(0, len(tokens[k])))]
        elif f[k]:
            f[k] = f[k][:-1] + b"\xc3"          # (an aux field, a trailing field: bytes that are not UTF-8)
    lines[i] = b"\t".join(f)
    return b"\n".join(lines)


def _text_case(fmt, seed):
    rng = np.random.default_rng({"bed": 6000, "sam": 7000}[fmt] + seed)
    n_lines = int(rng.integers(3, 400))
    if fmt == "bed":
        base = BED.mixed(BED.rng(seed), n_lines, crlf_every=int(rng.integers(0, 9)), final_newline=bool(seed & 1))
        tokens, drop = BED_TOKENS, 10
    else:
        base = SAM.mixed(SAM.rng(seed), n_lines, crlf_every=int(rng.integers(0, 9)), final_newline=bool(seed & 1))
        tokens, drop = SAM_TOKENS, 10
    out = [mutate(base, rng, int(rng.integers(0, 4))), mutate_field(base, rng, tokens, drop)]
    out.append(mutate(mutate_field(base, rng, tokens, drop), rng, int(rng.integers(0, 3))))
    return [d or base for d in out]                     # (a truncation at byte 0 leaves nothing to scan)


def super_tile_case(fmt, k):
    """a base longer than one 32 KiB super-tile with one mutation at the super-tile boundary, -3 .. +3 bytes around it"""
    from test_fuzz_gpu import SPECIAL
    rng = np.random.default_rng(8000 + k)
    if fmt == "bed":
        base = BED.fill_to(BED.rng(100 + k), b"", TILE + 5000)
    else:
        base = SAM.fill_to(SAM.rng(100 + k), b"", TILE + 5000)
    out = []
    for delta in (-3, -1, 0, 1, 2):
        b = bytearray(base)
        pos = TILE + delta
        tok = SPECIAL[(k * 5 + delta + 3) % len(SPECIAL)]
        if (k + delta) % 3 == 0:
            b[pos:pos + 1] = tok
        elif (k + delta) % 3 == 1:
            b[pos:pos] = tok
        else:
            del b[pos:pos + int(rng.integers(1, 8))]
        out.append(bytes(b))
    return out


# ---------------------------------------------------------------- BAM
BAM_REFS = [(b"chr%d" % i, 250_000_000) for i in range(1, 23)] + [(b"chrX", 156_000_000), (b"a_decoy_contig_with_a_long_name", 5000)]
BAM_HEADER = BAM.header(BAM_REFS)


@functools.lru_cache(maxsize=None)
def bam_base():
    """600 short reads with the small records of test_bam_gpu.edge_records() spread among them: 6 tiles"""
    import test_bam_gpu
    recs = BAM.illumina_pairs(300, BAM_REFS, seed=31)
    edge = [r for r in test_bam_gpu.edge_records() if len(r) < 1000]
    for k, r in enumerate(edge):
        recs.insert(7 + 37 * k, r)
    return tuple(recs)


def offsets_of(recs):
    out, s = [], 0
    for r in recs:
        out.append(s)
        s += len(r)
    return out


def _bam_good(rng):
    n = int(rng.choice((0, 1, 13, 36, 150)))
    return dict(name=b"fz%d" % int(rng.integers(0, 10 ** 6)), flag=int(rng.integers(0, 4096)), ref=int(rng.integers(-1, len(BAM_REFS))),
                pos=int(rng.integers(-1, 10 ** 8)), mapq=int(rng.integers(0, 256)), cigar=[(n, "M")] if n else [(5, "H")],
                next_ref=int(rng.integers(-1, len(BAM_REFS))), next_pos=int(rng.integers(-1, 10 ** 8)),
                seq=bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, n)), qual=bytes(int(x) for x in rng.integers(0, 94, n)) if n else None,
                aux=BAM.aux_z(b"RG", b"grp1") if int(rng.integers(0, 2)) else b"")


def _bam_faults(rng, kw):
    """[(field group, overrides)]: the groups in the order a reader meets them"""
    n_ref, n = len(BAM_REFS), len(kw["seq"])
    size = len(BAM.record(**kw)) - 4
    seq_for_qual = kw["seq"] or b"A"
    qual = bytearray(kw["qual"] if n else b"\x1e")
    qual[int(rng.integers(0, len(qual)))] = int(rng.choice((0x5E, 0xFF)))
    ops = list(kw["cigar"]) + [(3, int(rng.integers(9, 16)))]
    rng.shuffle(ops)
    return [
        ("block_size", dict(block_size=int(rng.choice((0, 31, size - 1, size + 5, size - 20, 1 << 30))))),
        ("read_name", dict(l_read_name=int(rng.choice((0, len(kw["name"]), len(kw["name"]) + 2, 255))))),
        ("read_name", dict(raw_name=kw["name"] + b"!")),
        ("n_cigar", dict(n_cigar=int(rng.choice((60000, len(kw["cigar"]) + 1, 65535))))),
        ("l_seq", dict(l_seq=int(rng.choice((5000, -1, n + 7, 2 ** 31 - 1))))),
        ("ref", dict(ref=int(rng.choice((-2, n_ref, n_ref + 1, 2 ** 31 - 1, -2 ** 31))))),
        ("ref", dict(ref=int(rng.choice((-1, n_ref - 1))))),                      # (both ends, inside: no fault)
        ("next_ref", dict(next_ref=int(rng.choice((-2, n_ref, 2 ** 31 - 1, -2 ** 31))))),
        ("cigar", dict(cigar=[(int(ln), op) for ln, op in ops])),
        ("qual", dict(seq=seq_for_qual, qual=bytes(qual))),
    ]


def _bam_field_mutant(rng, two):
    recs = list(bam_base())
    i = int(rng.integers(0, len(recs)))
    kw = _bam_good(rng)
    faults = _bam_faults(rng, kw)
    a = faults[int(rng.integers(0, len(faults)))]
    over = dict(a[1])
    if two:
        others = [f for f in faults if f[0] != a[0] and not (set(f[1]) & set(over))]
        over.update(others[int(rng.integers(0, len(others)))][1])
    recs[i] = BAM.record(**dict(kw, **over))
    return b"".join(recs)


def _bam_case(seed):
    rng = np.random.default_rng(9000 + seed)
    base = b"".join(bam_base())
    return [mutate_binary(base, rng, int(rng.integers(0, 4))), mutate_binary(base, rng, int(rng.integers(1, 3))),
            _bam_field_mutant(rng, two=False), _bam_field_mutant(rng, two=True)]


def bam_reference(stream):
    p = BAM.parse_decoded(BAM_HEADER + stream)
    s = 0
    for _ in p.rows:                                         # where record k begins: the chain of block sizes
        s += 4 + struct.unpack_from("<I", stream, s)[0]
    err = None if p.error is None else (p.error[0], p.error[1], s)
    return Outcome(p.rows, err, s if err else len(stream))


# ---------------------------------------------------------------- BCF
@functools.lru_cache(maxsize=None)
def bcf_text():
    import test_bcf_gpu
    return test_bcf_gpu.header(samples=test_bcf_gpu.SAMPLES3)


@functools.lru_cache(maxsize=None)
def bcf_dicts():
    return BCF.dictionaries(bcf_text())


@functools.lru_cache(maxsize=None)
def bcf_base():
    """500 three-sample cohort records (300 are 45 KB: two tiles) with the first eight of every_form among them: 3 tiles"""
    import test_bcf_gpu
    text = bcf_text()
    recs = test_bcf_gpu.cohort(text, 500, 3)
    for k, r in enumerate(test_bcf_gpu.every_form(text, 3)[:8]):
        recs.insert(5 + 60 * k, r)
    return tuple(recs)


def _reserved(rng, width):
    """one of the six reserved values of an integer width (missing + 2 .. + 7), as bytes"""
    return struct.pack(BCF.PACK[width], BCF.INT_MISSING[width] + int(rng.integers(2, 8)))


def _bad_value(rng):
    """a typed value a reader refuses, or one it must take in its stride: types 0, 4, 6, 8-15; long-form counts that are
    negative, zero or larger than the record; each reserved integer in each width"""
    kind = int(rng.integers(0, 6))
    if kind == 0:
        t = int(rng.choice((4, 6, 8, 9, 10, 11, 12, 13, 14, 15)))
        return BCF.raw_value(t, int(rng.integers(0, 3)), b"\0" * 8)
    if kind == 1:
        return BCF.raw_value(0, int(rng.integers(1, 15)), b"")                   # type 0 with a count: no data, `.`
    if kind == 2:
        t = int(rng.choice((1, 2, 3, 5, 7)))
        return BCF.raw_value(t, int(rng.choice((-1, -128, -40000))), b"", long_form=True)
    if kind == 3:
        return BCF.raw_value(int(rng.choice((1, 2, 3, 5, 7))), 0, b"", long_form=True)
    if kind == 4:
        return BCF.raw_value(int(rng.choice((1, 2, 3, 5, 7))), int(rng.choice((200, 40000, 2 ** 31 - 1))), b"abc", long_form=True)
    w = int(rng.integers(1, 4))
    n, at = int(rng.choice((1, 3, 20, 100))), 0
    vals = [struct.pack(BCF.PACK[w], int(rng.integers(0, 100))) for _ in range(n)]
    at = int(rng.integers(0, n))
    vals[at] = _reserved(rng, w)
    if int(rng.integers(0, 4)) == 0 and at:                                     # behind an end-of-vector: not an error
        vals[int(rng.integers(0, at))] = struct.pack(BCF.PACK[w], BCF.INT_MISSING[w] + 1)
    return BCF.raw_value(w, n, b"".join(vals), long_form=n >= 15)


def _bcf_good(rng, text):
    import test_bcf_gpu
    k = lambda name: test_bcf_gpu.K(text, name)
    info = [(k("DP"), BCF.ints([int(rng.integers(0, 5000))])), (k("AF"), BCF.floats([0.25])), (k("DB"), BCF.flag()),
            (k("STR"), BCF.chars(b"tandem"))][:int(rng.integers(1, 5))]
    return dict(chrom=int(rng.integers(0, 3)), pos=int(rng.integers(0, 10 ** 8)), id_=b"rs%d" % int(rng.integers(0, 999)),
                alleles=[b"A", b"G", b"<DEL>"][:int(rng.integers(1, 4))], qual=30.0, filters=[[0], None, [k("q10"), k("s50")]][int(rng.integers(0, 3))],
                info=info, n_sample=3, fmt=test_bcf_gpu.default_fmt(text, 3, random.Random(int(rng.integers(0, 1 << 30)))))


def _bcf_faults(rng, text, kw):
    """[(field group, function(kw) -> kw)]: the groups in the order a reader meets them; `info` and `fmt` faults are placed at a
    random entry, so that two of them fall in either order"""
    import test_bcf_gpu
    n_str = len(bcf_dicts()[0])
    k = lambda name: test_bcf_gpu.K(text, name)
    size = len(BCF.record(**kw))
    l_shared, l_indiv = struct.unpack_from("<II", BCF.record(**kw))

    def info_with(entry):
        def f(d):
            info = list(d["info"])
            info.insert(int(rng.integers(0, len(info) + 1)), entry)
            return dict(d, info=info)
        return f

    def fmt_with(key, values):
        def f(d):
            fmt = list(d["fmt"])
            fmt.insert(int(rng.integers(0, len(fmt) + 1)), (key, values))
            return dict(d, fmt=fmt)
        return f

    def sample_value():
        w, vals = int(rng.integers(1, 4)), []
        bad = int(rng.integers(0, 3))
        for s in range(3):
            v = [struct.pack(BCF.PACK[w], int(rng.integers(0, 90))) for _ in range(2)]
            if s == bad:
                v[int(rng.integers(0, 2))] = _reserved(rng, w)
            vals.append(BCF.raw_value(w, 2, b"".join(v)))
        return vals

    bad_filter = [BCF.raw_value(1, 1, bytes([n_str])), BCF.raw_value(2, 2, struct.pack("<hh", 0, -1)), BCF.raw_value(1, 2, bytes([0, 0x83])),
                  BCF.raw_value(int(rng.choice((4, 5, 6, 7, 9, 15))), 1, b"\0\0\0\0"), BCF.raw_value(0, 3, b""),
                  BCF.raw_value(1, int(rng.choice((-1, 0, 40000))), b"", long_form=True), BCF.raw_value(3, 1, struct.pack("<i", 2 ** 31 - 1))]
    bad_key = [n_str, n_str + 5, -1, 2 ** 31 - 1, bytes([0x16, 1]), bytes([0x21, 1, 0]), bytes([0x15, 0, 0, 0, 0])]
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]
    t_bad, n_long = int(rng.choice((4, 6, 8, 12, 15))), int(rng.choice((-1, 30000)))
    return [
        ("fixed", lambda d: dict(d, chrom=int(rng.choice((3, -1, 2 ** 31 - 1))))),
        ("fixed", lambda d: dict(d, n_allele=int(rng.choice((0, len(d["alleles"]) + 1, len(d["alleles"]) - 1 or 5))))),
        ("fixed", lambda d: dict(d, n_sample_field=int(rng.choice((2, 4, 0, 0xFFFFFF))))),
        ("lengths", lambda d: dict(d, l_shared=int(rng.choice((23, 0, l_shared - 1, l_shared - 9, l_shared + 3, 24))))),
        ("lengths", lambda d: dict(d, l_indiv=int(rng.choice((9, 0, l_indiv - 1, l_indiv + 4, size * 400))))),
        ("filter", lambda d: dict(d, filter_value=pick(bad_filter))),
        ("info", info_with((k("BIG"), _bad_value(rng)))),
        ("info", info_with((k("BIG"), _bad_value(rng)))),
        ("info", info_with((pick(bad_key), BCF.ints([1])))),
        ("fmt", fmt_with(k("GQ"), sample_value())),
        ("fmt", fmt_with(k("GT"), [BCF.ints([2, int(rng.choice((-3, 4)))], width=1) for _ in range(3)])),
        ("fmt", fmt_with(pick(bad_key), [BCF.ints([1]) for _ in range(3)])),
        ("fmt", fmt_with(k("PL"), [BCF.raw_value(t_bad, 1, b"\0") for _ in range(3)])),
        ("fmt", fmt_with(k("PL"), [BCF.raw_value(0, 2, b"") for _ in range(3)])),
        ("fmt", fmt_with(k("PL"), [BCF.raw_value(2, n_long, b"", long_form=True) for _ in range(3)])),
    ]


def _bcf_field_mutant(rng, two):
    text = bcf_text()
    recs = list(bcf_base())
    i = int(rng.integers(0, len(recs)))
    kw = _bcf_good(rng, text)
    faults = _bcf_faults(rng, text, kw)
    a = faults[int(rng.integers(0, len(faults)))]
    chosen = [a]
    if two:
        # two faults in different fields; two INFO (or two FORMAT) entries count as different fields: they fall in either order
        others = [f for f in faults if f is not a and (f[0] != a[0] or f[0] in ("info", "fmt"))]
        chosen.append(others[int(rng.integers(0, len(others)))])
        if int(rng.integers(0, 2)):
            chosen.reverse()
    for _, f in chosen:
        kw = f(kw)
    recs[i] = BCF.record(**kw)
    return b"".join(recs)


def _id_type_mutant(rng):
    """the type nibble of one record's ID (or first allele) descriptor overwritten: a value of type 0 with a count, a string of
    type 1, ..."""
    recs = bcf_base()
    offs = offsets_of(recs)
    b = bytearray(b"".join(recs))
    i = int(rng.integers(0, len(recs)))
    at = offs[i] + 32
    if int(rng.integers(0, 2)):
        at += 1 + (b[at] >> 4) if b[at] >> 4 < 15 else 0          # the first allele's descriptor (behind a short-form ID)
    b[at] = (b[at] & 0xF0) | int(rng.choice((0, 0, 1, 5, 4)))
    return bytes(b)


def _bcf_case(seed):
    rng = np.random.default_rng(10000 + seed)
    base = b"".join(bcf_base())
    third = _id_type_mutant(rng) if seed % 4 == 0 else _bcf_field_mutant(rng, two=False)
    return [mutate_binary(base, rng, int(rng.integers(0, 4))), mutate_binary(base, rng, int(rng.integers(1, 3))),
            third, _bcf_field_mutant(rng, two=True)]


def bcf_reference(records):
    strings, contigs, n_samples = bcf_dicts()
    r = BCF.Rendered(records, strings, contigs, n_samples)
    return Outcome(r.lines, r.error, r.consumed, r)


# ---------------------------------------------------------------- the cases
def case(fmt, seed):
    """the inputs of case (fmt, seed): a list of bytes, addressed by their index (the mutant index)"""
    if fmt in ("bed", "sam"):
        return _text_case(fmt, seed)
    return _bam_case(seed) if fmt == "bam" else _bcf_case(seed)


def reference(fmt, data):
    if fmt == "bed":
        rows, err = BED.read(data)
    elif fmt == "sam":
        rows, err = SAM.read(data)
    elif fmt == "bam":
        return bam_reference(data)
    else:
        return bcf_reference(data)
    return Outcome(rows, err, err[2] if err else len(data))


def error_codes(fmt):
    """every record error of a format"""
    return {"bed": [BED.E_INVALID_UTF8] + list(range(BED.E_FIELD_COUNT, BED.E_BLOCKS + 1)),
            "sam": [SAM.E_INVALID_UTF8] + list(range(SAM.E_FIELD_COUNT, SAM.E_LENGTHS + 1)),
            "bam": list(range(BAM.E_BLOCK_SIZE, BAM.E_QUALITY + 1)),
            "bcf": list(range(BCF.E_RECORD_LENGTH, BCF.E_SAMPLE_COUNT + 1))}[fmt]
