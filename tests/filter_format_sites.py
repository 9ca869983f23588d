"""The edge files of tests/test_filters_formats_gpu.py and tests/test_filters_formats_host.py (helper, not collected): GTF, FASTA
and BCF files of 333 rows each, built so that every filterable column carries the values at which a comparison goes wrong, with
the rows an independent reader gives for them — gtf_files.read, oracle.fasta_parse, and oracle.vcf_parse over the VCF text that
bcf_files' renderer makes of the BCF records.  Nothing here touches the device: a Site is a path, rows and literals.

List lengths: columns that are to be told apart cycle with coprime periods (11, 7, 9, 5, 4, 17 for GTF), as vcf_bytes() does."""
import math
import struct

import bcf_files as BCF
import gtf_files as G
import test_filters_gpu as TF

N_ROWS = TF.N_ROWS
I63 = 2 ** 63 - 1
# (number of random trees, seed) of every test that draws some; tests/test_filters_formats_host.py holds each to the 80 % of
# check_trees with keep() alone
TREES = {"gtf": (80, 5), "fasta": (80, 6), "fasta new_reader": (80, 7), "bcf": (80, 8), "fastq shard": (80, 9),
         "gtf zst": (24, 10), "gtf gz": (24, 11), "fasta gz": (24, 12), "fasta bz2": (24, 13), "gtf shards": (24, 14), "fasta shards": (24, 16)}     # (seed 15 gives FASTA 19 of 24: below the 80 %)


def int_literals(values):
    """every value, its two neighbours (inside int64), and literals that make an integer column compare as float64"""
    out = set()
    for v in values:
        out |= {x for x in (v - 1, v, v + 1) if -2 ** 63 <= x <= I63}
    return [str(v) for v in sorted(out | {-1})] + ["4.5", "9007199254740992.0", "9007199254740993.0", "1e10"]


def f32_of(text):
    return TF.fo.f32(float(text))


def f32_neighbours(x):
    """the float32 below and the one above x (finite ones only)"""
    bits = struct.unpack("<I", struct.pack("<f", x))[0]
    out = []
    for step in (-1, 1):
        if bits & 0x7FFFFFFF == 0:
            b = (0x80000001 if step < 0 else 0x00000001)
        elif bits >> 31:
            b = bits - step
        else:
            b = bits + step
        y = struct.unpack("<f", struct.pack("<I", b))[0]
        if math.isfinite(y):
            out.append(y)
    return out


def float_literals(texts, more=()):
    """the finite values as the file spells them, the float32 on either side of each (nine digits: they read back exactly), `more`"""
    out = []
    for t in texts:
        x = f32_of(t)
        if not math.isfinite(x):
            continue
        out.append(t)
        out += ["%.9g" % y for y in f32_neighbours(x)]
    seen, uniq = set(), []
    for t in out + list(more):
        if t not in seen:
            seen.add(t)
            uniq.append(t)
    return uniq


# ---- GTF ---------------------------------------------------------------------------------------------------------------------
GTF_SEQNAMES = TF.VCF_CHROMS                                                   # 11: lengths 1, 4, 11, 12, 13, 300; pairs that differ at byte 5, at byte 13, in length; UTF-8
GTF_SOURCES = [b"havana", b"ensembl_havana", b"ensembl_havaNA", b"."]          # "ensembl_hava": a shared prefix of 12 bytes; "." is a string here, not NULL
GTF_TYPES = [b"exon", b"CDS", b"five_prime_utr", b"five_prime_uTR", b"gene"]   # "five_prime_u": the same
GTF_STARTS = [1, 2 ** 31 - 1, 2 ** 31, 2 ** 53, 2 ** 53 + 1, I63, 5]            # 2^63 - 1: the largest the scan accepts
GTF_ENDS = [1, 2 ** 31 - 1, 2 ** 31, 2 ** 53, 2 ** 53 + 1, I63, 4, I63 - 1, 100]  # (neither reader orders start and end)
GTF_SCORES = [b".", b"0", b"-0", b"0.1", b"-0.1", b"0.5", b"1e-45", b"-1e-45", b"3.4028235e38", b"-3.4028235e38", b"inf", b"-inf", b"nan", b"16777216",
              b"16777217", b"-1.5", b"0.3"]                                    # 17
GTF_STRANDS = [b"+", b"-", b"."]
GTF_FRAMES = [b"0", b"1", b"2", b"."]
GTF_FLAT = G.NAMES[:8]
GTF_SCHEMA = {"seqname": "u", "source": "u", "type": "u", "start": "l", "end": "l", "score": "f", "strand": "u", "frame": "u"}
GTF_LITERALS = {
    "seqname": TF.string_literals(GTF_SEQNAMES),
    "source": TF.string_literals(GTF_SOURCES),
    "type": TF.string_literals(GTF_TYPES),
    "start": int_literals(GTF_STARTS),
    "end": int_literals(GTF_ENDS),
    # (`inf` and `nan` are no literals: the grammar refuses them, tests/test_filter_parse.py REFUSED)
    "score": float_literals([s.decode() for s in GTF_SCORES if s != b"."], more=["-0", "0.30000001", "5", "-5"]),
    "strand": [b"+", b"-", b"", b"+ ", b"."],
    "frame": [b"0", b"1", b"2", b"", b"0 ", b"."],
}
# lines that are comments, by their ordinal among all lines; the file's last line is one more
GTF_RUN70 = range(126, 196)                      # 70 lines: bits 126, 127 of keep word 1, all of word 2, bits 0..3 of word 3
GTF_LONG_RUN = range(320, 480)                   # 160 lines of 90 bytes: 14 kB, several device batches of 4 096 bytes without a row; word 4 stays full
GTF_COMMENTS = {0, 1, 63, 64, 65} | set(GTF_RUN70) | set(GTF_LONG_RUN)


def gtf_bytes():
    rng = G.rng(77)
    lines, r = [], 0
    while r < N_ROWS:
        k = len(lines)
        if k in GTF_COMMENTS:
            lines.append(b"#" if k == 64 else b"#!long-run %03d " % k + b"x" * 72 if k in GTF_LONG_RUN else b"#!c%d" % k)
            continue
        attrs = G.attributes(rng, n_entries=rng.randrange(2, 7), tags=0)
        if r % 50 == 7:
            attrs = b'note "5; prime  end ; see x"; ' + G.attributes(rng, n_entries=rng.randrange(1, 6), tags=0)
        lines.append(b"\t".join([GTF_SEQNAMES[r % 11], GTF_SOURCES[r % 4], GTF_TYPES[r % 5], b"%d" % GTF_STARTS[r % 7], b"%d" % GTF_ENDS[r % 9],
                                 GTF_SCORES[r % 17], GTF_STRANDS[(r // 4) % 3], GTF_FRAMES[(r // 3) % 4], attrs]))
        r += 1
    lines.append(b"#the last line")
    return b"".join(ln + (b"\r\n" if k % 7 == 6 else b"\n") for k, ln in enumerate(lines))


def gtf_rows(data):
    rows, keep, err = G.read(data)
    assert err is None, err
    return [dict(zip(G.NAMES, G.user_row(r))) for r in rows], keep


def gtf_site(path, data=None):
    """(the Site, keep): `path` is written unless `data` is given (a copy in another encoding: the rows are `data`'s)"""
    if data is None:
        data = gtf_bytes()
        with open(path, "wb") as f:
            f.write(data)
    rows, keep = gtf_rows(data)
    return TF.Site(path, "gtf", "read_gtf", G.NAMES, GTF_FLAT, GTF_SCHEMA, rows, GTF_LITERALS, beside=["attributes"]), keep


def gtf_row_selector(site, k):
    """(seqname, start, type) cycle with 11, 7 and 5: they name one row of the first 385"""
    r = site.rows[k]
    return TF.and_(TF.cmp("seqname", "=", r["seqname"]), TF.cmp("start", "=", str(r["start"])), TF.cmp("type", "=", r["type"]))


def gtf_row_of_line(keep, line):
    """the row index of the feature line with ordinal `line`"""
    assert keep[line]
    return sum(keep[:line])


# ---- FASTA -------------------------------------------------------------------------------------------------------------------
def _seq(seed, n):
    rng = G.rng(seed)
    return bytes(rng.choice(b"ACGT") for _ in range(n))


_L300 = _seq(1, 300)
_P120 = _seq(2, 120)
FA_IDS = TF.FQ_NAMES                                                           # 11
FA_DESCS = [None, b"", b"d", b"0123456789ab", b"0123456789abc", b"D" * 300, b"desc with space"]      # 7 (b"": `>id ` with nothing behind the blank)
FA_SEQS = [b"A", b"ACGT", b"ACGTACGTACGT", b"ACGTACGTACGTA", b"ACGTACGTACGTC",             # 1, 4, 12, 13 and 13 bytes, the last two differ in the last byte
           _L300, _L300[:240] + bytes([_L300[240] ^ 6]) + _L300[241:],                     # five lines of 60; the second differs in the first byte of its last line
           _P120, _P120 + _seq(3, 60)]                                                     # a proper prefix that ends where two lines are joined; 9 values
FA_FLAT = ["id", "description", "sequence"]
FA_SCHEMA = dict.fromkeys(FA_FLAT, "u")
FA_LITERALS = {"id": TF.string_literals(FA_IDS), "description": TF.string_literals([d for d in FA_DESCS if d]), "sequence": TF.string_literals(FA_SEQS)}


def fasta_bytes():
    out = []
    for r in range(N_ROWS):
        name, desc, seq = FA_IDS[r % 11], FA_DESCS[r % 7], FA_SEQS[r % 9]
        nl = b"\r\n" if r % 3 == 0 else b"\n"
        out.append(b">" + name + (b"" if desc is None else b" " + desc) + nl + b"".join(seq[k:k + 60] + nl for k in range(0, len(seq), 60)))
    return b"".join(out)


def fasta_rows(oracle, data):
    res = oracle.fasta_parse(data)
    assert res.error_code == 0, (res.error_code, res.error_message)
    cols = [res.columns[k].to_list() for k in FA_FLAT]
    return [dict(zip(FA_FLAT, t)) for t in zip(*cols)]


def fasta_site(oracle, path, data=None):
    if data is None:
        data = fasta_bytes()
        with open(path, "wb") as f:
            f.write(data)
    return TF.Site(path, "fasta", "read_fasta", FA_FLAT, FA_FLAT, FA_SCHEMA, fasta_rows(oracle, data), FA_LITERALS)


# ---- BCF ---------------------------------------------------------------------------------------------------------------------
BCF_CONTIGS = [b"1", b"chr1", b"chr1_random", b"chr1_randomA", b"chr1_randomAB", b"chr1_randomAC", b"chr1Xrandom", b"L" * 300, b"L" * 299 + b"M"]    # 9, ASCII
BCF_POS0 = [-1, 0, 4, 2 ** 31 - 3, 2 ** 31 - 2, 2 ** 31 - 1, 99999]            # the record's 0-based int32; POS = pos + 1: 0 .. 2^31
BCF_REFS = TF.VCF_REFS                                                         # 1, 4, 12, 13 and 300 bytes
# FLOAT_EDGES of tests/test_bcf_gpu.py, and missing.  Left out, because the VCF rule "QUAL is a non-negative float" (a negative
# QUAL, -inf included, is a parse error of the VCF reader: tests/test_filters_gpu.py) makes the record's line an error, not a row:
#   0x807FFFFF (-1.17549421e-38), 0xFF7FFFFF (-3.40282347e+38), 0xFF800000 (-inf).   0x80000000 (-0) stays: it is not below zero.
BCF_QUAL_REFUSED = [0x807FFFFF, 0xFF7FFFFF, 0xFF800000]
BCF_QUAL_BITS = [0x00000000, 0x80000000, 0x00000001, 0x00800000, 0x7F7FFFFF, 0x3F800000, 0x3DCCCCCD, 0x7F800000, 0x7FC00000, 0x7F800003, 0x501502F9, 0x2EDBE6FF,
                 0x4B800000, 0x461C4000]
BCF_QUALS = [BCF.MISSING] + [("bits", b) for b in BCF_QUAL_BITS]               # 15
BCF_INFOS = [("DP", "1", "Integer")]


def bcf_header():
    return BCF.header_text(contigs=tuple(c.decode() for c in BCF_CONTIGS), infos=BCF_INFOS)


def bcf_records(quals=None):
    text = bcf_header()
    dp = BCF.dictionaries(text)[0].index(b"DP")
    quals = BCF_QUALS if quals is None else quals
    return [BCF.record(chrom=r % 9, pos=BCF_POS0[r % 7], alleles=(BCF_REFS[r % 5], b"C"), qual=quals[r % len(quals)], info=[(dp, BCF.ints([r]))])
            for r in range(N_ROWS)]


def bcf_as_vcf(records):
    """the VCF text the independent renderer makes of the records (header included), and the renderer's error"""
    text = bcf_header()
    strings, contigs, n_samples = BCF.dictionaries(text)
    rendered = BCF.Rendered(b"".join(records), strings, contigs, n_samples)
    return text + rendered.text, rendered.error


def bcf_literals():
    quals = [BCF.fmt_float(b).decode() for b in BCF_QUAL_BITS]
    return {"chrom": TF.string_literals(BCF_CONTIGS), "ref": TF.VCF_LITERALS["ref"],
            "pos": int_literals([p + 1 for p in BCF_POS0]) + ["2147483648.5"],
            "qual": float_literals(quals, more=["-0", "5", "0.30000001", "-1.5", "-3.4028235e38"])}


def bcf_site(oracle, path):
    records = bcf_records()
    with open(path, "wb") as f:
        f.write(BCF.bgzf_file(bcf_header(), records, member_bytes=1500))      # records straddle the BGZF members
    vcf, err = bcf_as_vcf(records)
    assert err is None, err
    return TF.Site(path, "bcf", "read_bcf_file_records", oracle.VCF_FIELDS, TF.VCF_FLAT, TF.VCF_SCHEMA, TF.vcf_oracle_rows(oracle, vcf), bcf_literals())
