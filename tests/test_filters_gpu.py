"""Pushed-down `filters` on the device against DuckDB's semantics (tests/filter_oracle.py), at the three places that feed the
row predicate: exg_rd_batch.cpp (VCF through ShardReader and the table function), exg_arrow_stream.cpp (FASTQ and VCF through
new_reader) and exg_rd_bam.cpp (BAM through ShardReader and the table function).  DuckDB does not evaluate a pushed filter
again, so a wrong row here is a silently wrong query result.

Each file has 333 rows (not a multiple of 64) and is read with the default device batch and with EXG_DEVICE_BATCH_BYTES=4096,
the floor, which spreads the selection over several device batches and validity words.  The expected rows come from
oracle.pyoracle / bam_files.parse_decoded and filter_oracle.keep(), never from the reader under test.

What the formats leave out of the edge sets: a negative VCF QUAL, `-inf` included, is a parse error (the file has `-0` only), CHROM / REF must be
valid UTF-8 (bytes >= 0x80 appear as two-byte sequences, and literals cut them in the middle), the nested VCF columns (INFO
among them) are not filterable, a BAM flag is 16 bits wide (65535 stands in for INT32_MAX) and a BAM start is never 0.
Literals: every distinct value of the column, every proper prefix of the strings of up to 13 bytes (of the 300-byte ones: the
prefixes of 1, 4, 11, 12, 13 and 299 bytes — the comparison has one loop and no path that depends on the length beyond
inlined / out-of-line), and every string extended by one byte."""
import math
import random
import struct
import time

import pytest

import bam_files as B
import filter_oracle as fo
from filter_oracle import and_, cmp, isnull, notnull, or_

pytestmark = pytest.mark.gpu

N_ROWS = 333
SMALL_BATCH = "4096"
N_TREES = 150
INT32_MAX = 2 ** 31 - 1


def norm(v):
    """a value as something == compares exactly: floats by their float32 bits, every NaN the same"""
    if isinstance(v, float):
        return ("nan",) if math.isnan(v) else ("f", struct.pack("<f", v))
    if isinstance(v, str):
        return v.encode()
    return v


def norm_rows(rows):
    return [tuple(norm(v) for v in r) for r in rows]


def string_literals(values):
    out = []
    for s in values:
        cuts = range(len(s)) if len(s) <= 13 else (1, 4, 11, 12, 13, len(s) - 1)
        out += [s] + [s[:k] for k in cuts] + [s + b" "]
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


# ---- the three files ---------------------------------------------------------------------------------------------------------
VCF_CHROMS = [b"1", b"chr1", b"chr1_random", b"chr1_randomA", b"chr1_randomAB", b"chr1_randomAC", b"chr1Xrandom", b"chr\xc3\xa9", b"\xc3\xa9",
              b"L" * 300, b"L" * 299 + b"M"]                                  # lengths 1, 4, 11, 12, 13, 300; pairs that differ at byte 5, at byte 13, in length
VCF_POS = [1, 2147483647, 2147483648, 9007199254740992, 9007199254740993, 2 ** 63 - 1, 5]       # 2^63 - 1: the largest the scan accepts
VCF_REFS = [b"A", b"ACGT", b"ACGTACGTACGT", b"ACGTACGTACGTA", b"N" * 300]
VCF_QUALS = [b".", b"0", b"-0", b"0.1", b"0.5", b"1e-45", b"3.4028235e38", b"inf", b"nan", b"16777216", b"16777217", b"50.5", b"1.5"]
VCF_INFOS = [b"DP=1", b".", b"DP=12345678", b"DP=123456789"]
VCF_HEADER = (b"##fileformat=VCFv4.2\n##INFO=<ID=DP,Number=1,Type=Integer,Description=\"depth\">\n"
              b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
VCF_FLAT = ["chrom", "pos", "ref", "qual"]                                      # the filterable columns (the others are nested)
VCF_SCHEMA = {"chrom": "u", "pos": "l", "ref": "u", "qual": "f"}
VCF_LITERALS = {
    "chrom": string_literals(VCF_CHROMS),
    "ref": string_literals(VCF_REFS),
    "pos": [str(v) for v in VCF_POS] + ["0", "2", "2147483649", "9223372036854775806", "9007199254740992.0", "9007199254740993.0", "4.5", "1e10"],
    "qual": ["0", "-0", "0.1", "0.5", "1e-45", "3.4028235e38", "16777216", "16777217", "50.5", "1.5", "-1.5", "5", "0.30000001", "-3.4028235e38"],
}


def vcf_bytes():
    # 11, 7 and 5 are coprime: (chrom, pos, ref) names one row of the first 385
    lines = [b"\t".join([VCF_CHROMS[r % 11], str(VCF_POS[r % 7]).encode(), b".", VCF_REFS[r % 5], b"C", VCF_QUALS[r % 13], b"PASS", VCF_INFOS[r % 4]]) + b"\n"
             for r in range(N_ROWS)]
    return VCF_HEADER + b"".join(lines)


def vcf_oracle_rows(oracle, data):
    res = oracle.vcf_parse(data, want_string_t=False)
    assert res.error_code == 0 and res.n_rows == N_ROWS, (res.error_code, res.error_message, res.n_rows)
    chrom, ref = res.columns["chrom"].to_list(), res.columns["ref"].to_list()
    pos, qual, ok = res.extra["pos"].tolist(), res.extra["qual"].tolist(), res.extra["qual_valid"].tolist()
    return [{"chrom": chrom[k], "pos": pos[k], "ref": ref[k], "qual": qual[k] if ok[k] else None} for k in range(N_ROWS)]


FQ_NAMES = [b"a", b"abcd", b"read_prefix_A", b"read_prefix_B", b"read_prefix_AB", b"read_prefix", b"read_prefix_", b"r\xc3\xa9ad", b"N" * 300, b"read_prefix_A1",
            b"read_pRefix_A"]
FQ_DESCS = [None, b"d", b"desc with space", b"0123456789abc", None, b"0123456789ab", b"it's"]
FQ_SEQS = [b"ACGT", b"A", b"ACGTACGTACGTA", b"ACGTACGTACGTC", b"GGGGGGGGGGGG"]
FQ_FLAT = ["name", "description", "sequence", "quality_scores"]
FQ_SCHEMA = dict.fromkeys(FQ_FLAT, "u")
FQ_LITERALS = {"name": string_literals(FQ_NAMES), "description": string_literals([d for d in FQ_DESCS if d is not None]),
               "sequence": string_literals(FQ_SEQS)}


def fastq_bytes():
    out = []
    for r in range(N_ROWS):
        name, desc, seq = FQ_NAMES[r % 11], FQ_DESCS[r % 7], FQ_SEQS[r % 5]
        out.append(b"@" + name + (b"" if desc is None else b" " + desc) + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
    return b"".join(out)


def fastq_oracle_rows(oracle, data):
    res = oracle.fastq_parse(data, want_string_t=False)
    assert res.error_code == 0 and res.n_rows == N_ROWS
    cols = [res.columns[k].to_list() for k in FQ_FLAT]
    return [dict(zip(FQ_FLAT, t)) for t in zip(*cols)]


BAM_REFS = [(b"chr1", 2 ** 31 - 1), (b"chr1_random_x", 1000), (b"chr1_random_y", 1000), (b"c", 5)]
BAM_POS = [-1, 0, 1, 3, 8, 99, INT32_MAX - 1]                                  # start = pos + 1: NULL, 1, 2, 4, 9, 100, INT32_MAX
BAM_FLAGS = [0, 1, 99, 65535, 4]
BAM_CIGARS = [(), ((1, "M"),), ((10, "M"),), ((5, "M"), (3, "D"))]
BAM_MAPQ = [255, 0, 60, 7, 255, 100]
BAM_REF_IDS = [-1, 0, 1, 2, 3, 0, -1, 1, 2]
BAM_MATE_IDS = [-1, 1, 0, 3, -1, 2, 0]                                        # mate_reference: NULL and each reference, apart from `reference`
BAM_SEQS = [b"A", b"AC", b"ACG", b"ACGT", b"ACGTN", b"", b"ACGTACGTACGTA", b"ACGTACGTACGTC"]
BAM_NAMES = [b"q", b"read_prefix_A", b"read_prefix_B", b"read_prefix_AB", b"r" * 200]
BAM_FLAT = list(B.NAMES)                                                       # all ten columns are filterable
BAM_SCHEMA = {n: "i" if t == "INTEGER" else "u" for n, t in zip(B.NAMES, B.TYPES)}
BAM_LITERALS = {
    "name": string_literals(BAM_NAMES),
    "reference": string_literals([n for n, _ in BAM_REFS]),
    "mapping_quality": [b"0", b"60", b"7", b"100", b"", b"6", b"600", b"255"],
    "flag": ["0", "1", "99", "65535", "4", "65536", str(INT32_MAX), "-1", "98.5"],
    "start": ["0", "1", "2", "4", "5", "9", "100", str(INT32_MAX), str(INT32_MAX - 1), "2147483648", "8.5"],
    "end": ["0", "1", "2", "4", "8", "11", "109", str(INT32_MAX), str(INT32_MAX - 1), "2147483648", "-1"],
    "mate_reference": string_literals([n for n, _ in BAM_REFS]),
    "cigar": [b"", b"1M", b"10M", b"5M3D", b"5M", b"1", b"5M3D "],
    "sequence": string_literals(BAM_SEQS),
    "quality_score": [b"", b"?", b"??", b"?????", b"I", b"?I", b"?" * 13, b"?" * 12],
}


def bam_qual(r):
    n = len(BAM_SEQS[r % 8])
    return None if r % 11 == 0 or n == 0 else bytes([30] * (n - 1) + [40 if r % 2 else 30])      # absent (""), "??..?" or "??..I"


def bam_raw():
    recs = [B.record(name=BAM_NAMES[r % 5] + (b"" if r % 3 else b"/%d" % r), flag=BAM_FLAGS[r % 5], ref=BAM_REF_IDS[r % 9], pos=BAM_POS[r % 7],
                     mapq=BAM_MAPQ[r % 6], cigar=BAM_CIGARS[r % 4], next_ref=BAM_MATE_IDS[r % 7], seq=BAM_SEQS[r % 8],
                     qual=bam_qual(r))
            for r in range(N_ROWS)]
    return B.header(BAM_REFS) + b"".join(recs)


class Site:
    """one file and the ways to read it"""

    def __init__(self, path, fmt, fn, names, flat, schema, rows, literals, beside=()):
        """flat: the filterable columns; beside: columns that are read and compared with them but never named in a filter (GTF's
        `attributes`: the rows' dicts carry them)"""
        self.path, self.fmt, self.fn, self.flat, self.schema, self.rows, self.literals = str(path), fmt, fn, flat, schema, rows, literals
        self.names = list(names)                                       # every column of the format, in schema order
        self.read = list(flat) + list(beside)                          # what a read without `columns` compares
        self.nullable = {c for c in flat if any(r[c] is None for r in rows)}
        self._rel = None

    def want(self, tree, columns=None):
        cols = self.read if columns is None else columns
        return norm_rows([tuple(r[c] for c in cols) for r in self.rows if fo.keep(tree, r, self.schema)])

    def shard_rows(self, text, columns=None, **kw):
        """kw: passed on to ShardReader (compression, shard_index, shard_count)"""
        from exon_duckdb_amd.reader import ShardReader
        idx = [self.names.index(c) for c in (self.read if columns is None else columns)]
        r = ShardReader(self.path, self.fmt, filters=text, columns=idx, **kw)
        try:
            got = r.rows()
        finally:
            r.close()
        at = [sorted(idx).index(i) for i in idx]                       # rows() yields the projected columns in schema order
        return norm_rows([tuple(row[k] for k in at) for row in got])

    def shard_count(self, text, **kw):
        from exon_duckdb_amd.reader import ShardReader
        r = ShardReader(self.path, self.fmt, filters=text, **kw)
        try:
            return r.count()
        finally:
            r.close()

    def arrow_rows(self, text):
        from exon_duckdb_amd.arrow import new_reader
        tab = new_reader(self.path, self.fmt, filters=text).read_all()
        cols = [tab.column(c).to_pylist() for c in self.read]
        return norm_rows(list(zip(*cols)))

    @property
    def rel(self):
        if self._rel is None:
            from exon_duckdb_amd import table_function
            self._rel = table_function.connect().table_function(self.fn, self.path)
        return self._rel

    def tf_rows(self, filters, columns=None):
        return norm_rows(self.rel.fetchall(columns=self.read if columns is None else columns, filters=filters))


def sql(tree):
    return fo.render_sql(tree, "full").encode("latin-1")


@pytest.fixture(scope="module")
def vcf(gpu, oracle, tmp_path_factory):
    data = vcf_bytes()
    p = tmp_path_factory.mktemp("filters_vcf") / "edge.vcf"
    p.write_bytes(data)
    return Site(p, "vcf", "read_vcf", oracle.VCF_FIELDS, VCF_FLAT, VCF_SCHEMA, vcf_oracle_rows(oracle, data), VCF_LITERALS)


@pytest.fixture(scope="module")
def fastq(gpu, oracle, tmp_path_factory):
    data = fastq_bytes()
    p = tmp_path_factory.mktemp("filters_fastq") / "edge.fastq"
    p.write_bytes(data)
    return Site(p, "fastq", "read_fastq", FQ_FLAT, FQ_FLAT, FQ_SCHEMA, fastq_oracle_rows(oracle, data), FQ_LITERALS)


@pytest.fixture(scope="module")
def bam(gpu, tmp_path_factory):
    raw = bam_raw()
    p = tmp_path_factory.mktemp("filters_bam") / "edge.bam"
    p.write_bytes(B.bgzf(raw, member_bytes=1500))
    parsed = B.parse_decoded(raw)
    assert parsed.error is None and len(parsed.rows) == N_ROWS
    rows = [dict(zip(B.NAMES, r)) for r in parsed.rows]
    return Site(p, "bam", "read_bam_file_records", B.NAMES, BAM_FLAT, BAM_SCHEMA, rows, BAM_LITERALS)


@pytest.fixture(params=["default", "small"])
def batch(request, monkeypatch):
    if request.param == "small":
        monkeypatch.setenv("EXG_DEVICE_BATCH_BYTES", SMALL_BATCH)
    else:
        monkeypatch.delenv("EXG_DEVICE_BATCH_BYTES", raising=False)
    return request.param


# ---- D1: every single leaf ---------------------------------------------------------------------------------------------------
def leaves_of(site, col):
    out = [cmp(col, op, lit) for lit in site.literals.get(col, []) for op in fo.OPS]
    return out + [isnull(col), notnull(col)]


def check_leaves(site, col, read):
    t0, bad = time.time(), []
    trees = leaves_of(site, col)
    for t in trees:
        got, want = read(sql(t)), site.want(t)
        if got != want:
            bad.append((sql(t)[:80], len(got), len(want)))
    print(f"{site.fmt}.{col}: {len(trees)} leaves in {time.time() - t0:.2f} s")
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("col", VCF_FLAT)
def test_vcf_every_leaf(vcf, batch, col):
    check_leaves(vcf, col, vcf.shard_rows)


@pytest.mark.parametrize("col", ["pos", "qual"])
def test_vcf_every_leaf_new_reader(vcf, batch, col):
    check_leaves(vcf, col, vcf.arrow_rows)


@pytest.mark.parametrize("col", FQ_FLAT)
def test_fastq_every_leaf_new_reader(fastq, batch, col):
    check_leaves(fastq, col, fastq.arrow_rows)


@pytest.mark.parametrize("col", BAM_FLAT)
def test_bam_every_leaf(bam, batch, col):
    check_leaves(bam, col, bam.shard_rows)


# ---- D2: random trees --------------------------------------------------------------------------------------------------------
def n_leaves(t):
    return sum(n_leaves(k) for k in t[1]) if t[0] in ("and", "or") else 1


def is_informative(site, t):
    return 0 < sum(fo.keep(t, r, site.schema) for r in site.rows) < len(site.rows)


def trees_for(site, n, seed):
    """depth <= 3, at most 16 leaves (31 ops fit the program).  Tuned with keep() alone: about a third of the plain draws select
    no row or every row (an AND of equalities, an OR of `!=`), so three in four of those are drawn again; the rest stay in."""
    rnd = random.Random(seed)
    out, redrawn = [], 0
    while len(out) < n:
        t = fo.random_tree(rnd, site.literals, site.nullable, 3, p_leaf=0.25)
        if n_leaves(t) > 16:
            continue
        if not is_informative(site, t) and rnd.random() < 0.75:
            redrawn += 1
            continue
        out.append(t)
    print(f"{site.fmt}: {redrawn} uninformative trees drawn again on the way to {n}")
    return out


def informative(site, trees):
    return sum(is_informative(site, t) for t in trees)


def check_trees(site, trees, read, shard=True):
    from exon_duckdb_amd.table_function import F
    t0, fit = time.time(), 0
    share = informative(site, trees) / len(trees)
    for t in trees:
        text, named = sql(t), fo.columns_of(t)
        want = site.want(t)
        assert read(text) == want, text
        proj = [c for c in site.read if c not in named]
        if shard:
            assert site.shard_count(text) == len(want), text
            if proj:
                assert site.shard_rows(text, columns=proj) == site.want(t, proj), text
        d = fo.render_filter_set(t, site.schema, F)
        if d is not None:
            fit += 1
            assert site.tf_rows(d) == want, text
            assert site.rel.count(filters=d) == len(want), text
            if proj:
                assert site.tf_rows(d, columns=proj) == site.want(t, proj), text
    print(f"{site.fmt}: {len(trees)} trees ({fit} fit a TableFilterSet) in {time.time() - t0:.2f} s; "
          f"{share:.0%} select a non-empty proper subset, {len(trees) - round(share * len(trees))} do not")
    assert share >= 0.8, share


def test_vcf_random_trees(vcf, batch):
    check_trees(vcf, trees_for(vcf, N_TREES, 1), vcf.shard_rows)


def test_fastq_random_trees_new_reader(fastq, batch):
    check_trees(fastq, trees_for(fastq, N_TREES, 2), fastq.arrow_rows, shard=False)


def test_bam_random_trees(bam, batch):
    check_trees(bam, trees_for(bam, N_TREES, 3), bam.shard_rows)


# ---- D3: named regressions ------------------------------------------------------------------------------------------------------
def test_or_beside_another_column_keeps_its_tree(bam, batch):
    """TableFilterSet {start: start<5 OR start>=9, flag: flag=99}: rendered without parentheses it read as
    start<5 OR (start>=9 AND flag=99) and returned the rows with start<5 of any flag"""
    from exon_duckdb_amd.table_function import F
    t = and_(or_(cmp("start", "<", "5"), cmp("start", ">=", "9")), cmp("flag", "=", "99"))
    loose = or_(cmp("start", "<", "5"), and_(cmp("start", ">=", "9"), cmp("flag", "=", "99")))
    assert len(bam.want(loose)) > len(bam.want(t)) > 0                 # the file tells the two readings apart
    d = {"start": F.or_(F.cmp("<", 5), F.cmp(">=", 9)), "flag": F.cmp("=", 99)}
    assert bam.tf_rows(d) == bam.want(t)
    assert bam.rel.count(filters=d) == len(bam.want(t))
    assert bam.shard_rows(sql(t)) == bam.want(t)


def test_or_under_and_on_one_column_keeps_its_tree(bam, vcf, batch):
    from exon_duckdb_amd.table_function import F
    t = and_(or_(cmp("start", "<", "5"), cmp("start", ">=", "9")), cmp("start", "!=", "1"))
    assert 0 < len(bam.want(t)) < len(bam.want(t[1][0]))
    assert bam.tf_rows({"start": F.and_(F.or_(F.cmp("<", 5), F.cmp(">=", 9)), F.cmp("!=", 1))}) == bam.want(t)
    v = and_(or_(cmp("chrom", "=", b"1"), cmp("chrom", ">=", b"chr1_random")), cmp("chrom", "!=", b"1"))
    assert 0 < len(vcf.want(v)) < len(vcf.want(v[1][0]))
    assert vcf.tf_rows({"chrom": F.and_(F.or_(F.cmp("=", b"1"), F.cmp(">=", b"chr1_random")), F.cmp("!=", b"1"))}) == vcf.want(v)


@pytest.mark.parametrize("op,lit", [(">", "5"), ("=", "0.1"), ("<=", "0.1"), (">=", "16777217")])
def test_qual_compares_in_float32_with_nan_on_top(vcf, batch, op, lit):
    """qual>5 keeps the NaN rows; qual=0.1 keeps the rows whose QUAL text is 0.1; 16777217 rounds to 16777216"""
    from exon_duckdb_amd.table_function import F
    t = cmp("qual", op, lit)
    want = vcf.want(t)
    nan_rows = sum(1 for r in want if r[3] == ("nan",))
    point1 = sum(1 for r in want if r[3] == norm(fo.f32(0.1)))
    big = sum(1 for r in want if r[3] == norm(16777216.0))
    assert {">": nan_rows, "=": point1, "<=": point1, ">=": big}[op] > 0 and (op != ">=" or nan_rows > 0)
    assert vcf.shard_rows(sql(t)) == want
    assert vcf.arrow_rows(sql(t)) == want
    assert vcf.tf_rows({"qual": F.cmp(op, lit)}) == want
    assert vcf.shard_count(sql(t)) == len(want)


# ---- D4: selection shapes (k_row_map and the gathers) ------------------------------------------------------------------------------
def vcf_row_selector(vcf, k):
    r = vcf.rows[k]
    return and_(cmp("chrom", "=", r["chrom"]), cmp("pos", "=", str(r["pos"])), cmp("ref", "=", r["ref"]))


def batch_starts(vcf):
    """row index of the first row of every device batch, from an unfiltered read"""
    import ctypes as C
    from exon_duckdb_amd.reader import ShardReader
    from exon_duckdb_amd.table_function import Chunk
    r = ShardReader(vcf.path, "vcf", columns=[1])
    starts, n, last = [], 0, None
    try:
        while True:
            ch = Chunk()
            assert r._l.exg_next_chunk(r._r, C.byref(ch)) == 0
            if ch.n_rows == 0:
                return starts
            if ch.batch_no != last:
                starts.append(n)
                last = ch.batch_no
            n += int(ch.n_rows)
            r._l.exg_release_chunk(r._r, C.byref(ch))
    finally:
        r.close()


def test_selection_shapes(vcf, batch):
    starts = batch_starts(vcf)
    if batch == "small":
        assert len(starts) >= 3, starts                                 # the selection crosses several device batches
    shapes = {
        "no row": cmp("pos", "<", "0"),
        "every row": cmp("pos", ">=", "1"),
        "the last row": vcf_row_selector(vcf, N_ROWS - 1),
        "the first row of the last batch": vcf_row_selector(vcf, starts[-1]),
        "the first row": vcf_row_selector(vcf, 0),
        "two rows with 199 and 132 rejected in a run": or_(vcf_row_selector(vcf, 0), vcf_row_selector(vcf, 200)),
        "the first and the last row": or_(vcf_row_selector(vcf, 0), vcf_row_selector(vcf, N_ROWS - 1)),
    }
    sizes = {"no row": 0, "every row": N_ROWS, "the last row": 1, "the first row of the last batch": 1, "the first row": 1,
             "two rows with 199 and 132 rejected in a run": 2, "the first and the last row": 2}
    for name, t in shapes.items():
        want = vcf.want(t)
        assert len(want) == sizes[name], name
        assert vcf.shard_rows(sql(t)) == want, name
        assert vcf.shard_count(sql(t)) == len(want), name
        assert vcf.arrow_rows(sql(t)) == want, name
        assert vcf.shard_rows(sql(t), columns=["qual"]) == vcf.want(t, ["qual"]), name


# ---- D5: refusals that never threw ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", ["pos=1.2.3", "qual='x'"])
def test_refusals(vcf, text):
    from exon_duckdb_amd import ExgError
    from exon_duckdb_amd.arrow import new_reader
    from exon_duckdb_amd.reader import ShardReader
    with pytest.raises(ExgError, match="could not execute sql"):
        ShardReader(vcf.path, "vcf", filters=text)
    with pytest.raises(ExgError, match="could not execute sql"):
        new_reader(vcf.path, "vcf", filters=text)
    assert vcf.shard_count(b"pos>=1") == N_ROWS                          # and the next open is fine
