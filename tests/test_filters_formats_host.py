"""What keeps tests/test_filters_formats_gpu.py from passing vacuously, checked without a device: the edge files of
tests/filter_format_sites.py parse, with the independent readers, to the 333 rows the tests expect; the GTF file's comment lines
fall where the keep words are to be mixed, empty and full; the NULLs are where the design puts them; the random trees of every
seed select, four in five, a non-empty proper subset; every column has a leaf that tells rows apart; and the GTF scores tell
the orderings of -0, the negative denormal, -FLT_MAX and -inf apart.  Only keep() of tests/filter_oracle.py decides here."""
import pytest

import bcf_files as BCF
import filter_format_sites as S
import filter_oracle as fo
import gtf_files as G
import test_filters_gpu as TF
from filter_oracle import cmp, isnull, notnull

N_ROWS = S.N_ROWS


@pytest.fixture(scope="module")
def sites(oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("filter_sites")
    gtf, keep = S.gtf_site(d / "edge.gtf")
    gtf.keep = keep
    fq = TF.fastq_bytes()
    fastq = TF.Site(d / "edge.fastq", "fastq", "read_fastq", TF.FQ_FLAT, TF.FQ_FLAT, TF.FQ_SCHEMA, TF.fastq_oracle_rows(oracle, fq), TF.FQ_LITERALS)
    return {"gtf": gtf, "fasta": S.fasta_site(oracle, d / "edge.fasta"), "bcf": S.bcf_site(oracle, d / "edge.bcf"), "fastq": fastq}


def selected(site, tree):
    return frozenset(k for k, r in enumerate(site.rows) if fo.keep(tree, r, site.schema))


def test_every_file_parses_to_333_rows(oracle, sites):
    rows, keep, err = G.read(S.gtf_bytes())
    assert err is None and len(rows) == N_ROWS == keep.count(True)
    assert all(2 <= len(r[8]) <= 6 for r in rows)                                            # two to six attributes a line
    quoted = [r for r in rows if any(b";" in v and b" " in v for _, v in r[8])]
    assert 5 <= len(quoted) <= 9                                                             # one line in about fifty
    res = oracle.fasta_parse(S.fasta_bytes())
    assert res.error_code == 0 and res.n_rows == N_ROWS
    vcf, err = S.bcf_as_vcf(S.bcf_records())
    assert err is None
    res = oracle.vcf_parse(vcf, want_string_t=False)
    assert res.error_code == 0 and res.n_rows == N_ROWS
    assert all(len(s.rows) == N_ROWS for s in sites.values())


def test_gtf_comment_lines_mix_empty_and_fill_the_keep_words(sites):
    data, keep = S.gtf_bytes(), sites["gtf"].keep
    assert keep[62] and keep[63:66] == [False] * 3 and keep[66]
    words = [keep[k:k + 64] for k in range(0, len(keep), 64)]
    assert any(len(w) == 64 and not any(w) for w in words) and any(all(w) for w in words) and any(any(w) and not all(w) for w in words)
    assert not any(keep[k] for k in S.GTF_RUN70) and keep[S.GTF_RUN70[0] - 1] and keep[S.GTF_RUN70[-1] + 1]
    assert keep[-1] is False and data.endswith(b"#the last line\n")
    lines = G.lines_of(data)
    run = lines[S.GTF_LONG_RUN[0]][0], lines[S.GTF_LONG_RUN[-1] + 1][0]
    assert run[1] - run[0] >= 3 * 4096 and not any(keep[k] for k in S.GTF_LONG_RUN)          # whole batches of 4 096 bytes without a row
    assert all(k != sum(keep[:k]) for k in range(len(keep)) if keep[k])                      # no row's index among lines is its index among rows
    raw = data.split(b"\n")[:-1]
    assert all((ln[-1:] == b"\r") == (k % 7 == 6) for k, ln in enumerate(raw))               # CRLF on every seventh line


def test_fasta_sequences_are_wrapped_and_joined_as_designed(sites):
    seqs = S.FA_SEQS
    assert [len(s) for s in seqs] == [1, 4, 12, 13, 13, 300, 300, 120, 180]
    assert seqs[3][:12] == seqs[4][:12] and seqs[3] != seqs[4]
    assert [k for k in range(300) if seqs[5][k] != seqs[6][k]] == [240]                      # the first byte of the last line of five
    assert seqs[8][:120] == seqs[7]                                                          # a proper prefix that ends at a line join
    data = S.fasta_bytes()
    assert b"\r\n" in data and max(len(ln) for ln in data.split(b"\n") if ln[:1] != b">") <= 61
    got = {r["sequence"] for r in sites["fasta"].rows}
    assert got == set(seqs)
    assert {len(r["description"]) for r in sites["fasta"].rows if r["description"] is not None} >= {1, 12, 13, 300}


def test_bcf_quals_left_out_are_the_ones_the_format_refuses(oracle):
    """every FLOAT_EDGES value of tests/test_bcf_gpu.py is in the file or is a parse error of the VCF line it renders to"""
    import test_bcf_gpu as TB
    assert sorted(S.BCF_QUAL_BITS + S.BCF_QUAL_REFUSED) == sorted(TB.FLOAT_EDGES)
    for bits in S.BCF_QUAL_REFUSED:
        vcf, err = S.bcf_as_vcf([BCF.record(chrom=0, pos=5, alleles=(b"A", b"C"), qual=("bits", bits))])
        res = oracle.vcf_parse(vcf, want_string_t=False)
        assert err is None and res.error_code != 0 and res.n_rows == 0 and "quality" in res.error_message, hex(bits)
    raw = BCF.file_header(S.bcf_header()) + b"".join(S.bcf_records())
    assert len(raw) > 10 * 1500                                                              # many BGZF members of 1 500 bytes


def test_nullable_columns(sites):
    assert sites["gtf"].nullable == {"score", "strand", "frame"}
    assert sites["fasta"].nullable == {"description"}
    assert sites["bcf"].nullable == {"qual"}


SEEDS = {"gtf": ["gtf", "gtf zst", "gtf gz", "gtf shards"], "fasta": ["fasta", "fasta new_reader", "fasta gz", "fasta bz2", "fasta shards"], "bcf": ["bcf"],
         "fastq": ["fastq shard"]}


@pytest.mark.parametrize("key", sorted(S.TREES))
def test_four_trees_in_five_select_a_proper_subset(sites, key):
    site = sites[next(name for name, keys in SEEDS.items() if key in keys)]
    n, seed = S.TREES[key]
    trees = TF.trees_for(site, n, seed)
    assert len(trees) == n and TF.informative(site, trees) / len(trees) >= 0.8


def test_every_column_has_a_leaf_that_tells_rows_apart(sites):
    for name in ("gtf", "fasta", "bcf"):
        site = sites[name]
        assert set(site.literals) == set(site.flat), name
        for col in site.flat:
            assert any(TF.is_informative(site, t) for t in TF.leaves_of(site, col)), (name, col)
        for col in site.nullable:
            assert TF.is_informative(site, isnull(col)) and TF.is_informative(site, notnull(col)), (name, col)


def test_gtf_scores_tell_the_negative_orderings_apart(sites):
    gtf = sites["gtf"]
    leaf = lambda op, lit: selected(gtf, cmp("score", op, lit))
    named = [leaf("<", "0"), leaf("<=", "-0"), leaf(">", "-1e-45"), leaf(">=", "-3.4028235e38")]
    assert len(set(named)) == 4 and all(0 < len(s) < N_ROWS for s in named)
    bits = lambda rows: {TF.norm(gtf.rows[k]["score"]) for k in rows}
    f = lambda x: TF.norm(fo.f32(x))
    assert bits(leaf("<=", "-0") - leaf("<", "0")) == {f(0.0), f(-0.0)}                      # -0 = +0: neither is below zero
    assert bits(leaf(">=", "-1e-45") - leaf(">", "-1e-45")) == {f(-1e-45)}                   # the negative denormal is not flushed to zero
    assert bits(leaf("<", "0") - leaf("<", "-1e-45")) == {f(-1e-45)}
    assert bits(leaf(">=", "-3.4028235e38") - leaf(">", "-3.4028235e38")) == {f(-3.4028235e38)}
    assert bits(selected(gtf, notnull("score")) - leaf(">=", "-3.4028235e38")) == {f(float("-inf"))}      # -inf below -FLT_MAX
    assert ("nan",) in bits(leaf(">", "3.4028235e38")) and f(float("inf")) in bits(leaf(">", "3.4028235e38"))   # NaN above +inf
