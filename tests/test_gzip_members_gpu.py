"""The device reader against the hand-built gzip / BGZF members of tests/gzip_members.py (proved against zlib in
tests/test_gzip_members.py): every header form RFC 1952 allows, the BC subfield wherever it may stand, empty members, sizes at
BGZF's limits, member boundaries on every byte of a record and across the compressed window, the trailer behind a final block
that ends at every bit phase on all three decoding paths (BGZF window, one wavefront, chunked decoder) — and every way a member
can be wrong: an error, behind the rows in front of it.

Rows and error / no error come from ShardReader(...).rows() and are compared with oracle.compressed_parse; the rows in front
of an error come from new_reader streamed in batches of 64.  Where the catalogue names a rule difference (gzip_members.py's
docstring; oracle/pyoracle.py decode_by_rule states them) the rows in front of the error are the rows of the case's own text."""
import os

import pytest

import gzip_members as gm

pytestmark = pytest.mark.gpu

FQ_NAMES = ("name", "description", "sequence", "quality_scores")


def oracle_rows(table):
    return list(zip(*[table.columns[k].to_list() for k in FQ_NAMES]))


def read_all(path, fmt, **kw):
    """-> (rows, None) or (None, the error)"""
    from exon_duckdb_amd._lib import ExgError
    from exon_duckdb_amd.reader import ShardReader
    r = None
    try:
        r = ShardReader(str(path), fmt, **kw)
        return r.rows(), None
    except ExgError as e:
        return None, e
    finally:
        if r is not None:
            r.close()


def stream_rows(path, fmt, **kw):
    """the Arrow stream in batches of 64 (test_fuzz_gpu._stream_rows): -> (rows handed out as tuples of bytes / None, failed)"""
    import pyarrow as pa
    from exon_duckdb_amd._lib import ExgError
    from exon_duckdb_amd.arrow import new_reader
    rows, failed = [], False
    try:
        for b in new_reader(str(path), fmt, batch_size=64, **kw):
            rows.extend(tuple(None if v is None else v.encode() for v in (d[k] for k in FQ_NAMES)) for d in b.to_pylist())
    except (pa.ArrowException, OSError, ExgError):
        failed = True
    return rows, failed


class Env:
    """a case's environment switches, for the duration of its read"""

    def __init__(self, env):
        self.env, self.old = env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def check_case(oracle, c, path):
    """-> a description of what is wrong with the reader on this case, or None"""
    path.write_bytes(c.data)
    exp = oracle.compressed_parse("fastq", c.data, "gzip")
    with Env(c.env):
        rows, err = read_all(path, "fastq", **c.reader)
        if c.valid:
            if err is not None:
                return "refused: %s" % err
            if exp.error is not None or rows != oracle_rows(exp.table):
                return "rows differ from the oracle's (%d, %d; oracle error %r)" % (len(rows), exp.table.n_rows, exp.error)
            want = oracle_rows(oracle.fastq_parse(c.text, want_string_t=False))
            if rows != want:
                return "rows differ from the plain text's (%d, %d)" % (len(rows), len(want))
            srows, failed = stream_rows(path, "fastq")
            if failed or srows != want:
                return "the Arrow stream differs (%d rows, failed %s)" % (len(srows), failed)
            return None
        if err is None:
            return "read without an error (%d rows)" % len(rows)
        if (exp.error is None) != (c.differs == "bsize_binds"):
            return "the oracle's verdict is not what the catalogue says (%r, differs %r)" % (exp.error, c.differs)
        front = oracle_rows(exp.table) if c.differs is None else oracle_rows(oracle.fastq_parse(c.text, want_string_t=False))
        srows, failed = stream_rows(path, "fastq")
        if not failed:
            return "the Arrow stream ended without an error (%d rows)" % len(srows)
        if srows != front:
            return "rows in front of the error: %d, want %d (%s)" % (len(srows), len(front), err)
    return None


@pytest.mark.parametrize("group", gm.GROUP_NAMES)
def test_catalogue_through_the_reader(gpu, oracle, tmp_path, group):
    cases = gm.groups()[group]
    ran, wrong = 0, []
    for c in cases:
        what = check_case(oracle, c, tmp_path / ("%s.fastq.gz" % c.name))
        ran += 1
        if what:
            wrong.append((c.name, c.clause, what))
    for w in wrong:
        print(w)
    assert not wrong, (len(wrong), "of", len(cases), [w[0] for w in wrong])
    assert ran == len(cases) > 0


def test_the_groups_are_the_whole_catalogue():
    g = gm.groups()
    assert set(g) == set(gm.GROUP_NAMES)
    assert sum(len(g[n]) for n in gm.GROUP_NAMES) == len(gm.valid()) + len(gm.invalid())


# ---- a subset of the valid forms around other formats, in shards, without read-ahead --------------------------------------------
X = (b"XX", b"\1\2\3")


def framings(text):
    """name -> (file bytes, pure BGZF?) of `text` cut into a few members of the forms the catalogue proves on FASTQ"""
    n = len(text)
    a, b, c = text[:n // 3], text[n // 3:2 * n // 3 + 1], text[2 * n // 3 + 1:]
    return {
        "all_optional_fields": (gm.member(a, extra=[X], fname=b"f", fcomment=b"c", fhcrc=True) + gm.member(b + c, fhcrc=True), False),
        "bc_second_then_other": (gm.member(a, extra=[X, gm.BC]) + gm.member(b, extra=[gm.BC, X]) + gm.bgzf_member(c) + gm.EOF_BLOCK, True),
        "bc_beside_fname_and_long_xlen": (gm.member(a, extra=[gm.BC], fname=b"n") + gm.member(b, extra=[gm.BC, (b"PD", b"\0" * 240)]) + gm.bgzf_member(c), False),
        "eof_blocks_everywhere": (gm.EOF_BLOCK + gm.bgzf_member(a) + gm.EOF_BLOCK + gm.EOF_BLOCK + gm.bgzf_member(b + c) + gm.EOF_BLOCK, True),
        "one_byte_members": (b"".join(gm.bgzf_member(text[i:i + 1]) for i in range(n)) + gm.EOF_BLOCK, True),
        "plain_bgzf_plain": (gm.member(a) + gm.bgzf_member(b) + gm.member(b"") + gm.member(c, fname=b""), False),
    }


@pytest.mark.parametrize("fmt", ["vcf", "fasta"])
def test_member_forms_around_vcf_and_fasta(gpu, oracle, tmp_path, fmt):
    text = {"vcf": gm.VCF, "fasta": gm.FA}[fmt]
    plain = tmp_path / ("plain." + fmt)
    plain.write_bytes(text)
    want, err = read_all(plain, fmt)
    assert err is None and len(want) == 2
    for name, (data, _) in framings(text).items():
        exp = oracle.compressed_parse(fmt, data, "gzip")
        assert exp.error is None and exp.table.n_rows == len(want), name
        p = tmp_path / ("%s.%s.gz" % (name, fmt))
        p.write_bytes(data)
        rows, err = read_all(p, fmt)
        assert err is None, (name, str(err))
        assert rows == want, name


@pytest.mark.parametrize("shards", [2, 3])
def test_pure_bgzf_forms_in_shards(gpu, oracle, tmp_path, shards):
    text = gm.FQ + gm.FQ2 + gm.TINY_A + gm.TINY_B + gm.TINY_C
    want = oracle_rows(oracle.fastq_parse(text, want_string_t=False))
    names = [n for n, (_, pure) in framings(text).items() if pure]
    assert len(names) == 3
    for name in names:
        p = tmp_path / (name + ".fastq.gz")
        p.write_bytes(framings(text)[name][0])
        got = []
        for i in range(shards):
            rows, err = read_all(p, "fastq", shard_index=i, shard_count=shards)
            assert err is None, (name, i, str(err))
            got.extend(rows)
        assert got == want, (name, shards)
    for name in ("straddles_256k_window", "cut_at_every_byte_of_a_record"):
        c = gm.valid()[name]
        assert c.pure_bgzf
        p = tmp_path / (name + ".fastq.gz")
        p.write_bytes(c.data)
        got = []
        for i in range(shards):
            rows, err = read_all(p, "fastq", shard_index=i, shard_count=shards)
            assert err is None, (name, i, str(err))
            got.extend(rows)
        assert got == oracle_rows(oracle.fastq_parse(c.text, want_string_t=False)), (name, shards)


def test_without_read_ahead(gpu, oracle, tmp_path, monkeypatch):
    monkeypatch.setenv("EXG_GZ_NO_READAHEAD", "1")
    for name in ("straddles_256k_window", "plain_bgzf_plain", "bc_xlen_241", "eof_middle", "phase_3_bgzf"):
        c = gm.valid()[name]
        assert check_case(oracle, c, tmp_path / (name + ".fastq.gz")) is None, name
    for name in ("crc_byte_2_bgzf", "bsize_takes_in_the_next_member", "tail_zero17_bgzf"):
        c = gm.invalid()[name]
        assert check_case(oracle, c, tmp_path / (name + ".fastq.gz")) is None, name


# ---- BAM: the reader takes BGZF members only -----------------------------------------------------------------------------------------
def test_bam_in_other_member_forms(gpu, tmp_path):
    import bam_files as B
    from exon_duckdb_amd._lib import ExgError
    refs = [(b"ref1", 250_000_000)]
    recs = B.illumina_pairs(3, refs, seed=1)
    raw = B.header(refs) + b"".join(recs)
    canon = tmp_path / "canon.bam"
    canon.write_bytes(B.bgzf(raw))
    want, err = read_all(canon, "bam")
    assert err is None and len(want) == len(recs) == 6
    half = len(raw) // 2
    forms = {
        "eof_in_the_middle": gm.bgzf_member(raw[:half]) + gm.EOF_BLOCK + gm.bgzf_member(raw[half:]) + gm.EOF_BLOCK,
        "eight_byte_members": b"".join(gm.bgzf_member(raw[i:i + 8]) for i in range(0, len(raw), 8)) + gm.EOF_BLOCK,
        "bc_second": gm.member(raw[:half], extra=[X, gm.BC]) + gm.member(raw[half:], extra=[X, gm.BC]) + gm.EOF_BLOCK,
    }
    for name, data in forms.items():
        p = tmp_path / (name + ".bam")
        p.write_bytes(data)
        rows, err = read_all(p, "bam")
        assert err is None, (name, str(err))
        assert rows == want, name
    # a member the BGZF walk refuses (FNAME beside FEXTRA): a valid gzip member, but not BGZF — and BAM is BGZF
    p = tmp_path / "with_fname.bam"
    p.write_bytes(gm.bgzf_member(raw[:half]) + gm.member(raw[half:], extra=[gm.BC], fname=b"x") + gm.EOF_BLOCK)
    rows, err = read_all(p, "bam")
    assert isinstance(err, ExgError) and "not a BGZF member" in str(err), err
