"""UTF-8 validation on the device, through the C-ABI scans of the six text formats and every algorithm selector their own tests
use: every ill-formed form of tests/utf8_forms.py in LDS (short records) and in global memory (far records, the general path),
every validated field and the ones that are not, characters on every seam of the tiling, inputs whose ONLY byte >= 0x80 sits
where just one of the gates (the window, the neighbouring super-tile, the header flag, the redo mark) can see it, and the order of
errors.  The verdict comes from utf8_forms.expect: the formats' references, held against Python's strict decoder.  Then the
readers: files that are mostly 2-, 3- and 4-byte characters through every way of reading them (Arrow re-validates the Utf8 buffers
of the three formats that have an Arrow boundary), an ill-formed form astride a batch cut, VCF's percent-decoded values and BCF.

Inputs are two to three super-tiles; an ill-formed input costs one launch.  Every launch of a (format, selector) case compares all
rows in front of the error, except on the seams, where one placement per form does (the lean selector's unmarked neighbours
deliver their rows unchanged: that is this comparison under EXG_ALGO_FUSED)."""
import numpy as np
import pytest

import test_bed_gpu as TB
import test_fasta_gpu as TA
import test_fastq_gpu as TQ
import test_gtf_gpu as TG
import test_sam_gpu as TS
import test_vcf_gpu as TV
import test_vcf_nested_gpu as TN
import utf8_forms as U
from exon_duckdb_amd import abi

pytestmark = pytest.mark.gpu

UTF8 = abi.EXG_PE_INVALID_UTF8
HALF, SUPER = U.HALF, U.SUPER
LINE_ALGOS = [abi.EXG_ALGO_AUTO, abi.EXG_ALGO_FUSED, abi.EXG_ALGO_MULTIPASS, abi.EXG_ALGO_FUSED_FULL]
ALGOS = {"fastq": TQ.ALGOS, "fasta": TA.ALGOS, "vcf": TV.ALGOS, "bed": LINE_ALGOS, "sam": LINE_ALGOS, "gtf": LINE_ALGOS}
CASES = [pytest.param(fmt, algo, id=f"{fmt}-algo{algo}") for fmt in U.FORMATS for algo in ALGOS[fmt]]
LINE_LAUNCH = {"bed": TB.launch, "sam": TS.launch, "gtf": TG.launch}
SURROGATE, CUT, CHAR4 = b"\xed\xa0\x80", b"\xe2\x82", b"\xf0\x9f\x98\x80"
BAD_FLAGS = abi.EXG_RF_FALLBACK | abi.EXG_RF_CAPACITY | abi.EXG_RF_HEAD_UNRESOLVED | abi.EXG_RF_INDEX_OVERFLOW


def vcf_launch(data, algo):
    """data lines alone (what the reader hands the kernel behind the header it strips): every offset of the tiling is reachable"""
    from exon_duckdb_amd import device
    d_in = device.upload(data)
    scan = device.VcfScan(len(data))
    scan.launch(d_in, lead=0, payload_base=U.VCF_BASE, algo=algo)
    res = scan.fetch()
    return res, scan.host(int(res.n_records))


def run(fmt, data, algo, v=None, full=True):
    """one launch against the verdict: the error triple, n_records and the flags; full: every row in front as well"""
    v = v or U.expect(fmt, data)
    n = v.n_rows
    if fmt == "fastq":
        res, cols, words = TQ.run_gpu(data, algo)
    elif fmt == "fasta":
        res, cols, words, payload = TA.run_gpu(data, algo=algo)
    elif fmt == "vcf":
        res, got = vcf_launch(data, algo)
    else:
        scan, res = LINE_LAUNCH[fmt](data, algo)
    what = (fmt, algo, res.error_code, res.error_record, res.error_offset, res.n_records, v[:4])
    assert not res.flags & BAD_FLAGS, what
    assert res.error_code == v.code and res.n_records == n, what
    if v.code:
        assert (res.error_record, res.error_offset) == (v.record, v.offset), what
    else:
        assert res.consumed_bytes == len(data), what
        assert bool(res.flags & abi.EXG_RF_NON_ASCII) == (max(data) >= 0x80), what
    if not full:
        return res
    if fmt == "fastq":
        for k, name in enumerate(TQ.NAMES):
            want, want_words = v.ref.string_t[name]
            assert np.array_equal(cols[k], want), (what, name)
        valid = np.unpackbits(words.view(np.uint8), bitorder="little")[:n]
        assert np.array_equal(valid, v.ref.columns["description"].valid), what
    elif fmt == "fasta":
        valid = np.unpackbits(words.view(np.uint8), bitorder="little")[:n]
        assert np.array_equal(valid, v.ref.columns["description"].valid), what
        pl = payload.tobytes()
        for k, name in enumerate(["id", "description", "sequence"]):
            col = v.ref.columns[name]
            for i in range(n):
                want = col.row(i)
                assert (not cols[k][i].any()) if want is None else TA.resolve(cols[k][i], data, pl) == want, (what, name, i)
        if not v.code:
            assert pl == v.ref.columns["sequence"].values.tobytes(), what
    elif fmt == "vcf":
        from oracle import pyoracle
        for k, name in enumerate(pyoracle.VCF_FIELDS):
            assert np.array_equal(got["cols"][k], v.ref.string_t[name][0]), (what, name)
        assert np.array_equal(got["pos"], v.ref.extra["pos"]), what
        assert np.array_equal(TV.bits(got["qual_valid"], n), v.ref.extra["qual_valid"]), what
        assert np.array_equal(TV.bits(got["formats_valid"], n), v.ref.columns["formats"].valid), what
    else:
        if fmt == "gtf":
            assert scan.kept(n).tolist() == v.ref[1], what
        rows = scan.rows(n, data)
        if rows != v.ref[0]:
            k = next((i for i, (g, w) in enumerate(zip(rows, v.ref[0])) if g != w), min(len(rows), len(v.ref[0])))
            raise AssertionError((what, k, rows[k:k + 1], v.ref[0][k:k + 1]))
    return res


def expect_utf8_at(fmt, data, idx):
    v = U.expect(fmt, data)
    assert (v.code, v.record, v.n_rows) == (UTF8, idx, idx), (fmt, v[:4], idx)
    return v


def expect_clean(fmt, data):
    v = U.expect(fmt, data)
    assert v.code == 0, (fmt, v[:4])
    return v


# ---------------------------------------------------------------- a. every form, from LDS and from global memory
SHAPES = {"short": (SUPER + 5000, 20), "far": (SUPER + HALF + 200, 1500)}      # (the form's offset, ASCII in front of it in its field)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("fmt,algo", CASES)
def test_every_form_in_the_second_super_tile(gpu, fmt, algo, shape):
    """short: the record lies in one half (validated out of LDS); far: it begins more than the window in front of the half it
    ends in (validated from global memory behind the scan); the multipass selector validates from global memory in both"""
    at, pre = SHAPES[shape]
    forms = U.catalogue() if fmt in ("fastq", "bed") else U.boundary_subset()
    good = [f for f, ok in forms if ok]
    bad = [f for f, ok in forms if not ok]
    assert len(good) + len(bad) == len(forms) and len(bad) >= (60 if fmt in ("fastq", "bed") else 20)
    data, _ = U.build(fmt, [U.Site(b"x" * pre + b"a".join(good) + b"y" * 8, pre, at)])
    run(fmt, data, algo, expect_clean(fmt, data))
    for form in bad:
        text, k = U.in_field(form, pre=pre)
        data, (idx,) = U.build(fmt, [U.Site(text, k, at)])
        assert data[at:at + len(form)] == form and U.is_ascii_but(data, [(at, at + len(form))])
        run(fmt, data, algo, expect_utf8_at(fmt, data, idx))


# ---------------------------------------------------------------- b. every validated field, and the ones that are not
@pytest.mark.parametrize("fmt,algo", CASES)
def test_every_field_first_and_last_bytes(gpu, fmt, algo):
    f = U.FMT[fmt]
    for field in f.fields + f.unvalidated:
        for form in (CUT, SURROGATE, CHAR4):
            for text in (form + b"xxxx", b"xxxx" + form):
                data, (idx,) = U.build(fmt, [U.Site(text, 0, SUPER + 3000, field)])
                ok = U.strict(form) or field in f.unvalidated
                run(fmt, data, algo, expect_clean(fmt, data) if ok else expect_utf8_at(fmt, data, idx))
    for form in (CUT, SURROGATE, CHAR4):            # the input's last field, no newline behind it
        data, (idx,) = U.build(fmt, [U.Site(b"xxxx" + form, 0, SUPER + 3000, f.last)], stop=True, final_newline=False)
        assert data.endswith(form)
        run(fmt, data, algo, expect_clean(fmt, data) if U.strict(form) else expect_utf8_at(fmt, data, idx))
    data, (idx,) = U.build(fmt, [U.Site(b"xxxx" + CUT + b"\r", 0, SUPER + 3000, f.free)])      # ... and directly in front of a CR LF
    run(fmt, data, algo, expect_utf8_at(fmt, data, idx))


# ---------------------------------------------------------------- c. seams
def seams_of(fmt):
    return U.FASTA_SEAMS if fmt == "fasta" else U.FUSED_SEAMS


def split_sequence_site(sf, seam, m, shift):
    """FASTA: the form's first m bytes, a line break on seam - shift, the rest: the joined sequence holds the form whole"""
    text = b"ACGT" * 5 + sf.form[:m] + b"\n" + sf.form[m:] + (b"" if sf.ends_field else b"ACGT")
    return U.Site(text, 20 + m, seam - shift, "sequence")


@pytest.mark.parametrize("fmt,algo", CASES)
def test_well_formed_characters_on_every_seam(gpu, fmt, algo):
    """each placement of each well-formed seam form, on all seams of one input"""
    seams = seams_of(fmt)
    n = 0
    for sf in U.SEAM_FORMS:
        if not U.strict(sf.form):
            continue
        for j in U.placements(sf):
            data, idx = U.build(fmt, [U.seam_site(fmt, sf, s, j) for s in seams], size=max(seams) + 4096)
            assert all(data[s - j:s - j + len(sf.form)] == sf.form for s in seams)
            run(fmt, data, algo, expect_clean(fmt, data))
            n += 1
        if fmt == "fasta":
            for m in range(1, len(sf.form)):
                for shift in (0, 1):
                    data, idx = U.build(fmt, [split_sequence_site(sf, s, m, shift) for s in seams if s > 64], size=max(seams) + 4096)
                    run(fmt, data, algo, expect_clean(fmt, data))
    assert n == 3 + 4 + 5


SEAM_CASES = [pytest.param(fmt, algo, s, id=f"{fmt}-algo{algo}-{s}") for fmt in U.FORMATS for algo in ALGOS[fmt] for s in seams_of(fmt)]


@pytest.mark.parametrize("fmt,algo,seam", SEAM_CASES)
def test_ill_formed_forms_on_a_seam(gpu, fmt, algo, seam):
    """first byte on seam - j, j = 0..L: wholly behind the seam, every split, wholly in front.  One launch each; the rows in front
    are compared in full for the first placement of each form"""
    n = 0
    for sf in U.SEAM_FORMS:
        if U.strict(sf.form):
            continue
        for j in U.placements(sf):
            data, (idx,) = U.build(fmt, [U.seam_site(fmt, sf, seam, j)], size=max(2 * SUPER, seam) + 4096)
            assert data[seam - j:seam - j + len(sf.form)] == sf.form
            run(fmt, data, algo, expect_utf8_at(fmt, data, idx), full=j == 0)
            n += 1
        if fmt == "fasta" and seam > 64:
            for m in range(1, len(sf.form)):
                data, (idx,) = U.build(fmt, [split_sequence_site(sf, seam, m, 0)], size=max(2 * SUPER, seam) + 4096)
                assert data[seam] == 10
                run(fmt, data, algo, expect_utf8_at(fmt, data, idx), full=False)
    assert n == 3 + 4 + 5 + 4 + 3


# ---------------------------------------------------------------- d. the gates: ONE byte >= 0x80 (or one character) in the input
def gate_in_front(fmt, boundary, d, payload):
    """a record that begins d bytes in front of `boundary` and ends behind it, the payload's last byte on boundary - 1 (a record
    whose first bytes are fixed begins as little earlier as the payload needs)"""
    field = U.FMT[fmt].early
    toff = U.record(fmt, 0, b"x", field)[1]
    d = max(d, toff + len(payload))
    k = d - toff - len(payload)
    return U.Site(b"x" * k + payload + b"y" * 80, k + len(payload) - 1, boundary - 1, field), boundary - d


def gate_behind(fmt, boundary, payload):
    """a record that begins 100 bytes in front of `boundary`, the payload 10 bytes behind it"""
    field = U.FMT[fmt].early
    k = 110 - U.record(fmt, 0, b"x", field)[1]
    return U.Site(b"x" * k + payload + b"y" * 20, k, boundary + 10, field), boundary - 100


@pytest.mark.parametrize("payload", [b"\xff", b"\xc3\xa9"], ids=["ff", "c3a9"])
@pytest.mark.parametrize("fmt,algo", CASES)
def test_the_only_non_ascii_byte_is_seen_by_every_gate(gpu, fmt, algo, payload):
    ok = U.strict(payload)

    def go(site, start=None, **kw):
        data, (idx,) = U.build(fmt, [site], **kw)
        at = data.index(payload)
        assert U.is_ascii_but(data, [(at, at + len(payload))])
        if start is not None:
            assert data[start:].startswith(U.record(fmt, idx, site.text, site.field)[0][:-1]), (fmt, start)
        run(fmt, data, algo, expect_clean(fmt, data) if ok else expect_utf8_at(fmt, data, idx))
        return data, at

    for boundary in (SUPER, 2 * SUPER, HALF, SUPER + HALF):
        for d in (1, 2, 512, 1023, 1024, 1025, 1040, 5000):       # within the window; a far record
            site, start = gate_in_front(fmt, boundary, d, payload)
            data, at = go(site, start, size=3 * SUPER)
            assert start <= at < boundary and at + len(payload) == boundary
        site, start = gate_behind(fmt, boundary, payload)
        data, at = go(site, start, size=3 * SUPER)
        assert at == boundary + 10
    for pos in (100, 35000, 69900):                               # a 70 KB field over three super-tiles
        text = b"x" * pos + payload + b"y" * (70000 - pos)
        data, at = go(U.Site(text, pos, SUPER - 5000 + pos), size=4 * SUPER)
        assert at // SUPER == (0, 1, 2)[(100, 35000, 69900).index(pos)]
    for tail in (b"", b"y" * 7):                                  # the input's last byte; its last 16-byte chunk
        data, at = go(U.Site(b"x" * 40 + payload + tail, 40, 2 * SUPER + 3000, U.FMT[fmt].last), stop=True, final_newline=False)
        assert at + len(payload) + len(tail) == len(data)


# ---------------------------------------------------------------- e. order
@pytest.mark.parametrize("fmt,algo", CASES)
def test_the_earlier_of_two_bad_records_wins_whichever_kind(gpu, fmt, algo):
    field = "sequence" if fmt == "fasta" else None
    kinds = {"utf8": (b"xx" + SURROGATE, False), "struct": (b"xxxx", True)}
    for first in kinds:
        for second in kinds:
            sites = [U.Site(kinds[first][0], 0, HALF + 3000, field, kinds[first][1]),
                     U.Site(kinds[second][0], 0, 2 * SUPER + 9000, field, kinds[second][1])]
            data, idx = U.build(fmt, sites, size=3 * SUPER)
            v = U.expect(fmt, data)
            assert v.record == idx[0] and (v.code == UTF8) == (first == "utf8") and v.code != 0, (fmt, first, second, v[:4])
            run(fmt, data, algo, v)


@pytest.mark.parametrize("fmt,algo", CASES)
def test_a_structural_error_of_the_same_record_wins(gpu, fmt, algo):
    field = "sequence" if fmt == "fasta" else None
    for at, pre in SHAPES.values():
        if fmt == "fasta":
            pre = 20                                    # (the sequence lines of a record are short)
        data, (idx,) = U.build(fmt, [U.Site(b"x" * pre + SURROGATE + b"y" * 8, pre, at, field, True)])
        v = U.expect(fmt, data)
        assert v.code not in (0, UTF8) and v.record == idx, (fmt, v[:4])
        run(fmt, data, algo, v)
    if fmt == "fasta":                                  # the definition line is a String before it is parsed: there UTF-8 comes first
        data, (idx,) = U.build(fmt, [U.Site(b"xx" + SURROGATE, 0, SUPER + 5000, "description", True)])
        run(fmt, data, algo, expect_utf8_at(fmt, data, idx))


# ---------------------------------------------------------------- f. dense, well-formed files through the readers
def want_rows(fmt, data):
    from oracle import pyoracle
    if fmt in ("fastq", "fasta"):
        ref = pyoracle.fastq_parse(data, want_string_t=False) if fmt == "fastq" else pyoracle.fasta_parse(data)
        assert ref.error_code == 0
        names = TQ.NAMES if fmt == "fastq" else ["id", "description", "sequence"]
        return list(zip(*(ref.columns[k].to_list() for k in names)))
    if fmt == "vcf":
        rows, err = pyoracle.vcf_typed_rows(data)
        assert err is None
        return rows
    if fmt == "gtf":
        return TG.user_rows(data)
    rows, err = U.B.read(data) if fmt == "bed" else U.S.read_file(data)
    assert err is None
    return rows


def read_rows(fmt, path, **kw):
    if fmt == "vcf":
        return TN.reader_rows(str(path), **kw)
    from exon_duckdb_amd.reader import ShardReader
    r = ShardReader(str(path), fmt, **kw)
    try:
        return r.rows()
    finally:
        r.close()


def same_rows(fmt, got, want, how):
    assert len(got) == len(want), (fmt, how, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert TN.same(g, w) if fmt == "vcf" else g == w, (fmt, how, i, g, w)


@pytest.mark.parametrize("fmt", U.FORMATS)
def test_dense_well_formed_files_through_every_reading(gpu, fmt, tmp_path, monkeypatch):
    import bz2
    import random

    import gzip_members
    import zstd_util
    data = U.dense(fmt)
    want = want_rows(fmt, data)
    assert len(want) > 300
    p = tmp_path / ("dense." + fmt)
    p.write_bytes(data)
    same_rows(fmt, read_rows(fmt, p), want, "whole")
    for batch in (4096, 65536):
        same_rows(fmt, read_rows(fmt, p, device_batch_bytes=batch), want, batch)
    same_rows(fmt, sum((read_rows(fmt, p, shard_index=i, shard_count=7) for i in range(7)), []), want, "7 shards")
    monkeypatch.setenv("EXON_GPU_SHARDS", "5")
    monkeypatch.setenv("EXG_FANOUT_WORKERS", "3")
    same_rows(fmt, read_rows(fmt, p, shard_count=0), want, "5 stripes")
    gz = tmp_path / f"dense.bgz.{fmt}.gz"
    gz.write_bytes(gzip_members.bgzf(data, 300))
    same_rows(fmt, read_rows(fmt, gz), want, "BGZF, 300-byte members")
    rng = random.Random(7)
    cuts = [0] + sorted(rng.sample(range(1, len(data)), 12)) + [len(data)]
    zst = tmp_path / f"dense.{fmt}.zst"
    zst.write_bytes(b"".join(zstd_util.compress(data[a:b]) for a, b in zip(cuts, cuts[1:])))
    assert any(not U.strict(data[a:b]) for a, b in zip(cuts, cuts[1:])), "no frame ends inside a character"
    same_rows(fmt, read_rows(fmt, zst), want, "zstd frames")
    bz = tmp_path / f"dense.{fmt}.bz2"
    bz.write_bytes(bz2.compress(data))
    same_rows(fmt, read_rows(fmt, bz, compression="bzip2"), want, "bzip2")
    if fmt in ("fastq", "fasta", "vcf"):                 # the Arrow boundary is built for these: Arrow re-validates every Utf8 buffer
        from exon_duckdb_amd.arrow import new_reader
        table = new_reader(str(p), fmt).read_all()
        table.validate(full=True)
        assert table.num_rows == len(want)
        if fmt != "vcf":
            cols = [table.column(k).to_pylist() for k in range(table.num_columns)]
            assert list(zip(*cols)) == [tuple(None if v is None else v.decode() for v in r) for r in want]
    else:                                                # the chunk boundary hands out bytes: every one of them decodes
        def decodes(v):
            return all(decodes(x) for x in v) if isinstance(v, (list, tuple)) else not isinstance(v, bytes) or U.strict(v)
        assert all(decodes(r) for r in read_rows(fmt, p))


def rows_until_error(fmt, path, **kw):
    """the rows a reader hands out before it fails -> (rows, the error's text or None)"""
    from exon_duckdb_amd import ExgError
    from exon_duckdb_amd.reader import ShardReader
    from exon_duckdb_amd.table_function import Chunk, decode_vector
    import ctypes as C
    r = ShardReader(str(path), fmt, **kw)
    out = []
    try:
        while True:
            ch = Chunk()
            rc = r._l.exg_next_chunk(r._r, C.byref(ch))
            if rc != 0:
                try:
                    r._fail(rc)
                except ExgError as e:
                    return out, str(e)
            if int(ch.n_rows) == 0:
                return out, None
            out.extend(zip(*(decode_vector(ch.vectors[k].contents, r.trees[k]) for k in range(len(r.names)))))
            r._l.exg_release_chunk(r._r, C.byref(ch))
    finally:
        r.close()


@pytest.mark.parametrize("fmt", U.FORMATS)
def test_reader_names_utf8_and_the_record_across_a_batch_cut(gpu, fmt, tmp_path):
    """an ill-formed form astride byte 4096 of the file, read in 4096-byte batches: the rows in front arrive, the error says UTF-8
    and where the record begins"""
    head = U.file_head(fmt)
    form = b"\xe2\x82\x41"
    text, k = U.in_field(form)
    body, (idx,) = U.build(fmt, [U.Site(text, k, 4095 - len(head))], size=SUPER)
    data = head + body
    assert data[4095:4098] == form
    v = U.expect(fmt, body)
    assert (v.code, v.record) == (UTF8, idx)
    sound, _ = U.build(fmt, [U.Site(b"x" * len(text), k, 4095 - len(head))], size=SUPER)
    want = want_rows(fmt, head + sound)[:idx]
    p = tmp_path / ("bad." + fmt)
    p.write_bytes(data)
    for kw in ({"device_batch_bytes": 4096}, {}):
        rows, msg = rows_until_error(fmt, p, **kw)
        assert msg is not None and f"invalid utf-8 at byte {v.offset + len(head)} of" in msg, (fmt, kw, msg)
        got = [dict(zip(["chrom", "pos", "id", "ref", "alt", "qual", "filter", "info", "formats"], map(TN.norm, t))) for t in rows] if fmt == "vcf" else rows
        same_rows(fmt, got, want, kw)


# ---------------------------------------------------------------- g. VCF's percent-decoded values, and BCF
def test_vcf_percent_decoded_values_at_both_boundaries(gpu, tmp_path):
    from exon_duckdb_amd.arrow import new_reader
    line = lambda i, info: b"1\t%d\t.\tA\tC\t.\t.\t" % i + info + b"\n"  # noqa: E731
    cases = {"value": (b"S=%C3%A9", None), "value_error": (b"S=%ED%A0%80", "invalid info field value"), "line_error": (b"S=\xc3%A9", "invalid utf-8")}
    for name, (info, error) in cases.items():
        p = tmp_path / (name + ".vcf")
        p.write_bytes(U.VCF_INFO_HDR + line(5, b"S=a") + line(6, info) + line(7, b"S=b"))
        if error is None:
            rows = TN.reader_rows(str(p))
            assert [r["info"]["S"] for r in rows] == ["a", "é", "b"]
            table = new_reader(str(p), "vcf").read_all()
            table.validate(full=True)
            assert [r["info"]["S"] for r in table.to_pylist()] == ["a", "é", "b"]
            continue
        rows, msg = rows_until_error("vcf", p)
        assert msg is not None and error in msg and ("invalid utf-8" in msg) == (error == "invalid utf-8"), (name, msg)
        assert len(rows) <= 1 and all(TN.norm(r[7])["S"] == "a" for r in rows), name
        with pytest.raises(Exception):
            new_reader(str(p), "vcf").read_all()


def test_bcf_strings_that_are_not_utf8_read_as_their_vcf_text_does(gpu, tmp_path):
    """a BCF record whose ID and INFO string hold ED A0 80: read_bcf_file_records gives what read_vcf gives on the text the
    renderer of bcf_files writes for the same records"""
    import bcf_files as BCF
    import test_bcf_gpu as TBC
    text = TBC.header()
    key = TBC.K(text, "STR")
    good = lambda pos, s: BCF.record(chrom=0, pos=pos, id_=b"id" + s, alleles=(b"A", b"C"), info=[(key, BCF.chars(b"v" + s))])  # noqa: E731
    for name, records in (("sound", [good(1, b"\xc3\xa9"), good(2, b"\xf0\x9f\x98\x80")]),
                          ("id_and_value", [good(1, b"a"), good(2, SURROGATE), good(3, b"b")])):
        strings, contigs, n_samples = BCF.dictionaries(text)
        rendered = BCF.Rendered(b"".join(records), strings, contigs, n_samples)
        assert rendered.error is None and len(rendered.lines) == len(records)
        bcf, vcf = tmp_path / (name + ".bcf"), tmp_path / (name + ".vcf")
        bcf.write_bytes(BCF.bgzf_file(text, records))
        vcf.write_bytes(text + rendered.text)
        rows_v, msg_v = rows_until_error("vcf", vcf)
        rows_b, msg_b = rows_until_error("bcf", bcf)
        assert (msg_v is None) == (msg_b is None) == (name == "sound"), (name, msg_v, msg_b)
        if name == "sound":
            assert len(rows_v) == 2
            TBC.same_rows(rows_b, rows_v)
        else:
            assert "invalid utf-8" in msg_v and "invalid utf-8" in msg_b, (msg_v, msg_b)
            TBC.same_rows(rows_b[:1], rows_v[:1])
