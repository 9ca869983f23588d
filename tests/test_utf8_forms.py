"""tests/utf8_forms.py on the CPU: the catalogue and two sweeps against the oracle's from_utf8, the formats' UTF-8 rules pinned on the
oracle and on the three Python readers, and the builders' placement."""
import itertools

import pytest

import bed_files as B
import gtf_files as G
import sam_files as S
import utf8_forms as U

SWEEP = bytes.fromhex("00417F808F909FA0BFC0C1C2DFE0E1ECEDEEEFF0F1F3F4F5F7F8FF")
UTF8 = U.E_INVALID_UTF8
SURROGATE, CUT, CHAR4 = b"\xed\xa0\x80", b"\xe2\x82", b"\xf0\x9f\x98\x80"


def test_catalogue_counts_and_the_oracle_agrees_with_the_strict_decoder(oracle):
    cat = U.catalogue()
    forms = [f for f, _ in cat]
    assert len(set(forms)) == len(forms) >= 90 and sum(1 for _, ok in cat if not ok) >= 60
    for f, ok in cat:
        assert oracle.is_valid_utf8(f) == ok == U.strict(f), f.hex()
    for lead in U.LEADS:
        assert any(f[0] == lead and len(f) == U.implied_length(lead) for f in forms), hex(lead)
    for lead, window in U.SECOND.items():
        for c1 in window:
            assert any(f[:2] == bytes([lead, c1]) and len(f) == U.implied_length(lead) for f in forms), (hex(lead), hex(c1))
    for ch in U.CHARS + U.EXTREMES:
        assert (ch, True) in cat and all((ch[:k], False) in cat for k in range(1, len(ch)))
    sub = U.boundary_subset()
    assert set(sub) <= set(cat) and {len(f) for f, _ in sub} == {2, 3, 4} and sum(1 for _, ok in sub if not ok) >= 20
    assert [sf.form for sf in U.SEAM_FORMS if U.strict(sf.form)] == list(U.CHARS) and len(U.SEAM_FORMS) == 8
    assert all(U.placements(sf) == list(range(len(sf.form) + 1)) for sf in U.SEAM_FORMS)


def test_sweep_every_1_and_2_byte_string_and_27_values_of_3_and_4(oracle):
    valid = oracle.lib().orc_is_valid_utf8
    n = bad = 0
    for length, alphabet in ((1, range(256)), (2, range(256)), (3, SWEEP), (4, SWEEP)):
        for t in itertools.product(alphabet, repeat=length):
            s = bytes(t)
            n += 1
            bad += bool(valid(s, length)) != U.strict(s)
    print(f"{n} strings, {bad} disagreements")
    assert len(SWEEP) == 27 and n == 616916 and bad == 0


def one(fmt, text, field=None, broken=False, **kw):
    data, (idx,) = U.build(fmt, [U.Site(text, 0, U.SUPER + 5000, field, broken)], **kw)
    return U.expect(fmt, data), idx


@pytest.mark.parametrize("fmt", U.FORMATS)
def test_every_string_field_is_validated_and_the_record_is_named(oracle, fmt):
    f = U.FMT[fmt]
    assert f.free in f.fields and f.early in f.fields and f.last in f.fields
    for field in f.fields:
        for bad in (SURROGATE + b"xx", b"xx" + CUT):
            v, idx = one(fmt, bad, field)
            assert (v.code, v.record, v.n_rows) == (UTF8, idx, idx), (field, bad, v[:4])
        v, idx = one(fmt, b"xx" + CHAR4, field)
        assert v.code == 0 and v.n_rows > idx, (field, v[:4])
    # the last field of an input that ends without a newline
    v, idx = one(fmt, b"xx" + CUT, f.last, stop=True, final_newline=False)
    assert (v.code, v.record) == (UTF8, idx)


def test_fastq_plus_line_is_not_validated_and_the_space_split_cuts_a_character(oracle):
    v, idx = one("fastq", b"\xff" + CUT, "plus")
    assert v.code == 0 and v.n_rows > idx
    r = oracle.fastq_parse(b"@x\xc3 \xa9\nAC\n+\n!!\n")
    assert (r.error_code, r.n_rows) == (UTF8, 0)
    assert oracle.fastq_parse(b"@x\xc3\xa9 \xc3\xa9\nAC\n+\xff\n!!\n").error_code == 0


def test_fasta_validates_the_joined_sequence_not_its_lines(oracle):
    for eol in (b"\n", b"\r\n"):
        r = oracle.fasta_parse(b">a" + eol + b"A\xc3" + eol + b"\xa9C" + eol)
        assert r.error_code == 0 and r.columns["sequence"].row(0) == b"A\xc3\xa9C", eol
        assert oracle.fasta_parse(b">a" + eol + b"A\xc3" + eol + b"C\xa9" + eol).error_code == UTF8
        v, idx = one("fasta", b"AC\xe2" + eol + b"\x82" + eol + b"\xacGT", "sequence")
        assert v.code == 0
        v, idx = one("fasta", b"AC\xe2" + eol + b"\x82" + eol + b"GT", "sequence")
        assert (v.code, v.record) == (UTF8, idx)


@pytest.mark.parametrize("fmt", U.FORMATS)
def test_a_structural_error_of_the_same_record_wins(oracle, fmt):
    field = "sequence" if fmt == "fasta" else U.FMT[fmt].free
    sound, idx = one(fmt, b"xx", field, broken=True)
    assert sound.code not in (0, UTF8) and sound.record == idx
    v, idx = one(fmt, b"x" + SURROGATE, field, broken=True)
    assert v[:4] == sound[:3] + (idx,)


def test_fasta_definition_line_is_read_into_a_string_before_it_is_parsed(oracle):
    """noodles-fasta reads the definition with read_line into a String and parses it afterwards: on that line UTF-8 comes first"""
    r = oracle.fasta_parse(b"> \xff\nAC\n")
    assert r.error_code == UTF8
    assert oracle.fasta_parse(b"> d\nA\xff\n").error_code == 6


def test_line_readers_put_utf8_behind_the_fields(oracle):
    for mod, bad, code in ((B, b"c\t1\tx\tn\xff", B.E_POSITION), (S, b"q\tx\tchr1\t1\t60\t*\t*\t0\t0\t*\t*\t\xff", S.E_FLAG),
                           (G, b"c\ts\texon\t1\t2\t.\t*\t.\tg \xff", G.E_STRAND)):
        assert mod.read(bad + b"\n")[-1][1] == code
    assert B.read(b"c\t1\t2\tn\xff\n")[-1][1] == S.read(b"q\t0\tchr1\t1\t60\t*\t*\t0\t0\t*\t*\t\xff\n")[-1][1] == UTF8
    assert G.read(b"c\ts\texon\t1\t2\t.\t+\t.\tg \xff\n")[-1][1] == UTF8


def test_vcf_percent_decoding_judges_the_raw_line_first(oracle):
    hdr = b'##fileformat=VCFv4.2\n##INFO=<ID=S,Number=1,Type=String,Description="s">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n'
    line = lambda info: hdr + b"1\t5\t.\tA\tC\t.\t.\t" + info + b"\n"  # noqa: E731
    rows, err = oracle.vcf_typed_rows(line(b"S=%C3%A9"))
    assert err is None and rows[0]["info"]["S"] == "é"
    rows, err = oracle.vcf_typed_rows(line(b"S=%ED%A0%80"))
    assert err == 0 and rows == [] and oracle.vcf_parse(line(b"S=%ED%A0%80")).error_code == 0       # a value error, not a line error
    assert oracle.vcf_parse(line(b"S=\xc3%A9")).error_code == UTF8


@pytest.mark.parametrize("fmt", U.FORMATS)
def test_builders_put_the_byte_where_they_were_asked_to(oracle, fmt):
    f = U.FMT[fmt]
    seams = U.FASTA_SEAMS if fmt == "fasta" else U.FUSED_SEAMS
    for sf in U.SEAM_FORMS:
        for j in U.placements(sf):
            data, idx = U.build(fmt, [U.seam_site(fmt, sf, s, j) for s in seams], size=3 * U.SUPER)
            assert len(data) >= 3 * U.SUPER and idx == sorted(idx) and len(set(idx)) == len(seams)
            for s in seams:
                assert data[s - j:s - j + len(sf.form)] == sf.form, (sf, j, s)
            assert U.is_ascii_but(data, [(s - j, s - j + len(sf.form)) for s in seams])
            v = U.expect(fmt, data)
            assert (v.code, v.record) == ((0, None) if U.strict(sf.form) else (UTF8, idx[0])), (sf, j, v[:4])
    # a record made far: it begins more than the window in front of the half it ends in
    text, k = U.in_field(b"\xff", pre=1500)
    data, (idx,) = U.build(fmt, [U.Site(text, k, U.SUPER + U.HALF + 200)])
    start = data.rfind(U.record(fmt, idx, text)[0])
    assert 0 < start < U.SUPER + U.HALF - U.WINDOW and data[U.SUPER + U.HALF + 200] == 0xFF
