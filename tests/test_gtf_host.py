"""read_gtf without a GPU: the Python GTF reader that is the oracle of the GTF tests (tests/gtf_files.py) against what the
reference pins (test_gtf_scan.test: one row and the count 77), one named test per rule of INTEGRATION.md (GTF), and the
library's surface that needs no device: the ctypes mirrors, the catalog, the replacement scan, the error strings, the
workspace size and the refusal at the Arrow boundary."""
import ctypes as C
import json
import os
import subprocess

import pytest

import gtf_files as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "exon_gpu.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gtf")
EXPECTED = json.load(open(os.path.join(GOLDEN, "expected_gtf.json")))
LINE = b'chr1\thavana\texon\t11869\t12227\t.\t+\t.\tgene_id "ENSG00000223972"; exon_number 1;'


def with_field(k, value, line=LINE):
    f = line.split(b"\t")
    f[k] = value
    return b"\t".join(f)


def error_of(data):
    return G.read(data)[2]


# ---- the reference's pins ---------------------------------------------------------------------------------------------------
def test_fixture_row_and_count_as_the_reference_pins_them():
    data = open(os.path.join(GOLDEN, "test.gtf"), "rb").read()
    rows, keep, err = G.read(data)
    assert err is None and len(rows) == EXPECTED["count"] == 77 and all(keep)
    first = rows[0]
    want = EXPECTED["first_row"]
    assert [v.decode() if isinstance(v, bytes) else v for v in first[:8]] == want[:8]
    gene_ids = [v for k, v in first[8] if k == b"gene_id"]              # attributes['gene_id'][1]: DuckDB lists are 1-based
    assert gene_ids[0].decode() == want[8]
    assert [k for k, _ in first[8]] == [b"gene_id", b"transcript_id", b"exon_number", b"gene_name", b"gene_biotype", b"transcript_name", b"exon_id"]


def test_fixture_encodings_hold_the_same_bytes():
    import bz2
    import gzip
    from zstd_util import decompress_stream
    data = open(os.path.join(GOLDEN, "test.gtf"), "rb").read()
    assert gzip.decompress(open(os.path.join(GOLDEN, "test.gtf.gz"), "rb").read()) == data
    assert bz2.decompress(open(os.path.join(GOLDEN, "test.gtf.bz2"), "rb").read()) == data
    assert decompress_stream(open(os.path.join(GOLDEN, "test.gtf.zst"), "rb").read()) == (True, data)


# ---- schema rules, one test each --------------------------------------------------------------------------------------------
def test_rule_seqname_and_type_are_never_empty_source_is_taken_as_it_stands():
    assert error_of(with_field(0, b""))[1] == G.E_EMPTY_FIELD and error_of(with_field(2, b""))[1] == G.E_EMPTY_FIELD
    assert G.parse_line(with_field(1, b"."))[1] == b"." and G.parse_line(with_field(1, b""))[1] == b""


def test_rule_start_and_end_are_digits_only_from_1_to_2_63_minus_1_without_an_order_check():
    for k in (3, 4):
        for bad in (b"0", b"", b"+5", b"-5", b"1.0", b"1e3", b" 7", b"9223372036854775808", b"0x10"):
            assert error_of(with_field(k, bad))[1] == G.E_POSITION, (k, bad)
        assert G.parse_line(with_field(k, b"9223372036854775807"))[k] == G.I63
        assert G.parse_line(with_field(k, b"007"))[k] == 7
    row = G.parse_line(with_field(3, b"500", with_field(4, b"20")))
    assert (row[3], row[4]) == (500, 20)                                   # start > end is not an error


def test_rule_score_dot_is_null_otherwise_the_float_literal_grammar_and_exact_rounding():
    assert G.parse_line(LINE)[5] is None
    for text, bits in ((b"0", 0), (b"-0", 0x80000000), (b"1", 0x3F800000), (b"0.1", 0x3DCCCCCD), (b"1e-45", 1), (b"1e39", 0x7F800000),
                       (b"-inf", 0xFF800000), (b"Infinity", 0x7F800000), (b"NaN", 0x7FC00000), (b"7.", 0x40E00000), (b".5", 0x3F000000),
                       (b"16777217", 0x4B800000), (b"16777217.0000000000000000001", 0x4B800001), (b"16777219", 0x4B800002)):
        assert G.parse_line(with_field(5, text))[5] == bits, text
    for bad in (b"", b"..", b"1e", b"e5", b"0x1p3", b" 1", b"1 ", b"1,5", b"nan(1)", b"--1", b"infin"):
        assert error_of(with_field(5, bad))[1] == G.E_SCORE, bad


def test_rule_strand_dot_is_null_plus_minus_question_are_text():
    assert G.parse_line(with_field(6, b"."))[6] is None
    for s in (b"+", b"-", b"?"):
        assert G.parse_line(with_field(6, s))[6] == s
    for bad in (b"", b"++", b"*", b"f"):
        assert error_of(with_field(6, bad))[1] == G.E_STRAND, bad


def test_rule_frame_dot_is_null_0_1_2_are_text():
    assert G.parse_line(with_field(7, b"."))[7] is None
    for s in (b"0", b"1", b"2"):
        assert G.parse_line(with_field(7, s))[7] == s
    for bad in (b"", b"3", b"00", b"-1"):
        assert error_of(with_field(7, bad))[1] == G.E_FRAME, bad


def test_rule_attributes_are_never_null_an_empty_field_is_an_empty_map():
    assert G.parse_line(with_field(8, b""))[8] == []
    assert G.parse_line(with_field(8, b" ; "))[8] == []


# ---- line rules -------------------------------------------------------------------------------------------------------------
def test_rule_nine_fields_fewer_is_an_error_a_ninth_tab_belongs_to_the_attributes():
    assert error_of(LINE.rsplit(b"\t", 1)[0])[1] == G.E_FIELD_COUNT
    row = G.parse_line(LINE + b' note "a\tb";')
    assert row[8][-1] == (b"note", b"a\tb")
    assert G.parse_line(with_field(8, b"k v\tw", LINE), attributes=False)[8] == b"k v\tw"


def test_rule_a_line_that_begins_with_a_hash_gives_no_row_wherever_it_stands():
    data = b"#!genome-build GRCh38\n" + LINE + b"\n# a comment in the middle\n#\n" + LINE + b"\n##tail"
    rows, keep, err = G.read(data)
    assert err is None and len(rows) == 2 and keep == [False, True, False, False, True, False]
    assert error_of(b" #not a comment\n")[1] == G.E_FIELD_COUNT


def test_rule_an_empty_line_is_an_error():
    assert error_of(LINE + b"\n\n" + LINE + b"\n")[:3] == (1, G.E_FIELD_COUNT, len(LINE) + 1)
    assert error_of(b"\r\n")[1] == G.E_FIELD_COUNT


def test_rule_cr_before_lf_is_stripped_and_the_last_line_needs_no_newline():
    rows, _, err = G.read(LINE + b"\r\n" + LINE)
    assert err is None and rows[0] == rows[1] == G.parse_line(LINE)


def test_rule_utf8_is_validated_behind_the_fields_in_comment_lines_too():
    assert G.parse_line(with_field(0, b"chr\xc3\xa9"))[0] == b"chr\xc3\xa9"
    assert error_of(with_field(0, b"chr\xe9"))[1] == G.E_INVALID_UTF8
    assert error_of(with_field(3, b"x", with_field(0, b"chr\xe9")))[1] == G.E_POSITION      # the field's error comes first
    assert error_of(b"#caf\xe9\n")[1] == G.E_INVALID_UTF8


def test_rule_errors_go_by_the_field_count_then_left_to_right():
    assert error_of(b"\t\t\t0")[1] == G.E_FIELD_COUNT
    assert error_of(with_field(0, b"", with_field(3, b"x")))[1] == G.E_EMPTY_FIELD
    assert error_of(with_field(4, b"x", with_field(5, b"y")))[1] == G.E_POSITION
    assert error_of(with_field(5, b"y", with_field(6, b"x")))[1] == G.E_SCORE
    assert error_of(with_field(6, b"x", with_field(7, b"9")))[1] == G.E_STRAND
    assert error_of(with_field(7, b"9", with_field(8, b"k")))[1] == G.E_FRAME


# ---- the attribute grammar --------------------------------------------------------------------------------------------------
def attrs(text):
    return G.parse_attributes(text)


def attr_error(text):
    with pytest.raises(G.GtfError) as e:
        G.parse_attributes(text)
    assert e.value.code == G.E_ATTRIBUTES
    return e.value.offset


def test_rule_entries_are_key_spaces_value_separated_by_semicolons_in_file_order():
    assert attrs(b'gene_id "g1"; transcript_id "t1";') == [(b"gene_id", b"g1"), (b"transcript_id", b"t1")]
    assert attrs(b'b "2";a "1"') == [(b"b", b"2"), (b"a", b"1")]
    assert attrs(b'k    "v"  ;   k2 v2 ;') == [(b"k", b"v"), (b"k2", b"v2")]


def test_rule_a_quoted_value_may_hold_semicolons_and_spaces_and_loses_its_quotes():
    assert attrs(b'note "5; prime end, see x"; empty "";') == [(b"note", b"5; prime end, see x"), (b"empty", b"")]


def test_rule_an_unquoted_value_is_a_run_without_space_semicolon_or_quote():
    assert attrs(b"exon_number 1; level 2") == [(b"exon_number", b"1"), (b"level", b"2")]


def test_rule_a_repeated_key_stays_a_second_entry():
    assert attrs(b'tag "basic"; tag "CCDS";') == [(b"tag", b"basic"), (b"tag", b"CCDS")]


def test_rule_blank_segments_are_skipped():
    assert attrs(b' ;; a 1;; ;b 2; ;') == [(b"a", b"1"), (b"b", b"2")]


def test_rule_an_entry_without_a_value_is_an_error_where_the_parser_stops():
    assert attr_error(b"gene_id") == 7 and attr_error(b'a "1"; gene_id ; b 2') == 15 and attr_error(b"k   ") == 4


def test_rule_an_unterminated_quote_is_an_error_where_it_opens():
    assert attr_error(b'a "1"; note "never closed; b 2') == 12


def test_rule_bytes_behind_a_closing_quote_other_than_spaces_and_a_semicolon_are_an_error():
    assert attr_error(b'a "1"x; b 2') == 5 and attr_error(b'a "1" x') == 6 and attr_error(b'a "1""2"') == 5
    assert attrs(b'a "1"   ;b 2') == [(b"a", b"1"), (b"b", b"2")]


def test_rule_a_quote_stands_nowhere_but_around_a_value():
    assert attr_error(b'"k" v') == 0 and attr_error(b'k"e"y v') == 1 and attr_error(b'k v"x"') == 3 and attr_error(b'k v w') == 4


# ---- the library's surface, no GPU ------------------------------------------------------------------------------------------
def test_catalog_has_read_gtf_and_still_no_read_gff():
    from exon_duckdb_amd import ExgError, table_function

    con = table_function.connect()
    assert con.has_table_function("read_gtf") and not con.has_table_function("read_gff")
    for name in ("a/genes.gtf", "A/GENES.GTF.GZ", "x.gtf.zst", "x.gtf.bz2"):
        assert con.replacement_scan(name) == "read_gtf", name
    for other in ("x.gff", "x.gff3", "x.gtf.tar", "x.gtfx"):
        assert con.replacement_scan(other) is None, other
    with pytest.raises(ExgError) as e:
        con.table_function("read_gtf", "/nonexistent/missing.gtf")
    assert "missing.gtf" in str(e.value)
    with pytest.raises(ExgError):
        con.table_function("read_gff", "x.gff")


def test_map_type_spelling_and_decoding_of_pairs():
    from exon_duckdb_amd import abi, table_function
    tree = (abi.EXG_TYPE_MAP, "attributes", [(abi.EXG_TYPE_STRUCT, "entries", [(abi.EXG_TYPE_VARCHAR, "key", []), (abi.EXG_TYPE_VARCHAR, "value", [])])])
    assert table_function.type_sql(tree) == "MAP(VARCHAR, VARCHAR)" and table_function.abi_type("MAP") == abi.EXG_TYPE_MAP == 8


def test_new_reader_says_chunk_boundary_only():
    from exon_duckdb_amd import load_library
    from exon_duckdb_amd._lib import LIB_PATH

    class Stream(C.Structure):
        _fields_ = [("f", C.c_void_p * 5)]

    class Result(C.Structure):
        _fields_ = [("error", C.c_char_p)]
    load_library()
    lib = C.CDLL(LIB_PATH)
    lib.new_reader.restype = Result
    lib.new_reader.argtypes = [C.POINTER(Stream), C.c_char_p, C.c_size_t, C.c_char_p, C.c_char_p, C.c_char_p]
    st = Stream()
    res = lib.new_reader(C.byref(st), b"/nonexistent/x.gtf", 2048, None, b"gtf", None)
    assert res.error and b"chunk boundary only" in res.error


def test_parse_error_strings_workspace_and_algo_hint():
    from exon_duckdb_amd import abi, load_library
    lib = load_library()
    lib.exg_parse_error_string.restype = C.c_char_p
    lib.exg_parse_error_string.argtypes = [C.c_uint32]
    codes = [abi.EXG_PE_GTF_FIELD_COUNT, abi.EXG_PE_GTF_EMPTY_FIELD, abi.EXG_PE_GTF_POSITION, abi.EXG_PE_GTF_SCORE, abi.EXG_PE_GTF_STRAND,
             abi.EXG_PE_GTF_FRAME, abi.EXG_PE_GTF_ATTRIBUTES]
    assert codes == list(range(57, 64)) == [G.E_FIELD_COUNT, G.E_EMPTY_FIELD, G.E_POSITION, G.E_SCORE, G.E_STRAND, G.E_FRAME, G.E_ATTRIBUTES]
    texts = {lib.exg_parse_error_string(c) for c in codes}
    assert len(texts) == 7 and b"unknown parse error" not in texts
    assert lib.exg_parse_error_string(56) == lib.exg_parse_error_string(64) == b"unknown parse error"      # (56 stays unassigned: tests/test_bcf_host.py probes it)
    lib.exg_scan_workspace_bytes.restype = C.c_uint64
    lib.exg_scan_workspace_bytes.argtypes = [C.c_int, C.c_uint64]
    small, large = lib.exg_scan_workspace_bytes(abi.EXG_FMT_GTF, 0), lib.exg_scan_workspace_bytes(abi.EXG_FMT_GTF, 1 << 30)
    assert 0 < small and ((1 << 30) // 16) * 8 < large < (1 << 30)
    assert large - lib.exg_scan_workspace_bytes(abi.EXG_FMT_BED, 1 << 30) < 1 << 16           # BED's, plus the list of slow score literals
    assert abi.EXG_FMT_GTF == 8 and abi.EXG_GTF_COLUMNS == 9 and abi.EXG_RF_ROWS_SKIPPED == 128
    sample = G.mixed(G.rng(2), 400)
    assert lib.exg_scan_algo_hint(abi.EXG_FMT_GTF, sample, len(sample)) == abi.EXG_ALGO_FUSED_FULL
    lib.exg_gtf_attributes_workspace_bytes.restype = C.c_uint64
    lib.exg_gtf_attributes_workspace_bytes.argtypes = [C.c_uint64]
    assert 0 < lib.exg_gtf_attributes_workspace_bytes(0) < lib.exg_gtf_attributes_workspace_bytes(1 << 20) < 14 << 20


def test_gtf_mirrors_match_the_c_layout(tmp_path):
    from exon_duckdb_amd import abi

    structs = {"exg_gtf_scan_args": abi.GtfScanArgs, "exg_gtf_attributes_args": abi.GtfAttributesArgs,
               "struct exg_gtf_attributes_result": abi.GtfAttributesResult}
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs.items():
        prog.append(f'printf("{cname.split()[-1]} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            prog.append(f'printf("{cname.split()[-1]}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    prog.append('printf("consts %d %d %d %d\\n", EXG_FMT_GTF, EXG_GTF_COLUMNS, EXG_TYPE_MAP, (int)EXG_RF_ROWS_SKIPPED); return 0; }')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    got = dict(line.split() for line in lines if not line.startswith("consts"))
    for cname, cls in structs.items():
        cname = cname.split()[-1]
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)
    assert C.sizeof(abi.GtfAttributesResult) == 64
    assert [ln for ln in lines if ln.startswith("consts")] == ["consts 8 9 8 128"]


def test_gtf_format_is_opened_by_name(tmp_path):
    """exg_open knows the format: what stops a reader here is the missing device (or nothing), never the format's name; a filter on
    the attributes column is refused like the nested VCF columns"""
    from exon_duckdb_amd import ExgError, abi
    from exon_duckdb_amd.reader import ShardReader
    p = tmp_path / "x.gtf"
    p.write_bytes(LINE + b"\n")
    try:
        r = ShardReader(str(p), "GTF")
    except ExgError as e:
        assert e.code == abi.EXG_E_NO_DEVICE, (e.code, str(e))
    else:
        assert r.names == G.NAMES and r.types == [1, 1, 1, 2, 2, 3, 1, 1, 8]
        r.close()
        with pytest.raises(ExgError) as e:
            ShardReader(str(p), "gtf", filters="attributes = 'x'")
        assert e.value.code == abi.EXG_E_INVALID_ARG


def test_the_shim_still_compiles_against_the_stub_without_logical_type_map():
    """the shim reaches LogicalType::MAP through overload resolution: the stub has none, and the syntax-only compile passes with
    the LIST(STRUCT(key, value)) fallback"""
    stub = os.path.join(ROOT, "tests", "duckdb_stub")
    assert "MAP" not in open(os.path.join(stub, "duckdb.hpp")).read()
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", stub, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "exon_duckdb_amd", "csrc"), os.path.join(ROOT, "duckdb_shim", "exon_extension.cpp")])
