"""read_bed_file without a GPU: the Python BED reader that is the oracle of the BED tests against the reference's pinned
row, every recalled rule of INTEGRATION.md's BED table as a test of its own (someone with a real exon build can falsify each),
the catalog / replacement scan / bind surface, the error strings, the ctypes mirror of exg_bed_scan_args and the workspace."""
import ctypes as C
import gzip
import json
import os
import subprocess

import pytest

import bed_files as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "exon_gpu.h")
EXPECTED = json.load(open(os.path.join(GOLDEN, "expected_bed.json")))


def as_row(values):
    """a row of expected_bed.json (str / int / null) as the reader's tuple (bytes / int / None)"""
    return tuple(v.encode() if isinstance(v, str) else v for v in values)


def one(text):
    """the row of a single line, or the code it is refused with"""
    rows, err = B.read(text)
    return rows[0] if err is None else err[1]


LINE12 = b"sq0\t7\t13\tn\t5\t+\t7\t13\t1,2,3\t2\t2,1\t0,3"


def with_field(k, value, n_fields=12):
    f = LINE12.split(b"\t")[:n_fields]
    f[k] = value
    return b"\t".join(f) + b"\n"


def test_python_reader_reproduces_the_pinned_rows():
    pinned = EXPECTED["test3.bed"]
    assert EXPECTED["columns"] == B.NAMES and sorted(pinned["row_lines"].values()) == list(range(7, 19))
    for f in pinned["files"]:
        raw = open(os.path.join(GOLDEN, f), "rb").read()
        if f.endswith(".gz"):
            raw = gzip.decompress(raw)
        if f.endswith(".zst"):
            continue  # (no zstd in the standard library: the device decodes it in tests/test_bed_gpu.py)
        rows, err = B.read(raw)
        assert err is None and rows == [as_row(r) for r in pinned["rows"]], f
    rows, err = B.read(open(os.path.join(GOLDEN, "bed/hg38.head.bed"), "rb").read())
    assert err is None and rows == [as_row(r) for r in EXPECTED["hg38.head.bed"]["rows"]] and len(rows) == 10


def test_writer_reader_round_trip():
    rng = B.rng(1)
    for n in B.FIELD_COUNTS:
        for _ in range(50):
            ln = B.line(rng, n)
            row = B.parse_line(ln)
            assert sum(v is not None for v in row) <= n and all(v is None for v in row[(n if n < 12 else 12):])
    data = B.mixed(rng, 500, crlf_every=7, final_newline=False)
    rows, err = B.read(data)
    assert err is None and len(rows) == 500 and not data.endswith(b"\n")
    assert B.read(data + b"\n")[0] == rows and {sum(v is not None for v in r) for r in rows} >= {3}
    assert B.read(b"") == ([], None)


# ---- the rules the reference's tests pin (test_bed_io.test:4-18) ----------------------------------------------------
def test_pinned_start_and_thick_start_are_one_based_end_is_as_written():
    row = one(b"sq0\t7\t13\t.\t0\t.\t7\t13\t0\t2\t2,1\t0,3\n")
    assert (row[1], row[2], row[6], row[7]) == (8, 13, 8, 13)


def test_pinned_dot_name_dot_strand_zero_score_zero_color_are_null():
    row = one(b"sq0\t7\t13\t.\t0\t.\t7\t13\t0\t2\t2,1\t0,3\n")
    assert row[3] is None and row[4] is None and row[5] is None and row[8] is None
    assert (row[9], row[10], row[11]) == (2, b"2,1", b"0,3")


# ---- [RECALLED] rules: exon 0.2.6 over noodles-bed 0.10.0 -------------------------------------------------------------
def test_recalled_score_zero_is_null_other_scores_are_1_to_1000():
    assert one(with_field(4, b"0"))[4] is None
    assert one(with_field(4, b"1"))[4] == 1 and one(with_field(4, b"1000"))[4] == 1000
    for bad in (b"1001", b"00", b"+0", b".", b"", b"-1", b"1.5"):
        assert one(with_field(4, bad)) == B.E_SCORE, bad


def test_recalled_color_zero_is_null_otherwise_three_decimals_0_to_255():
    assert one(with_field(8, b"0"))[8] is None
    assert one(with_field(8, b"255,0,0"))[8] == b"255,0,0" and one(with_field(8, b"0,0,0"))[8] == b"0,0,0"
    for bad in (b"256,0,0", b"1,2", b"1,2,3,4", b".", b"", b"1,,3", b"a,b,c", b"1, 2,3"):
        assert one(with_field(8, bad)) == B.E_COLOR, bad


def test_recalled_field_counts_10_and_11_are_refused_and_so_are_1_2_13():
    f = LINE12.split(b"\t")
    for n in range(1, 14):
        got = one(b"\t".join((f + [b"x"])[:n]) + b"\n")
        assert (got == B.E_FIELD_COUNT) == (n not in B.FIELD_COUNTS), n
    assert one(b"sq0 7 13\n") == B.E_FIELD_COUNT          # the only separator is the tab


def test_recalled_integers_are_rust_usize_from_str():
    assert one(b"c\t+7\t13\n")[1] == 8                    # an optional single '+'
    assert one(b"c\t007\t13\n")[1] == 8
    for bad in (b"", b"-1", b" 5", b"5 ", b"++7", b"7a", b"0x7", b"1e3"):
        assert one(b"c\t" + bad + b"\t13\n") == B.E_POSITION, bad
    assert one(b"c\t%d\t%d\n" % (2 ** 63 - 2, 2 ** 63 - 1))[1:3] == (2 ** 63 - 1, 2 ** 63 - 1)
    assert one(b"c\t%d\t13\n" % (2 ** 63 - 1)) == B.E_POSITION     # start + 1 must fit
    assert one(b"c\t1\t%d\n" % 2 ** 63) == B.E_POSITION
    assert one(b"c\t1\t" + b"9" * 20 + b"\n") == B.E_POSITION


def test_recalled_end_zero_is_refused_start_zero_is_not():
    assert one(b"c\t0\t1\n")[1:3] == (1, 1)
    assert one(b"c\t0\t0\n") == B.E_POSITION
    assert one(with_field(7, b"0")) == B.E_POSITION       # thick_end likewise


def test_recalled_strand():
    assert one(with_field(5, b"+"))[5] == b"+" and one(with_field(5, b"-"))[5] == b"-" and one(with_field(5, b"."))[5] is None
    for bad in (b"", b"*", b"++", b"plus"):
        assert one(with_field(5, bad)) == B.E_STRAND, bad


def test_recalled_block_lists_take_block_count_items_and_drop_a_trailing_comma():
    assert one(with_field(10, b"2,1,"))[10] == b"2,1"
    assert one(with_field(10, b"2,1,9,9"))[10] == b"2,1"          # ends before the separator of item block_count + 1
    assert one(with_field(10, b"2")) == B.E_BLOCKS                # fewer items
    assert one(with_field(10, b"2,")) == B.E_BLOCKS
    assert one(with_field(10, b"2,x")) == B.E_BLOCKS
    row = one(with_field(9, b"0"))
    assert (row[9], row[10], row[11]) == (0, b"", b"")            # block_count 0: empty strings, not NULL
    assert one(with_field(11, b"0")) == B.E_BLOCKS


def test_recalled_every_line_is_a_record_no_header_no_comments():
    for text in (b"track name=x\n", b"browser position chr1:1-2\n", b"#chrom\tstart\tend\n", b"\n"):
        rows, err = B.read(text + b"c\t1\t2\n")
        assert rows == [] and err[0] == 0 and err[1] in (B.E_FIELD_COUNT, B.E_POSITION), text
    assert one(b"track name=x\n") == B.E_FIELD_COUNT and one(b"\n") == B.E_FIELD_COUNT
    assert B.read(b"c\t1\t2\n\n") == ([(b"c", 2, 2) + (None,) * 9], (1, B.E_FIELD_COUNT, 6))    # an empty line in the middle or at the end


def test_line_ends_reference_name_utf8_and_precedence():
    assert one(b"c\t1\t2\r\n") == one(b"c\t1\t2\n") == one(b"c\t1\t2")
    assert one(b"c\t1\t2\r") == B.E_POSITION                       # an unterminated line keeps its CR
    assert one(b"c\t1\t2\tn\r\r\n")[3] == b"n\r"                   # ONE CR is stripped
    assert one(b"\t1\t2\n") == B.E_REFERENCE_NAME
    assert one(b"c\t1\t2\tn\xc3\xa9\n")[3] == b"n\xc3\xa9" and one(b"c\t1\t2\tn\xff\n") == B.E_INVALID_UTF8
    assert one(b"\t1\tx\tn\xff\n") == B.E_REFERENCE_NAME           # fields left to right, then UTF-8
    assert one(b"c\tx\t2\tn\xff\t5000\n") == B.E_POSITION
    rows, err = B.read(b"c\t1\t2\nc\t1\t0\nc\tx\t2\n")
    assert len(rows) == 1 and err == (1, B.E_POSITION, 6)         # the first failing line in file order


# ---- the library's surface, no GPU ----------------------------------------------------------------------------------------
def test_catalog_replacement_scan_and_bind():
    from exon_duckdb_amd import ExgError, load_library, table_function

    con = table_function.connect()
    assert con.has_table_function("read_bed_file")
    for name in ("x.bed", "X.BED.GZ", "x.bed.zst", "./t/x.bed.bz2"):
        assert con.replacement_scan(name) == "read_bed_file", name
    for other in ("a/b.txt", "x.gz", "x.bedgraph", "x.bed.tar"):
        assert con.replacement_scan(other) is None, other

    class RS(C.Structure):
        _fields_ = [("file_type", C.c_char_p)]
    lib = load_library()
    lib.replacement_scan.restype = RS
    lib.replacement_scan.argtypes = [C.c_char_p]
    assert lib.replacement_scan(b"a/b.bed").file_type == b"BED"
    with pytest.raises(ExgError) as e:
        con.table_function("read_bed_file", "/nonexistent/missing.bed")
    assert "missing.bed" in str(e.value)


def test_new_reader_says_chunk_boundary_only():
    from exon_duckdb_amd import load_library
    from exon_duckdb_amd._lib import LIB_PATH

    class Stream(C.Structure):
        _fields_ = [("f", C.c_void_p * 5)]

    class Result(C.Structure):
        _fields_ = [("error", C.c_char_p)]
    load_library()
    lib = C.CDLL(LIB_PATH)      # a handle of this test's own: the shared one keeps the signature exon_duckdb_amd.arrow gave new_reader
    lib.new_reader.restype = Result
    lib.new_reader.argtypes = [C.POINTER(Stream), C.c_char_p, C.c_size_t, C.c_char_p, C.c_char_p, C.c_char_p]
    st = Stream()
    res = lib.new_reader(C.byref(st), b"/nonexistent/x.bed", 2048, None, b"bed", None)
    assert res.error and b"chunk boundary only" in res.error


def test_parse_error_strings_workspace_and_algo_hint():
    from exon_duckdb_amd import abi, load_library
    lib = load_library()
    lib.exg_parse_error_string.restype = C.c_char_p
    lib.exg_parse_error_string.argtypes = [C.c_uint32]
    codes = [abi.EXG_PE_BED_FIELD_COUNT, abi.EXG_PE_BED_REFERENCE_NAME, abi.EXG_PE_BED_POSITION, abi.EXG_PE_BED_SCORE,
             abi.EXG_PE_BED_STRAND, abi.EXG_PE_BED_COLOR, abi.EXG_PE_BED_BLOCKS]
    assert codes == list(range(22, 29)) == [B.E_FIELD_COUNT, B.E_REFERENCE_NAME, B.E_POSITION, B.E_SCORE, B.E_STRAND, B.E_COLOR, B.E_BLOCKS]
    texts = {lib.exg_parse_error_string(c) for c in codes}
    assert len(texts) == 7 and b"unknown parse error" not in texts
    assert lib.exg_parse_error_string(29) == b"unknown parse error"
    lib.exg_scan_workspace_bytes.restype = C.c_uint64
    lib.exg_scan_workspace_bytes.argtypes = [C.c_int, C.c_uint64]
    small, large = lib.exg_scan_workspace_bytes(abi.EXG_FMT_BED, 0), lib.exg_scan_workspace_bytes(abi.EXG_FMT_BED, 1 << 30)
    assert 0 < small and 0 < large < (1 << 30)                     # under one byte of workspace per input byte
    assert abi.EXG_FMT_BED == 5 and abi.EXG_BED_COLUMNS == 12 and lib.exg_abi_version() == abi.EXG_ABI_VERSION == 9
    sample = B.mixed(B.rng(2), 400)
    assert lib.exg_scan_algo_hint(abi.EXG_FMT_BED, sample, len(sample)) == abi.EXG_ALGO_FUSED_FULL
    assert lib.exg_scan_algo_hint(abi.EXG_FMT_BED, None, 0) == abi.EXG_ALGO_FUSED_FULL


def test_bed_scan_mirror_matches_the_c_layout(tmp_path):
    from exon_duckdb_amd import abi

    cname, cls = "exg_bed_scan_args", abi.BedScanArgs
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
            f'printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        prog.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    prog.append('printf("fmt %d cols %d\\n", EXG_FMT_BED, EXG_BED_COLUMNS); return 0; }')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    got = dict(line.split() for line in lines if not line.startswith("fmt"))
    assert int(got[cname]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname
    assert [ln for ln in lines if ln.startswith("fmt")] == ["fmt 5 cols 12"]
