"""read_sam_file_records without a GPU: the Python SAM reader that is the oracle of the SAM tests against the reference's
pinned row, every recalled rule of INTEGRATION.md's SAM table as a test of its own (someone with a real exon build can falsify
each), the same records as BAM and as SAM text through the two independent readers, the catalog / replacement scan / bind
surface, the error strings, the ctypes mirror of exg_sam_scan_args, the workspace, and the header-end finder as a program
under AddressSanitizer + UBSan."""
import bz2
import ctypes as C
import gzip
import json
import os
import subprocess

import pytest

import bam_files as BAM
import sam_files as S
from exon_duckdb_amd import abi

assert (abi.EXG_FMT_SAM, abi.EXG_PE_SAM_FIELD_COUNT) == (6, S.E_FIELD_COUNT)      # (the oracle's rules are those of a format the library has)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sam")
HEADER = os.path.join(ROOT, "include", "exon_gpu.h")
CSRC = os.path.join(ROOT, "exon_duckdb_amd", "csrc")
EXPECTED = json.load(open(os.path.join(GOLDEN, "expected_sam.json")))

LINE = b"q1\t99\tchr1\t100\t60\t10M\t=\t300\t210\tACGTACGTAC\tIIIIIIIIII"


def as_row(values):
    """a row of expected_sam.json (str / int / null) as the reader's tuple (bytes / int / None)"""
    return tuple(v.encode() if isinstance(v, str) else v for v in values)


def one(text):
    """the row of a single line, or the code it is refused with"""
    rows, err = S.read(text)
    return rows[0] if err is None else err[1]


def with_field(k, value, extra=()):
    f = LINE.split(b"\t")
    f[k] = value
    return b"\t".join(f + list(extra)) + b"\n"


def test_python_reader_reproduces_the_pinned_row():
    pinned = EXPECTED["example1.sam"]
    assert EXPECTED["columns"] == S.NAMES == BAM.NAMES and S.TYPES == BAM.TYPES and sorted(pinned["row_lines"].values()) == list(range(8, 18))
    want = [as_row(r) for r in pinned["rows"]]
    assert want == [(b"ref1_grp1_p001", 99, b"ref1", 1, 10, b"0", b"10M", b"ref1", b"CGAGCTCGGT", b"!!!!!!!!!!")]
    for f in pinned["files"]:
        raw = open(os.path.join(ROOT, "tests", "golden", f), "rb").read()
        if f.endswith(".zst"):
            continue  # (no zstd in the standard library: the device decodes it in tests/test_sam_gpu.py)
        raw = gzip.decompress(raw) if f.endswith(".gz") else bz2.decompress(raw) if f.endswith(".bz2") else raw
        assert S.read_file(raw) == (want, None), f
    for name, n in (("little.sam", 2), ("comment1.sam", 4)):
        rows, err = S.read_file(open(os.path.join(GOLDEN, name), "rb").read())
        assert err is None and len(rows) == n and rows == [as_row(r) for r in EXPECTED[name]["rows"]], name
    assert os.path.getsize(os.path.join(GOLDEN, "example1.sam")) == 437 and os.path.getsize(os.path.join(GOLDEN, "comment1.sam")) == 1365


def test_writer_reader_round_trip():
    rng = S.rng(1)
    seen = set()
    for _ in range(400):
        ln = S.line(rng)
        row = S.parse_line(ln)
        f = ln.split(b"\t")
        assert row[0] == f[0] and row[1] == int(f[1]) and row[6] == (b"" if f[5] == b"*" else f[5])
        seen |= {("ref", row[2] is None), ("mate", f[6] if f[6] in b"=*" else b"name"), ("seq", f[9] == b"*"), ("qual", f[10] == b"*"),
                 ("aux", len(f) > 11)}
    assert len(seen) == 11                                         # every shape of the writer came up
    data = S.header() + S.mixed(S.rng(2), 50, crlf_every=7, final_newline=False)
    rows, err = S.read_file(data)
    assert err is None and len(rows) == 50


# ---- the [RECALLED] rules, one test each ------------------------------------------------------------------------------------
def test_rule_header_is_the_leading_run_of_at_lines():
    rec = LINE + b"\n"
    assert S.read_file(S.header() + rec) == ([S.parse_line(LINE)], None)
    assert S.read_file(S.header()) == ([], None) and S.read_file(b"") == ([], None)      # header only, empty: 0 rows
    assert S.read_file(b"@CO\tno line feed") == ([], None)
    assert S.read_file(b"@HD\tVN:1.6\r\n" + rec)[0] == [S.parse_line(LINE)]
    # behind the header a line that starts with '@' is a record error: the field count first, then the name's first byte
    rows, err = S.read_file(S.header() + rec + b"@CO\tlate\n" + rec)
    assert len(rows) == 1 and err == (1, S.E_FIELD_COUNT, len(S.header()) + len(rec))
    assert one(with_field(0, b"@q1")) == S.E_HEADER_LINE


def test_rule_line_ends():
    row = S.parse_line(LINE)
    assert S.read(LINE + b"\n" + LINE + b"\r\n" + LINE) == ([row] * 3, None)           # LF, CRLF, an unterminated last line
    assert S.lines_of(b"a\r\r\nb") == [(0, b"a\r"), (4, b"b")]                           # one CR is stripped, not two
    assert one(LINE + b"\r\r\n") == S.E_LENGTHS                                           # (the other one is QUAL's eleventh byte)
    assert one(b"\n") == S.E_FIELD_COUNT and one(b"\r\n") == S.E_FIELD_COUNT             # an empty line is an error


def test_rule_field_count_and_empty_fields():
    f = LINE.split(b"\t")
    assert one(b"\t".join(f[:10]) + b"\n") == S.E_FIELD_COUNT
    assert one(b"\t".join(f[:10]) + b"\t\n") == S.E_EMPTY_FIELD                          # eleven fields, the last one empty
    assert one(LINE + b"\tNM:i:0\t\t\tXX:Z:\n") == S.parse_line(LINE)                      # aux fields are not read, empty ones included
    for k in range(11):
        assert one(with_field(k, b"")) == S.E_EMPTY_FIELD, k


def test_rule_numbers_are_digits_only():
    for k, code in ((1, S.E_FLAG), (3, S.E_POSITION), (4, S.E_MAPQ)):
        for bad in (b"+1", b"-1", b" 1", b"1 ", b"1.0", b"0x1", b"1e1"):
            assert one(with_field(k, bad)) == code, (k, bad)
        assert one(with_field(k, b"0000000000000000000000001"))[0] == b"q1"               # leading zeros are digits


def test_rule_flag_range():
    assert one(with_field(1, b"65535"))[1] == 65535 and one(with_field(1, b"0"))[1] == 0
    assert one(with_field(1, b"65536")) == S.E_FLAG


def test_rule_start_is_pos_and_zero_is_null():
    assert one(with_field(3, b"1"))[3:5] == (1, 10) and one(with_field(3, b"0"))[3:5] == (None, None)
    assert one(with_field(3, b"2147483647"))[3] == 2147483647 and one(with_field(3, b"2147483648")) == S.E_POSITION


def test_rule_mapping_quality_is_canonical_text_and_255_is_null():
    assert one(with_field(4, b"007"))[5] == b"7" and one(with_field(4, b"000"))[5] == b"0" and one(with_field(4, b"60"))[5] == b"60"
    assert one(with_field(4, b"255"))[5] is None and one(with_field(4, b"0255"))[5] is None and one(with_field(4, b"254"))[5] == b"254"
    assert one(with_field(4, b"256")) == S.E_MAPQ


def test_rule_reference_and_mate_reference():
    assert one(with_field(2, b"*"))[2] is None and one(with_field(2, b"**"))[2] == b"**"
    assert one(with_field(6, b"*"))[7] is None and one(with_field(6, b"chr2"))[7] == b"chr2"
    assert one(with_field(6, b"="))[7] == b"chr1" and one(with_field(6, b"=="))[7] == b"=="
    f = LINE.split(b"\t")
    f[2], f[6] = b"*", b"="
    assert S.parse_line(b"\t".join(f))[7] is None                                        # `=` of an absent reference


def test_rule_cigar():
    assert one(with_field(5, b"*"))[6] == b"" and one(with_field(5, b"*"))[4] == 99       # span 0: end = start - 1
    assert one(with_field(5, b"3S4M1I2D1N1=1X5H6P"))[4] == 100 + 4 + 2 + 1 + 1 + 1 - 1
    assert one(with_field(5, b"268435455M"))[6] == b"268435455M" and one(with_field(5, b"268435456M")) == S.E_CIGAR
    for bad in (b"M", b"10", b"10M5", b"10m", b"10B", b"1 0M", b"**", b"-1M", b"+1M", b"10M*"):
        assert one(with_field(5, bad)) == S.E_CIGAR, bad
    assert one(with_field(5, b"0010M"))[6] == b"0010M"                                    # taken verbatim


def test_rule_end_from_the_cigar_in_64_bits():
    assert one(with_field(3, b"0"))[4] is None                                            # without a start
    assert one(with_field(5, b"*").replace(b"\t100\t", b"\t1\t"))[3:5] == (1, None)         # below 1
    big = b"268435455M" * 8                                                               # span 2^31 - 8
    assert one(with_field(5, big).replace(b"\t100\t", b"\t8\t"))[4] == 2147483647         # exactly INTEGER's maximum
    assert one(with_field(5, big).replace(b"\t100\t", b"\t9\t"))[3:5] == (9, None)        # one past it
    assert one(with_field(5, b"268435455N" * 40))[4] is None                              # the sum passes 2^32 without wrapping


def test_rule_sequence_and_quality():
    assert one(with_field(9, b"*"))[8:] == (b"", b"IIIIIIIIII") and one(with_field(10, b"*"))[8:] == (b"ACGTACGTAC", b"")
    f = LINE.split(b"\t")
    f[9] = f[10] = b"*"
    assert S.parse_line(b"\t".join(f))[8:] == (b"", b"")
    # QUAL `*` is `*` wherever the aux tabs fall: here one lies exactly len(SEQ) bytes behind it
    assert one(with_field(9, b"ACGTACGT", [b"NM:i:0"]).replace(b"IIIIIIIIII", b"*"))[8:] == (b"ACGTACGT", b"")
    assert one(with_field(10, b"IIIIIIIII")) == S.E_LENGTHS and one(with_field(10, b"IIIIIIIIIII")) == S.E_LENGTHS
    assert one(with_field(9, b"acgtnNRYKM"))[8] == b"acgtnNRYKM"            # the alphabet is not validated
    assert one(with_field(10, b"~~~~~~~ ~~"))[9] == b"~~~~~~~ ~~"
    assert one(with_field(7, b"x"))[0] == b"q1" and one(with_field(8, b"y"))[0] == b"q1"   # PNEXT / TLEN: only their tabs


def test_rule_error_precedence():
    assert one(b"\t".join([b"", b"x", b"", b"x", b"x", b"x"]) + b"\n") == S.E_FIELD_COUNT     # the field count comes first
    assert one(with_field(1, b"x").replace(b"\t100\t", b"\ty\t")) == S.E_FLAG                    # then the leftmost field
    assert one(with_field(4, b"999").replace(b"\t10M\t", b"\t10Q\t")) == S.E_MAPQ
    assert one(with_field(5, b"1Q").replace(b"IIIIIIIIII", b"II")) == S.E_CIGAR
    assert one(with_field(3, b"x").replace(b"q1", b"q\xff")) == S.E_POSITION                      # UTF-8 behind the fields
    assert one(LINE.replace(b"q1", b"q\xff") + b"\n") == S.E_INVALID_UTF8
    assert one(LINE + b"\tCO:Z:\xc3\xa9\n")[0] == b"q1" and one(LINE + b"\tCO:Z:\xe9\n") == S.E_INVALID_UTF8
    rows, err = S.read(LINE + b"\n" + with_field(1, b"x") + with_field(3, b"x"))
    assert len(rows) == 1 and err == (1, S.E_FLAG, len(LINE) + 1)                                  # the first failing line in file order


# ---- the same records as BAM and as SAM text -----------------------------------------------------------------------------------
def cross_format_records():
    """keyword arguments of bam_files.record(): every NULL, `=` / other / absent mates, absent SEQ / QUAL, every CIGAR operation"""
    recs = [dict(name=b"ref1_grp1_p001", flag=99, ref=0, pos=0, mapq=0, cigar=[(10, "M")], next_ref=0, next_pos=24, tlen=34,
                 seq=b"CGAGCTCGGT", qual=bytes(10)),
            dict(name=b"unmapped", flag=4),
            dict(name=b"mate_elsewhere", flag=1, ref=1, pos=999, mapq=60, cigar=[(3, "S"), (4, "M"), (1, "I"), (2, "D"), (1, "N"), (1, "="), (1, "X"), (5, "H"), (6, "P")],
                 next_ref=2, next_pos=5, seq=b"ACGTNACGTN", qual=bytes(range(10))),
            dict(name=b"no_qual", flag=16, ref=2, pos=5, mapq=255, cigar=[(4, "M")], seq=b"ACGT"),
            dict(name=b"no_seq", flag=0, ref=0, pos=7, mapq=1, cigar=[(4, "M")]),
            dict(name=b"end_past_integer", ref=0, pos=2147483600, mapq=3, cigar=[(100, "M")], seq=b"A", qual=b"\x05"),
            dict(name=b"iupac", ref=3, pos=1, mapq=254, cigar=[(16, "=")], next_ref=-1, seq=BAM.SEQ_CODES, qual=bytes([93] * 16))]
    import random
    rng = random.Random(5)
    for i in range(40):
        n = rng.choice((1, 35, 150))
        recs.append(dict(name=b"r%d" % i, flag=rng.randrange(4096), ref=rng.randrange(-1, 4), pos=rng.randrange(-1, 10 ** 8), mapq=rng.choice((0, 30, 255)),
                         cigar=[(n, "M")], next_ref=rng.randrange(-1, 4), next_pos=rng.randrange(-1, 10 ** 8), tlen=rng.randrange(-500, 500),
                         seq=bytes(rng.choice(b"ACGT") for _ in range(n)), qual=bytes(rng.randrange(0, 94) for _ in range(n))))
    return recs


def test_cross_format_bam_and_sam_text_give_equal_rows():
    recs = cross_format_records()
    bam = BAM.parse_decoded(BAM.header(S.REFS) + b"".join(BAM.record(**r) for r in recs))
    text = S.header(S.REFS) + b"".join(S.from_bam_fields(S.REFS, **r) + b"\n" for r in recs)
    rows, err = S.read_file(text)
    assert bam.error is None and err is None and len(rows) == len(recs) == 47
    assert rows == bam.rows
    assert rows[0] == (b"ref1_grp1_p001", 99, b"chr1", 1, 10, b"0", b"10M", b"chr1", b"CGAGCTCGGT", b"!!!!!!!!!!")
    assert rows[1][2:8] == (None, None, None, None, b"", None) and rows[5][3:5] == (2147483601, None)


# ---- the library's surface, no GPU ----------------------------------------------------------------------------------------
def test_catalog_and_bind():
    """(the replacement scan does not answer `.sam`: tests/test_bam_host.py holds `x.sam` to no replacement, so the table function
    is called by name)"""
    from exon_duckdb_amd import ExgError, table_function

    con = table_function.connect()
    assert con.has_table_function("read_sam_file_records")
    for other in ("a/b.txt", "x.gz", "x.cram", "x.sam.tar", "x.sami"):
        assert con.replacement_scan(other) is None, other
    # test_sam_record_scan.test:19-22: a missing file is an error at bind time (no GPU is needed to say so)
    with pytest.raises(ExgError) as e:
        con.table_function("read_sam_file_records", "/nonexistent/missing.sam")
    assert "missing.sam" in str(e.value)


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
    res = lib.new_reader(C.byref(st), b"/nonexistent/x.sam", 2048, None, b"sam", None)
    assert res.error and b"chunk boundary only" in res.error


def test_parse_error_strings_workspace_and_algo_hint():
    from exon_duckdb_amd import abi, load_library
    lib = load_library()
    lib.exg_parse_error_string.restype = C.c_char_p
    lib.exg_parse_error_string.argtypes = [C.c_uint32]
    codes = [abi.EXG_PE_SAM_FIELD_COUNT, abi.EXG_PE_SAM_EMPTY_FIELD, abi.EXG_PE_SAM_HEADER_LINE, abi.EXG_PE_SAM_FLAG, abi.EXG_PE_SAM_POSITION,
             abi.EXG_PE_SAM_MAPQ, abi.EXG_PE_SAM_CIGAR, abi.EXG_PE_SAM_LENGTHS]
    assert codes == list(range(35, 43)) == [S.E_FIELD_COUNT, S.E_EMPTY_FIELD, S.E_HEADER_LINE, S.E_FLAG, S.E_POSITION, S.E_MAPQ, S.E_CIGAR, S.E_LENGTHS]
    texts = {lib.exg_parse_error_string(c) for c in codes}
    assert len(texts) == 8 and b"unknown parse error" not in texts
    assert lib.exg_parse_error_string(34) == lib.exg_parse_error_string(43) == b"unknown parse error"      # (34 stays unassigned)
    lib.exg_scan_workspace_bytes.restype = C.c_uint64
    lib.exg_scan_workspace_bytes.argtypes = [C.c_int, C.c_uint64]
    small, large = lib.exg_scan_workspace_bytes(abi.EXG_FMT_SAM, 0), lib.exg_scan_workspace_bytes(abi.EXG_FMT_SAM, 1 << 30)
    # the line index holds the densest valid input: a line per 22 bytes (eleven one-byte fields, ten tabs, LF), 8 bytes each
    dense = b"q\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*"
    assert len(dense) == 21 and S.parse_line(dense) == (b"q", 0, None, None, None, b"0", b"", None, b"", b"")
    assert 0 < small and ((1 << 30) // 22) * 8 < large < (1 << 30) // 2
    assert abi.EXG_FMT_SAM == 6 and abi.EXG_SAM_COLUMNS == 10 and lib.exg_abi_version() == abi.EXG_ABI_VERSION == 9
    sample = S.mixed(S.rng(2), 400)
    assert lib.exg_scan_algo_hint(abi.EXG_FMT_SAM, sample, len(sample)) == abi.EXG_ALGO_FUSED_FULL
    assert lib.exg_scan_algo_hint(abi.EXG_FMT_SAM, None, 0) == abi.EXG_ALGO_FUSED_FULL


def test_sam_scan_mirror_matches_the_c_layout(tmp_path):
    from exon_duckdb_amd import abi

    cname, cls = "exg_sam_scan_args", abi.SamScanArgs
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
            f'printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        prog.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    prog.append('printf("fmt %d cols %d\\n", EXG_FMT_SAM, EXG_SAM_COLUMNS); return 0; }')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    got = dict(line.split() for line in lines if not line.startswith("fmt"))
    assert int(got[cname]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname
    assert [ln for ln in lines if ln.startswith("fmt")] == ["fmt 6 cols 10"]


def test_sam_format_is_opened_by_name(tmp_path):
    """exg_open knows the sixth format: what stops a reader here is the missing device (or nothing), never the format's name"""
    from exon_duckdb_amd import ExgError, abi
    from exon_duckdb_amd.reader import ShardReader
    p = tmp_path / "x.sam"
    p.write_bytes(S.header() + LINE + b"\n")
    try:
        r = ShardReader(str(p), "SAM")
    except ExgError as e:
        assert e.code == abi.EXG_E_NO_DEVICE, (e.code, str(e))
    else:
        r.close()


def test_gzip_members_read_as_plain_sam_are_refused_at_open(tmp_path):
    """SAM is text: a BAM file (or a gzip'd SAM whose name hides it) opened as uncompressed "sam" is EXG_E_UNSUPPORTED, before a
    device is asked for; the same bytes with the compression named get past that check"""
    from exon_duckdb_amd import ExgError, abi
    from exon_duckdb_amd.reader import ShardReader
    text = S.header() + LINE + b"\n"
    for name, data in (("x.bam", BAM.bgzf(BAM.header())), ("hidden.sam", gzip.compress(text, 6, mtime=0))):
        p = tmp_path / name
        p.write_bytes(data)
        with pytest.raises(ExgError) as e:
            ShardReader(str(p), "sam")
        assert e.value.code == abi.EXG_E_UNSUPPORTED and "gzip members" in str(e.value) and name in str(e.value)
    for name, kw in (("named.sam.gz", {}), ("hidden.sam", {"compression": "gzip"})):
        p = tmp_path / name
        p.write_bytes(gzip.compress(text, 6, mtime=0))
        try:
            ShardReader(str(p), "sam", **kw).close()
        except ExgError as e:
            assert e.code == abi.EXG_E_NO_DEVICE, (name, e.code, str(e))


def test_header_end_finder_under_asan_ubsan(tmp_path):
    """the host C++ that finds the header's end, as a program of its own: a header ending exactly at the buffer's end, none,
    header only, a CR before the LF, every cut"""
    exe = tmp_path / "sam_header"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           "-o", str(exe), os.path.join(ROOT, "tests", "sam_header_driver.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], env=env, capture_output=True, text=True)
    assert res.returncode == 0 and "cases ok" in res.stdout, (res.returncode, res.stdout + res.stderr)
