"""read_bam_file_records without a GPU: the Python BAM reader that is the oracle of the BAM tests against the reference's
pinned rows, the writer against the reader, the catalog / replacement scan / bind surface, the ctypes mirror of
exg_bam_scan_args, and the BAM header parser under ASan / UBSan."""
import ctypes as C
import gzip
import json
import os
import subprocess

import pytest

import bam_files as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "exon_gpu.h")
CSRC = os.path.join(ROOT, "exon_duckdb_amd", "csrc")
EXPECTED = json.load(open(os.path.join(GOLDEN, "expected_bam.json")))


def as_row(values):
    """a row of expected_bam.json (str / int / null) as the reader's tuple (bytes / int / None)"""
    return tuple(v.encode() if isinstance(v, str) else v for v in values)


def test_python_reader_reproduces_the_pinned_rows():
    p = B.parse(os.path.join(GOLDEN, "bam/example1.bam"))
    assert p.error is None and p.rows == [as_row(r) for r in EXPECTED["bam/example1.bam"]["rows"]]
    p = B.parse(os.path.join(GOLDEN, "bam-index/test.bam"))
    assert p.error is None and len(p.rows) == EXPECTED["bam-index/test.bam"]["count"] == 61
    assert p.rows[0] == as_row(EXPECTED["bam-index/test.bam"]["first_row"])
    assert all(r[2] == b"chr1" for r in p.rows)          # (why the full scan equals bam_query(..., 'chr1'))
    p = B.parse(os.path.join(GOLDEN, "bam/test.bam"))
    assert p.error is None and len(p.rows) == EXPECTED["bam/test.bam"]["count"] and len(p.refs) == EXPECTED["bam/test.bam"]["n_ref"]


def test_writer_reader_round_trip(tmp_path):
    refs = [(b"chr1", 1000), (b"a_reference_name_longer_than_twelve", 5)]
    recs = [B.record(b"q1", 99, 0, 9, 60, [(5, "M"), (2, "I"), (3, "D"), (4, "N"), (1, "S"), (6, "="), (7, "X")], 1, 99, 10, b"ACGTNACGTNACGTN",
                     bytes(range(15)), B.aux_z(b"RG", b"x")),
            B.record(b"unmapped", 4, -1, -1, 255, (), -1, -1, 0, b"ACG", None),
            B.record(b"empty", 0, 0, 0, 0, [(1, "H"), (1, "P")])]
    raw = B.header(refs, b"@HD\tVN:1.6\n") + b"".join(recs)
    path = tmp_path / "t.bam"
    path.write_bytes(B.bgzf(raw, cuts=[3, 40, 41, 77, len(raw) - 1], level=6) )
    assert gzip.decompress(path.read_bytes()) == raw
    p = B.parse(str(path))
    assert p.error is None and p.refs == refs
    assert p.rows[0] == (b"q1", 99, b"chr1", 10, 10 + 5 + 3 + 4 + 6 + 7 - 1, b"60", b"5M2I3D4N1S6=7X", refs[1][0], b"ACGTNACGTNACGTN",
                         bytes(33 + i for i in range(15)))
    assert p.rows[1] == (b"unmapped", 4, None, None, None, None, b"", None, b"ACG", b"")
    assert p.rows[2] == (b"empty", 0, b"chr1", 1, None, b"0", b"1H1P", None, b"", b"")
    # stored blocks, an empty member in the middle, a truncated record
    mixed = B.bgzf(raw[:50], stored=True, eof=False) + B.BGZF_EOF + B.bgzf(raw[50:], level=0)
    assert gzip.decompress(mixed) == raw
    assert B.parse_decoded(raw[:-1]).error == (2, B.E_TRUNCATED) and len(B.parse_decoded(raw[:-1]).rows) == 2
    big = tmp_path / "big.bam"
    n = B.write_repeated(str(big), B.header(refs), b"".join(recs), 50)
    assert len(B.parse(str(big)).rows) == 150 and n == len(B.header(refs)) + 50 * len(b"".join(recs))


def test_catalog_replacement_scan_and_bind():
    from exon_duckdb_amd import ExgError, load_library, table_function

    con = table_function.connect()
    assert con.has_table_function("read_bam_file_records")
    assert con.replacement_scan("./t/x.bam") == "read_bam_file_records"
    assert con.replacement_scan("./t/X.BAM") == "read_bam_file_records"
    for other in ("a/b.txt", "x.gz", "table.parquet", "x.sam"):
        assert con.replacement_scan(other) is None

    class RS(C.Structure):
        _fields_ = [("file_type", C.c_char_p)]
    lib = load_library()
    lib.replacement_scan.restype = RS
    lib.replacement_scan.argtypes = [C.c_char_p]
    assert lib.replacement_scan(b"a/b.bam").file_type == b"BAM"
    assert lib.replacement_scan(b"a/b.txt").file_type is None
    # test_bam_record_scan.test:19-22: a missing file is an error at bind time (no GPU is needed to say so)
    with pytest.raises(ExgError) as e:
        con.table_function("read_bam_file_records", "/nonexistent/missing.bam")
    assert "missing.bam" in str(e.value)


def test_sam_and_shards_are_refused_loudly_at_open(tmp_path):
    from exon_duckdb_amd import ExgError, abi
    from exon_duckdb_amd.reader import ShardReader

    p = tmp_path / "x.bam"
    p.write_bytes(B.bgzf(B.header()))
    with pytest.raises(ExgError) as e:
        ShardReader(str(p), "sam")
    assert e.value.code == abi.EXG_E_UNSUPPORTED and "sam" in str(e.value).lower()
    with pytest.raises(ExgError) as e:
        ShardReader(str(p), "BAM", shard_index=0, shard_count=2)
    assert e.value.code == abi.EXG_E_UNSUPPORTED and "shard" in str(e.value)


def test_new_reader_says_chunk_boundary_only(tmp_path):
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
    res = lib.new_reader(C.byref(st), b"/nonexistent/x.bam", 2048, None, b"bam", None)
    assert res.error and b"chunk boundary only" in res.error


def test_parse_error_strings_and_workspace():
    from exon_duckdb_amd import abi, load_library
    lib = load_library()
    lib.exg_parse_error_string.restype = C.c_char_p
    lib.exg_parse_error_string.argtypes = [C.c_uint32]
    texts = {lib.exg_parse_error_string(c) for c in range(abi.EXG_PE_BAM_BLOCK_SIZE, abi.EXG_PE_BAM_QUALITY + 1)}
    assert len(texts) == 7 and b"unknown parse error" not in texts
    lib.exg_scan_workspace_bytes.restype = C.c_uint64
    lib.exg_scan_workspace_bytes.argtypes = [C.c_int, C.c_uint64]
    small, large = lib.exg_scan_workspace_bytes(abi.EXG_FMT_BAM, 0), lib.exg_scan_workspace_bytes(abi.EXG_FMT_BAM, 1 << 30)
    assert 0 < small < 1 << 20 and (1 << 28) < large < (1 << 30)     # under one byte of workspace per input byte


def test_bam_scan_mirrors_match_the_c_layout(tmp_path):
    from exon_duckdb_amd import abi

    structs = {"exg_bam_scan_args": abi.BamScanArgs, "exg_bam_scan_result": abi.BamScanResult}
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs.items():
        prog.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            prog.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    prog.append('printf("stats %zu %zu\\n", sizeof(exg_reader_stats), offsetof(exg_reader_stats, bam_tiles)); return 0; }')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    got = dict(line.split() for line in lines if not line.startswith("stats"))
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert C.sizeof(abi.BamScanResult) == 64
    stats = [ln for ln in lines if ln.startswith("stats")][0].split()
    assert int(stats[1]) == C.sizeof(abi.ReaderStats) == 14 * 8 and int(stats[2]) == abi.ReaderStats.bam_tiles.offset   # (ABI 9's layout)


def test_bam_header_parser_under_asan_ubsan(tmp_path):
    exe = tmp_path / "bam_header_asan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           os.path.join(ROOT, "tests", "bam_header_driver.cpp"), os.path.join(CSRC, "exg_bam_header.cpp"), "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr[-3000:]
