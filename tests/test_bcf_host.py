"""read_bcf_file_records without a GPU: the Python renderer that is the oracle of the BCF tests against the reference's pair
index.bcf / index.vcf (which pins the rule set), the header parser and dictionary builder under ASan / UBSan as a program of
its own, the float renderer compiled for the host on millions of bit patterns, and the ABI's mirrors."""
import ctypes as C
import gzip
import os
import re
import subprocess

import pytest

import bam_files as BAM
import bcf_files as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exon_duckdb_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "exon_gpu.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_renderer_on_index_bcf_gives_index_vcf():
    """the rules of INTEGRATION.md (BCF), as bcf_files.py states them, turn the 621 records of index.bcf into the 621 data lines of
    index.vcf: text-equal, or float32-equal field by field (two lines spell a float with more digits)"""
    raw = gzip.decompress(open(os.path.join(GOLDEN, "bcf", "index.bcf"), "rb").read())
    text, r = B.render_file(raw)
    vcf = open(os.path.join(GOLDEN, "vcf", "index.vcf"), "rb").read()
    lines = [ln for ln in vcf.split(b"\n") if ln and not ln.startswith(b"#")]
    assert r.error is None and len(r.lines) == len(lines) == 621
    exact = sum(a == b for a, b in zip(r.lines, lines))
    assert exact == 619
    for a, b in zip(r.lines, lines):
        assert B.text_equal(a, b) is None, (a, b)
    assert B.text_equal(b"1\t5\t.\tA\tC\t0.5\n", b"1\t5\t.\tA\tC\t0.25\n") is not None        # (the comparison does tell floats apart)
    assert B.text_equal(b"1\t5\t.\tA\tC\t5e-1\n", b"1\t5\t.\tA\tC\t0.5\n") is None
    # the header's text is the VCF's header but for the IDX= attributes and the PASS filter bcftools adds
    strip = lambda t: [re.sub(rb",IDX=\d+", b"", ln) for ln in t.split(b"\n") if ln and b"ID=PASS" not in ln and not ln.startswith(b"##bcftools")]
    assert strip(text) == strip(b"\n".join(ln for ln in vcf.split(b"\n") if ln.startswith(b"#")))


def test_writer_and_renderer_agree_on_what_they_share():
    """the writer's bytes through the renderer: the values that went in (a self-check of the test's own tools)"""
    text = B.header_text(infos=[("DP", "1", "Integer"), ("AF", "A", "Float")], formats=[("GT", "1", "String"), ("PL", "G", "Integer")], samples=("a", "b"), idx=True)
    strings, contigs, n = B.dictionaries(text)
    assert strings[:5] == [b"PASS", b"DP", b"AF", b"GT", b"PL"] and contigs == [b"1", b"2"] and n == 2
    rec = B.record(chrom=1, pos=99, id_=b"rs1", alleles=(b"A", b"C", b"GT"), qual=12.5, filters=[0],
                   info=[(1, B.ints([7])), (2, B.floats([0.5, B.MISSING]))], n_sample=2,
                   fmt=[(3, [B.ints([2, 5]), B.ints([0, 0])]), (4, [B.ints([0, 10, 300], pad_to=4), B.ints([B.MISSING], pad_to=4, width=2)])])
    r = B.Rendered(rec + rec[:11], strings, contigs, n)
    assert r.lines == [b"2\t100\trs1\tA\tC,GT\t12.5\tPASS\tDP=7;AF=0.5,.\tGT:PL\t0|1:0,10,300\t./.:."]
    assert r.error == (1, B.E_TRUNCATED, len(rec)) and r.consumed == len(rec)
    assert B.Rendered(rec + rec[:11], strings, contigs, n, eof=False).error is None


@pytest.fixture(scope="module")
def header_driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bcf_header") / "bcf_header"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-o", str(exe),
                           os.path.join(ROOT, "tests", "bcf_header_driver.cpp"), os.path.join(CSRC, "exg_bcf_header.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(data, *args):
        p = exe.parent / "in.raw"
        p.write_bytes(data)
        res = subprocess.run([str(exe), str(p), *args], env=env, capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stdout + res.stderr)
        lines = res.stdout.splitlines()
        table = lambda what: [None if ln.split(" ", 2)[2] == "-" else ln.split(" ", 2)[2].encode() for ln in lines if ln.startswith(what + " ")]
        return lines, table("string"), table("contig")
    return run


def test_header_parser_and_dictionaries_under_asan_ubsan(header_driver):
    raw = gzip.decompress(open(os.path.join(GOLDEN, "bcf", "index.bcf"), "rb").read())
    text, _ = B.render_file(raw)
    lines, strings, contigs = header_driver(raw)
    want_s, want_c, n = B.dictionaries(text)
    assert lines[0].startswith(f"rc 0 need 0 end {9 + len(text) + 1} samples {n} gt -1") and strings == want_s and contigs == want_c and len(contigs) == 86
    infos, formats = [("DP", "1", "Integer"), ("XX", "1", "String")], [("GT", "1", "String"), ("DP", "1", "Integer")]
    for idx in (True, False):                                              # IDX= present / absent; DP in INFO and FORMAT has one index
        text = B.header_text(filters=("q10",), infos=infos, formats=formats, samples=("a", "b", "c"), idx=idx)
        lines, strings, contigs = header_driver(B.file_header(text) + b"records follow")
        assert strings == [b"PASS", b"q10", b"DP", b"XX", b"GT"] == B.dictionaries(text)[0] and contigs == [b"1", b"2"]
        assert lines[0].startswith(f"rc 0 need 0 end {9 + len(text) + 1} samples 3 gt 4")
    # PASS undeclared, IDX with a gap and out of order, a quoted Description with commas and an escaped quote, no contigs, no samples
    text = (b'##fileformat=VCFv4.2\n##INFO=<ID=B,Number=1,Type=String,Description="x, ID=Z,IDX=9 \\" y",IDX=5>\n##FILTER=<ID=lo,Description="l",IDX=2>\n'
            b'##INFO=<ID=A,Number=0,Type=Flag,Description="a">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n')
    lines, strings, contigs = header_driver(B.file_header(text))
    assert strings == [b"PASS", None, b"lo", None, None, b"B", b"A"] and contigs == [] and " samples 0 gt -1" in lines[0]
    # refusals
    for data, why in ((B.file_header(text.split(b"#CHROM")[0]), "no #CHROM line"), (B.file_header(text, terminate=False), "not NUL-terminated"),
                      (B.file_header(text, minor=1), "2.1 is not supported"), (b"BAM\1" + b"\0" * 20, "magic"), (b"BCF", "shorter"),
                      (B.file_header(text)[:-3], "truncated BCF header")):
        lines, _, _ = header_driver(data)
        assert lines[0].startswith("rc -1") and why in lines[0], lines[0]
    # every cut of the header
    lines, _, _ = header_driver(B.file_header(B.header_text(infos=infos, formats=formats, samples=("a",), idx=True)) + b"xyz", "cuts")
    assert lines == ["cuts ok"]


def test_float_renderer_round_trips_under_asan_ubsan(tmp_path):
    """the device's float spelling, compiled for the host: 2 M random bit patterns and the edges (zeros, subnormals, FLT_MIN,
    FLT_MAX, powers of two and ten, infinities, NaN) come back from the decimal -> float32 conversion with the same bits"""
    exe = tmp_path / "bcf_float"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-o", str(exe),
                           os.path.join(ROOT, "tests", "bcf_float_driver.cpp")])
    res = subprocess.run([str(exe), "2000000", "20261020"], capture_output=True, text=True)
    assert res.returncode == 0 and re.search(r"checked 2\d{6} failures 0$", res.stdout.strip()), res.stdout[-2000:] + res.stderr[-2000:]


def test_abi_mirrors(tmp_path):
    from exon_duckdb_amd import abi, load_library, table_function
    src = open(HEADER).read()
    codes = dict(re.findall(r"#define (EXG_PE_BCF_\w+) (\d+)", src))
    assert len(codes) == 9 and sorted(int(v) for v in codes.values()) == list(range(47, 56)) and max(int(v) for v in codes.values()) < 128
    for name, v in codes.items():
        assert getattr(abi, name) == int(v), name
    assert [B.E_RECORD_LENGTH, B.E_TRUNCATED, B.E_TYPE, B.E_RESERVED, B.E_OVERRUN, B.E_CHROM, B.E_DICT, B.E_NO_ALLELE, B.E_SAMPLE_COUNT] == \
        [abi.EXG_PE_BCF_RECORD_LENGTH, abi.EXG_PE_BCF_TRUNCATED, abi.EXG_PE_BCF_TYPE, abi.EXG_PE_BCF_RESERVED_VALUE, abi.EXG_PE_BCF_OVERRUN,
         abi.EXG_PE_BCF_CHROM, abi.EXG_PE_BCF_DICT_INDEX, abi.EXG_PE_BCF_NO_ALLELE, abi.EXG_PE_BCF_SAMPLE_COUNT]
    assert re.search(r"#define EXG_FMT_BCF 7\b", src) and abi.EXG_FMT_BCF == 7
    assert re.search(r"#define EXG_ABI_VERSION 9\b", src) and abi.EXG_ABI_VERSION == 9
    lib = load_library()
    assert lib.exg_abi_version() == 9
    lib.exg_parse_error_string.restype = C.c_char_p
    texts = {lib.exg_parse_error_string(c) for c in range(47, 56)}
    assert len(texts) == 9 and b"unknown parse error" not in texts and lib.exg_parse_error_string(56) == lib.exg_parse_error_string(46) == b"unknown parse error"
    for sym in ("exg_bcf_workspace_bytes", "exg_bcf_to_vcf", "exg_bcf_result"):
        assert sym in abi.SIGNATURES and re.search(r"\b%s\(" % sym, src) and getattr(lib, sym)      # exports.map lets exg_* out
    assert "exg_*;" in open(os.path.join(CSRC, "exports.map")).read()
    lib.exg_bcf_workspace_bytes.restype, lib.exg_bcf_workspace_bytes.argtypes = C.c_uint64, [C.c_uint64, C.c_uint32]
    small, large = lib.exg_bcf_workspace_bytes(0, 0), lib.exg_bcf_workspace_bytes(1 << 30, 2504)
    assert 0 < small < 1 << 16 and (1 << 30) // 32 * 24 <= large < 1 << 30                      # three 8-byte arrays a possible record
    # the structs' layouts
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in (("exg_bcf_to_vcf_args", abi.BcfToVcfArgs), ("exg_bcf_to_vcf_result", abi.BcfToVcfResult)):
        prog.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        prog += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    prog.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(prog))
    subprocess.check_call(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")])
    got = dict(ln.split() for ln in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines())
    for cname, cls in (("exg_bcf_to_vcf_args", abi.BcfToVcfArgs), ("exg_bcf_to_vcf_result", abi.BcfToVcfResult)):
        assert int(got[cname]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    assert C.sizeof(abi.BcfToVcfResult) == 64
    # the surface
    con = table_function.connect()
    assert con.has_table_function("read_bcf_file_records")
    assert con.replacement_scan("a/b.bcf") == "read_bcf_file_records" and con.replacement_scan("a/B.BCF") == "read_bcf_file_records"
    assert con.replacement_scan("b.bcf.txt") is None
    lib.replacement_scan.restype = type("R", (C.Structure,), {"_fields_": [("file_type", C.c_char_p)]})
    lib.replacement_scan.argtypes = [C.c_char_p]
    assert lib.replacement_scan(b"a/b.bcf").file_type == b"BCF" and lib.replacement_scan(b"b.bcf.txt").file_type is None


def test_files_that_are_not_bgzf_are_refused_by_name_without_a_device(tmp_path):
    """a text file, an uncompressed BCF (bcftools -Ou) and a plain gzip member handed over as "bcf": EXG_E_UNSUPPORTED with the file's
    name, before a device is asked for; shard_count = 2 likewise; a BGZF file gets past both (what stops it here is the missing device)"""
    from exon_duckdb_amd import ExgError, abi
    from exon_duckdb_amd.reader import ShardReader
    text = B.header_text()
    raw = B.file_header(text) + B.record()
    for name, data in (("x.txt", b"hello\n" * 10), ("u.bcf", raw), ("g.bcf", gzip.compress(raw, 6, mtime=0))):
        (tmp_path / name).write_bytes(data)
        with pytest.raises(ExgError) as e:
            ShardReader(str(tmp_path / name), "bcf")
        assert e.value.code == abi.EXG_E_UNSUPPORTED and name in str(e.value) and "BGZF" in str(e.value), str(e.value)
    (tmp_path / "ok.bcf").write_bytes(BAM.bgzf(raw))
    with pytest.raises(ExgError) as e:
        ShardReader(str(tmp_path / "ok.bcf"), "bcf", shard_index=0, shard_count=2)
    assert e.value.code == abi.EXG_E_UNSUPPORTED and "one file is one shard" in str(e.value)
    try:
        ShardReader(str(tmp_path / "ok.bcf"), "Bcf").close()
    except ExgError as e:
        assert e.code == abi.EXG_E_NO_DEVICE, (e.code, str(e))
