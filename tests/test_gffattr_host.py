"""gff_parse_attributes without a GPU: the host scalar the DuckDB shim registers (exon_scan::GffParseAttributes through
table_function.gff_parse_attributes) against the oracle tests/gff_attr_ref.py — the four statements test_gff_scan.test:79-99 pins,
one named test per rule of INTEGRATION.md (GFF attributes), the exception's text byte for byte, a fuzz —, and the library's
surface that needs no device: the error code and its text, the ctypes mirrors against the header's layout, the exported symbols,
the refusals of exg_gff_attributes that come before any launch, the shim's registration, the sanitized stand-alone driver."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

import gff_attr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "exon_gpu.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gff")
EXPECTED = json.load(open(os.path.join(GOLDEN, "expected_gff_attributes.json")))
HIPCC = "/opt/rocm/bin/hipcc"


def scalar(field):
    from exon_duckdb_amd import table_function
    return table_function.gff_parse_attributes(field)


def error_of(field):
    """(offset, length, text) of the scalar's exception"""
    from exon_duckdb_amd import ExgError, abi
    with pytest.raises(ExgError) as e:
        scalar(field)
    assert e.value.parse_code == abi.EXG_PE_GFF_ATTRIBUTES and e.value.code == abi.EXG_E_PARSE
    return e.value.offset, e.value.length, str(e.value)


def both(field):
    """the scalar and the oracle on one field: the same entries, or the same offset, length and text -> the oracle's outcome"""
    want = R.outcome(field)
    if want[0] == "ok":
        assert scalar(field) == want[1], field
    else:
        off, length, text = error_of(field)
        assert (off, length) == want[1:], (field, off, length, want)
        assert R.error_text(field[off:off + length]) in text, (field, text)
    return want


# ---- the reference's pins ---------------------------------------------------------------------------------------------------
def test_the_four_pinned_statements():
    assert len(EXPECTED["pinned"]) == 4
    for p in EXPECTED["pinned"]:
        arg = p["argument"].encode()
        if "error" in p:
            assert error_of(arg)[2].endswith(p["error"]) and R.outcome(arg)[0] == "error"
        else:
            got = scalar(arg)
            assert [[k.decode(), v.decode()] for k, v in got] == p["entries"] and R.parse(arg) == got
        if "element_at_key_1" in p:
            assert [v for k, v in got if k == b"key"][0].decode() == p["element_at_key_1"]


def test_fixture_files_give_the_recorded_entries():
    counts = {}
    for name, rows in EXPECTED["files"].items():
        lines = [ln for ln in open(os.path.join(GOLDEN, name), "rb").read().split(b"\n") if ln and not ln.startswith(b"#")]
        assert len(lines) == len(rows)
        for line, row in zip(lines, rows):
            field = line.split(b"\t", 8)[8]
            assert field.decode() == row["field"]
            assert [[k.decode(), v.decode()] for k, v in scalar(field)] == row["entries"] == [[k.decode(), v.decode()] for k, v in R.parse(field)]
        counts[name] = (len(rows), sum(len(r["entries"]) for r in rows))
    assert counts == {"test.gff": (2, 4), "raw-test.gff": (10, 20)}
    assert max(len(r["field"]) for r in EXPECTED["files"]["raw-test.gff"]) == 68
    assert sum("; Parent=" in r["field"] for r in EXPECTED["files"]["raw-test.gff"]) == 2


# ---- one test per rule -------------------------------------------------------------------------------------------------------
def test_rule_r1_the_field_is_cut_at_every_semicolon_and_empty_segments_are_dropped():
    assert both(b"a=b;c=d") == ("ok", [(b"a", b"b"), (b"c", b"d")])
    assert both(b"a=b;") == both(b"a=b") == both(b";;a=b;;;") == ("ok", [(b"a", b"b")])


def test_rule_r1_a_field_without_a_segment_is_its_own_segment_and_fails():
    assert both(b"") == ("error", 0, 0) and both(b";") == ("error", 0, 1) and both(b";;;") == ("error", 0, 3)
    assert error_of(b";")[2].endswith("Invalid attribute: ';' expected 'key=value;key2=value2'")
    assert error_of(b"")[2].endswith("Invalid attribute: '' expected 'key=value;key2=value2'")


def test_rule_r2_a_segment_loses_the_six_ascii_blanks_at_both_ends_and_no_other_byte():
    assert both(b" \t\n\v\f\ra=b\r\f\v\n\t ;  c=d") == ("ok", [(b"a", b"b"), (b"c", b"d")])
    assert both(b"\xa0a=b\x85") == ("ok", [(b"\xa0a", b"b\x85")])                 # bytes >= 0x80 are never blank
    assert both(b"\x00a=b\x1f") == ("ok", [(b"\x00a", b"b\x1f")])
    assert both(b"a=b\xe9 ;") == ("ok", [(b"a", b"b\xe9")])


def test_rule_r2_keys_and_values_are_not_trimmed_on_their_own():
    assert both(b"a = b") == ("ok", [(b"a ", b" b")]) and both(b" a = b ") == ("ok", [(b"a ", b" b")])


def test_rule_r3_the_segment_is_cut_at_every_equals_sign_and_empty_pieces_are_dropped():
    assert both(b"a==b") == both(b"=a=b") == both(b"a=b=") == both(b"==a===b==") == ("ok", [(b"a", b"b")])
    assert both(b"a= =") == ("ok", [(b"a", b" ")]) and both(b"a=b= ") == ("ok", [(b"a", b"b")])


def test_rule_r3_anything_but_two_pieces_is_an_error():
    for field, want in ((b"a", (0, 1)), (b"a=", (0, 2)), (b"=a", (0, 2)), (b"a=b=c", (0, 5)), (b"a= =b", (0, 5)), (b"   ", (0, 0)), (b"ID", (0, 2)),
                        (b"===", (0, 3)), (b"a= ", (0, 2))):
        assert both(field) == ("error",) + want, field


def test_rule_r4_entries_come_in_field_order_and_a_repeated_key_is_a_second_entry():
    assert both(b"b=2;a=1;b=3") == ("ok", [(b"b", b"2"), (b"a", b"1"), (b"b", b"3")])


def test_rule_r5_nothing_is_decoded():
    assert both(b"ID=gene%3B1;Note=a%2Cb,c") == ("ok", [(b"ID", b"gene%3B1"), (b"Note", b"a%2Cb,c")])


def test_rule_r6_the_leftmost_failing_segment_is_reported_behind_its_trim():
    assert both(b"a=b;  x  ;c") == ("error", 6, 1) and both(b"a=b;  ;c=d") == ("error", 4, 0) and both(b"a=b; x=y=z ;k") == ("error", 5, 5)
    assert error_of(b"a=b;  x y  ;c")[2].endswith("Invalid attribute: 'x y' expected 'key=value;key2=value2'")


def test_rule_r7_null_gives_null():
    assert scalar(None) is None


def test_error_texts_byte_for_byte():
    for field, text in ((b"ID", "Invalid attribute: 'ID' expected 'key=value;key2=value2'"),
                        (b" a=b=c\t", "Invalid attribute: 'a=b=c' expected 'key=value;key2=value2'"),
                        (b"k=v; ;", "Invalid attribute: '' expected 'key=value;key2=value2'"),
                        (b"k=v;\xe9", "Invalid attribute: '\xe9' expected 'key=value;key2=value2'"),
                        (b"k=v;a\x00b", "Invalid attribute: 'a\x00b' expected 'key=value;key2=value2'")):
        assert error_of(field)[2].endswith(text), field
        assert R.error_text(field[R.outcome(field)[1]:][:R.outcome(field)[2]]) == text


def test_fuzz_2000_fields_against_the_oracle():
    fields = R.fuzz_fields(20231, 2000)
    assert max(map(len, fields)) <= 200 and min(map(len, fields)) == 0
    assert {b for f in fields for b in f} == {ord(c) for c in "ab=; \t\r"} | {0xE9}
    ok = sum(both(f)[0] == "ok" for f in fields)
    print(f"{ok} of {len(fields)} fuzz fields parse")
    assert ok >= len(fields) * R.VALID_SHARE and len(fields) - ok >= len(fields) // 5            # at least a third parse; errors are there too


# ---- the library's surface, no GPU ------------------------------------------------------------------------------------------
def test_error_code_65_in_header_and_abi_with_its_text_and_64_left_out():
    from exon_duckdb_amd import abi, load_library
    header = open(HEADER).read()
    assert re.search(r"#define EXG_PE_GFF_ATTRIBUTES 65\b", header) and abi.EXG_PE_GFF_ATTRIBUTES == 65
    assert not re.search(r"#define EXG_PE_\w+ 64\b", header) and re.search(r"#define EXG_ABI_VERSION 9\b", header)
    lib = load_library()
    lib.exg_parse_error_string.restype = C.c_char_p
    lib.exg_parse_error_string.argtypes = [C.c_uint32]
    assert lib.exg_parse_error_string(65) == b"invalid GFF attribute"
    assert lib.exg_parse_error_string(64) == lib.exg_parse_error_string(66) == b"unknown parse error"
    assert 0 < lib.exg_gff_attributes_workspace_bytes(0) < lib.exg_gff_attributes_workspace_bytes(1 << 20) < 14 << 20


def test_gff_mirrors_match_the_c_layout(tmp_path):
    from exon_duckdb_amd import abi
    structs = {"exg_gff_attributes_args": abi.GffAttributesArgs, "struct exg_gff_attributes_result": abi.GffAttributesResult}
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs.items():
        prog.append(f'printf("{cname.split()[-1]} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            prog.append(f'printf("{cname.split()[-1]}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    prog.append('printf("same %d\\n", (int)(sizeof(exg_gff_attributes_args) == sizeof(exg_gtf_attributes_args))); return 0; }')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    got = dict(line.split() for line in lines)
    for cname, cls in structs.items():
        cname = cname.split()[-1]
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)
    assert C.sizeof(abi.GffAttributesResult) == 64 and got["same"] == "1"
    assert [f for f, _ in abi.GffAttributesArgs._fields_] == [f for f, _ in abi.GtfAttributesArgs._fields_]     # a reader can feed either op
    assert abi.GffAttributesResult.error_length.offset == 40


def test_exported_symbols_are_declared_in_the_header():
    from exon_duckdb_amd import LIB_PATH, load_library
    load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    header = open(HEADER).read()
    ours = {"exg_gff_attributes_workspace_bytes", "exg_gff_attributes", "exg_gff_attributes_result"}
    assert ours <= exported and {s for s in exported if "gff" in s} == ours
    for s in ours:
        assert re.search(r"\b" + s + r"\(", header), s


def test_bad_arguments_are_refused_before_any_launch():
    """null or unaligned column, a workspace one byte short, chunk_rows without d_out_chunk_base, n_rows = 2^32 - 1: each is
    EXG_E_INVALID_ARG from the argument checks, which come before the first HIP call (no device is needed to see them)"""
    from exon_duckdb_amd import abi, load_library
    lib = load_library()
    lib.exg_last_error_message.restype = C.c_char_p
    block = (C.c_uint64 * 64)()
    p = (C.addressof(block) + 15) & ~15

    def complete(n=4):
        a = abi.GffAttributesArgs()
        a.d_strings, a.d_payload, a.n_rows = p, p, n
        a.d_workspace, a.workspace_bytes, a.d_result = p, lib.exg_gff_attributes_workspace_bytes(n), p
        return a

    def refused(a, word):
        assert lib.exg_gff_attributes(C.byref(a)) == abi.EXG_E_INVALID_ARG
        assert word in lib.exg_last_error_message(), lib.exg_last_error_message()

    a = complete()
    a.d_strings = None
    refused(a, b"column")
    a = complete()
    a.d_strings = p + 8
    refused(a, b"unaligned")
    a = complete()
    a.workspace_bytes -= 1
    refused(a, b"workspace too small")
    a = complete()
    a.chunk_rows = 2048
    refused(a, b"output")
    a = complete((1 << 32) - 1)
    refused(a, b"rows")
    a = complete()
    a.entries_capacity = 1
    refused(a, b"output")
    assert lib.exg_gff_attributes(None) == abi.EXG_E_INVALID_ARG
    assert lib.exg_gff_attributes_result(None, None, None) == abi.EXG_E_INVALID_ARG and b"exg_gff_attributes_result" in lib.exg_last_error_message()


def test_the_shim_registers_the_scalar_and_still_compiles_against_the_stub():
    shim = open(os.path.join(ROOT, "duckdb_shim", "exon_extension.cpp")).read()
    assert 'ScalarFunction("gff_parse_attributes", {LogicalType::VARCHAR}' in shim and "GffParseAttributesFunction" in shim
    assert "MakeMap<LogicalType>(LogicalType::VARCHAR, LogicalType::VARCHAR, 0)" in shim and "not registered" not in shim
    stub = os.path.join(ROOT, "tests", "duckdb_stub")
    assert "MAP" not in open(os.path.join(stub, "duckdb.hpp")).read()
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", stub, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "exon_duckdb_amd", "csrc"), os.path.join(ROOT, "duckdb_shim", "exon_extension.cpp")])


def test_falsifiability_kit_carries_the_recalled_and_decided_rules(tmp_path):
    """tools/falsify_kit.py: a statement per [RECALLED] / [DECIDED] rule for a real exon build, the oracle's answer beside it;
    compare_scalars.py says SAME when those answers come back and DIFFERENT when one does not"""
    import sys
    kit = tmp_path / "kit"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "falsify_kit.py"), str(kit)])
    cases = json.load(open(kit / "scalar_cases.json"))
    args = {c["case"]: re.search(r"gff_parse_attributes\('(.*)'\) AS m", c["sql"]).group(1) for c in cases}
    assert {"", ";", "a==b", " a = b ", "a=1;a=2", "a=b\u00a0"} <= set(args.values())
    run = open(kit / "run.sh").read()
    assert all(c["sql"] in run for c in cases) and not any(ch in a for a in args.values() for ch in "'\"$`\\")
    os.makedirs(kit / "got")
    for c in cases:
        e = json.load(open(kit / "expected" / (c["case"] + ".json")))
        want = R.outcome(args[c["case"]].encode())
        assert (e["error"] is None) == (want[0] == "ok")
        if e["error"]:
            assert e["error"] == R.error_text(args[c["case"]].encode()[want[1]:want[1] + want[2]])
            (kit / "got" / (c["case"] + ".err")).write_text("Error: ...")
        else:
            assert list(zip(e["rows"][0]["keys"], e["rows"][0]["values"])) == [(k.decode(), v.decode()) for k, v in want[1]]
            (kit / "got" / (c["case"] + ".json")).write_text("".join(json.dumps(r) + "\n" for r in e["rows"]))
    res = subprocess.run([sys.executable, "compare_scalars.py"], cwd=kit, capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.count("SAME") == len(cases) == 11, res.stdout[-2000:]
    (kit / "got" / "gff_parse_attributes_inner_blanks_stay.json").write_text(json.dumps({"keys": ["a"], "values": ["b"]}) + "\n")
    res = subprocess.run([sys.executable, "compare_scalars.py"], cwd=kit, capture_output=True, text=True)
    assert res.returncode == 1 and "DIFFERENT gff_parse_attributes_rules [gff_parse_attributes_inner_blanks_stay]" in res.stdout


def test_host_functions_under_asan_ubsan(tmp_path):
    """tests/gffattr_host_driver.cpp: a stand-alone program over exg_gffattr.hpp and exon_scan::GffParseAttributes (exactly-sized
    heap fields, the pins and every rule's examples, every prefix of a 200-byte field, segments astride the 64-byte seam, random
    fields, the fixture files — the device's word walk against the left-to-right parser on each), built with AddressSanitizer +
    UBSan; nothing is preloaded"""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "gffattr_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "exon_duckdb_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "gffattr_host_driver.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe), os.path.join(GOLDEN, "test.gff"), os.path.join(GOLDEN, "raw-test.gff")], env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "gffattr host functions ok: 12 fields, 24 entries from files" in res.stdout


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc is not installed")
def test_kernel_resources(tmp_path):
    """the code object's own report: no scratch in any kernel of the unit — the open segment's nine scalars and the
    per-lane copy the `;` lanes judge stay in registers — and at most 64 VGPRs, the full eight waves a SIMD, which is what hides
    the byte loads of a wave that walks one row"""
    from exon_duckdb_amd import build as B
    src = os.path.join(B.CSRC, "exg_gffattr.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + B._flags() + B.FILE_FLAGS.get("exg_gffattr.hip", []) + [
        "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "exg_gffattr.s")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    kernels = {}
    name = None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: +Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        m = re.search(r"remark: +(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            kernels[name][m.group(1).split()[0]] = int(m.group(2))
    ours = {k: v for k, v in kernels.items() if "gffattr" in k and ("k_rows" in k or "k_finish" in k)}
    assert len(ours) == 3, sorted(kernels)
    for k, v in ours.items():
        print(k, v)
        assert v["ScratchSize"] == 0 and v["VGPRs"] <= 64 and v["Occupancy"] == 8, (k, v)
