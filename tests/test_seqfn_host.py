"""CPU checks of the sequence scalars and the SAM flag predicates: the reference's own expectations
(tests/golden/scalar/expected_scalar_functions.json, from test_scalar_functions.test:5-89 and test_sam_flags.test) against the
independent restatement tests/seqfn_ref.py AND against the host arithmetic the DuckDB shim registers (reached through
libexon_tf_test.so), error texts character for character, every byte value through every mapping, the C layout of the two new
structs of include/exon_gpu.h, and the stand-alone AddressSanitizer / UBSan driver of the host functions."""
import ctypes as C
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import seqfn_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "exon_gpu.h")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "scalar", "expected_scalar_functions.json")))
OPS = {name: op for op, name in ref.OP_NAMES.items()}


def host(name):
    from exon_duckdb_amd import table_function
    return getattr(table_function, name)


def host_error(name, s):
    from exon_duckdb_amd import ExgError, abi
    with pytest.raises(ExgError) as e:
        host(name)(s)
    assert e.value.code == abi.EXG_E_PARSE
    text = str(e.value)
    return text[text.index(": ") + 2:].encode("latin-1")


def ref_error(name, s):
    with pytest.raises(ref.SeqError) as e:
        ref.apply(OPS[name], s)
    return e.value


def test_the_golden_file_holds_the_reference_cases():
    cases = GOLDEN["scalar_functions"]
    assert len(cases) == 20 and len(GOLDEN["sam_flags"]) == 13
    assert [c["input"] for c in cases if c.get("error")] == ["ATCGQ", "ATNN", "NNN", "AUNN"]
    by = {(c["function"], c["input"]): c.get("expected") for c in cases}
    assert by[("reverse_complement", "GGGG")] == "TTTT" and by[("reverse_complement", "ATCG")] == "CGAT"
    codons = next(c for c in cases if c["line"] == 72)
    assert len(codons["input"]) == 192 and len({codons["input"][i:i + 3] for i in range(0, 192, 3)}) == 64
    assert codons["expected"].startswith("KNNKIIIM") and codons["expected"].endswith("GGGG") and len(codons["expected"]) == 64


@pytest.mark.parametrize("case", GOLDEN["scalar_functions"], ids=lambda c: f"{c['function']}-{c['input']}"[:40])
def test_golden_scalar_functions(case):
    name = case["function"]
    s = None if case["input"] is None else case["input"].encode()
    if case.get("error"):
        e = ref_error(name, s)
        assert host_error(name, s) == e.text
        return
    for got in (ref.apply(OPS[name], s), host(name)(s)):
        if "expected_prefix" in case:
            assert f"{float(got):.6f}".startswith(case["expected_prefix"])
        elif case["expected"] is None:
            assert got is None
        elif name == "gc_content":
            assert np.float32(got) == np.float32(case["expected"])
        else:
            assert got == case["expected"].encode()


@pytest.mark.parametrize("case", GOLDEN["sam_flags"], ids=lambda c: f"{c['function']}-{c['flag']}")
def test_golden_sam_flags(case):
    assert ref.sam_flag(case["function"], case["flag"]) is case["expected"]
    assert host(case["function"])(case["flag"]) is case["expected"]


def test_error_texts_are_the_references():
    assert host_error("complement", b"ATCGQ") == b"Invalid character in sequence: Q"
    assert host_error("reverse_complement", b"NATC") == b"Invalid character in sequence: N"
    assert host_error("transcribe", b"ATNN") == b"Invalid character in sequence: N"
    assert host_error("transcribe", b"AUCG") == b"Invalid character in sequence: U"
    assert host_error("reverse_transcribe", b"AUNN") == b"Invalid character in sequence: N"
    assert host_error("reverse_transcribe", b"ATCG") == b"Invalid character in sequence: T"
    assert host_error("translate_dna_to_aa", b"ATTT") == b"Invalid sequence length: 4"
    assert host_error("translate_dna_to_aa", b"NNNN") == b"Invalid sequence length: 4"      # the length before any codon
    assert host_error("translate_dna_to_aa", b"NNN") == b"Invalid codon: NNN"
    assert host_error("translate_dna_to_aa", b"ATGATNCCC") == b"Invalid codon: ATN"       # the first from the left
    assert host_error("complement", b"ACGTacgt") == b"Invalid character in sequence: a"   # lower case is invalid
    assert host_error("complement", b"AC\xe9") == b"Invalid character in sequence: \xe9"
    for name, s in (("complement", b"ATCGQ"), ("translate_dna_to_aa", b"NNNN"), ("translate_dna_to_aa", b"ACGTTN"),
                    ("reverse_transcribe", b"T")):
        assert host_error(name, s) == ref_error(name, s).text


def test_null_in_null_out():
    for name in ref.OP_NAMES.values():
        assert host(name)(None) is None and ref.apply(OPS[name], None) is None
    for name in ref.SAM_FLAGS:
        assert host(name)(None) is None


def test_every_byte_value_through_every_function():
    for name, op in OPS.items():
        for c in range(256):
            for s in (bytes([c]), b"ACG" + bytes([c]) * 3, bytes([c]) * 3):
                try:
                    exp = ref.apply(op, s)
                except ref.SeqError as e:
                    assert host_error(name, s) == e.text, (name, s)
                    continue
                got = host(name)(s)
                assert (np.float32(got).tobytes() == exp.tobytes()) if op == ref.GC_CONTENT else got == exp, (name, s)
    assert host("gc_content")(b"gcGC\xc7\xc3") == np.float32(2) / np.float32(6)     # lower case and bytes >= 0x80 do not count


def test_empty_strings_and_the_inline_boundary():
    rng = random.Random(5)
    for name, op in OPS.items():
        alphabet = b"ACGU" if op == ref.REVERSE_TRANSCRIBE else b"ACGT"
        for n in (0, 1, 2, 3, 11, 12, 13, 36, 39, 150, 4096, 4097, 4098):
            s = bytes(rng.choice(alphabet) for _ in range(n))
            try:
                exp = ref.apply(op, s)
            except ref.SeqError as e:
                assert op == ref.TRANSLATE and n % 3 and host_error(name, s) == e.text
                continue
            got = host(name)(s)
            assert (np.float32(got).tobytes() == exp.tobytes()) if op == ref.GC_CONTENT else got == exp, (name, n)
            assert ref.apply_fast(op, s).tobytes() == exp.tobytes() if op == ref.GC_CONTENT else ref.apply_fast(op, s) == exp


def test_gc_content_is_one_float32_division():
    for n in (3, 7, 150):
        for k in range(n + 1):
            s = b"G" * (k // 2) + b"C" * (k - k // 2) + b"A" * (n - k)
            assert np.float32(host("gc_content")(s)).tobytes() == (np.float32(k) / np.float32(n)).tobytes()


def test_sam_flags_outside_u16():
    assert host("is_segmented")(65537) is True and ref.sam_flag("is_segmented", 65537)      # (uint16_t)65537 == 1
    assert host("is_segmented")(65536) is False
    assert host("is_supplementary")(-1) is True and host("is_supplementary")(-2049) is False
    assert host("is_unmapped")(-2147483648) is False and host("is_unmapped")(2147483647) is True
    rng = random.Random(7)
    for _ in range(200):
        f = rng.randrange(-2 ** 31, 2 ** 31)
        for name in ref.SAM_FLAGS:
            assert host(name)(f) is ref.sam_flag(name, f), (name, f)
    from exon_duckdb_amd import table_function
    assert table_function.SAM_FLAG_FUNCTIONS == tuple(ref.SAM_FLAGS)


def test_new_structs_have_the_c_layout(tmp_path):
    from exon_duckdb_amd import abi
    structs = {"exg_seq_result": abi.SeqResult, "exg_sequence_op_args": abi.SequenceOpArgs}
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs.items():
        prog.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            prog.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    for name in ("EXG_SEQ_COMPLEMENT", "EXG_SEQ_REVERSE_COMPLEMENT", "EXG_SEQ_TRANSCRIBE", "EXG_SEQ_REVERSE_TRANSCRIBE",
                 "EXG_SEQ_TRANSLATE", "EXG_SEQ_GC_CONTENT", "EXG_PE_SEQ_INVALID_CHARACTER", "EXG_PE_SEQ_LENGTH", "EXG_PE_SEQ_CODON"):
        prog.append(f'printf("{name} %d\\n", {name});')
    prog.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert got["exg_seq_result"] == "64"
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    for name, val in got.items():
        if name.startswith("EXG_SEQ_") or name.startswith("EXG_PE_SEQ_"):
            assert getattr(abi, name) == int(val), name
    assert (ref.PE_INVALID_CHARACTER, ref.PE_LENGTH, ref.PE_CODON) == (abi.EXG_PE_SEQ_INVALID_CHARACTER, abi.EXG_PE_SEQ_LENGTH, abi.EXG_PE_SEQ_CODON)
    assert tuple(ref.ALL_OPS) == (abi.EXG_SEQ_COMPLEMENT, abi.EXG_SEQ_REVERSE_COMPLEMENT, abi.EXG_SEQ_TRANSCRIBE,
                                  abi.EXG_SEQ_REVERSE_TRANSCRIBE, abi.EXG_SEQ_TRANSLATE, abi.EXG_SEQ_GC_CONTENT)


def test_library_surface_of_the_sequence_op():
    from exon_duckdb_amd import abi, load_library
    lib = load_library()
    for code, text in ((abi.EXG_PE_SEQ_INVALID_CHARACTER, b"invalid character in sequence"), (abi.EXG_PE_SEQ_LENGTH, b"invalid sequence length"),
                       (abi.EXG_PE_SEQ_CODON, b"invalid codon")):
        assert lib.exg_parse_error_string(code) == text
    for op in ref.ALL_OPS:
        last = 0
        for n in (0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 100000, 100001, 1 << 24, (1 << 32) - 2):
            b = lib.exg_sequence_workspace_bytes(op, n)
            assert b >= last and b >= 12 * n, (op, n)      # monotone in n_rows
            last = b
    # argument checks that need no device: they are made before anything is enqueued
    a = abi.SequenceOpArgs()
    assert lib.exg_sequence_op(None) == abi.EXG_E_INVALID_ARG
    assert lib.exg_sequence_op(C.byref(a)) == abi.EXG_E_INVALID_ARG and b"exg_sequence_op" in lib.exg_last_error_message()
    assert lib.exg_sequence_result(None, None, None) == abi.EXG_E_INVALID_ARG


def test_host_functions_under_asan_ubsan(tmp_path):
    """tests/seqfn_asan_driver.cpp: a stand-alone program over exg_seqfn.hpp and the host scalars of exon_table_function.hpp
    (empty, 1-byte, 12- and 13-byte and 1 MiB inputs, every error), built with AddressSanitizer + UBSan"""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "seqfn_asan"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "exon_duckdb_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "seqfn_asan_driver.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "seqfn host functions ok" in res.stdout
