"""CPU checks of the CIGAR scalars: the reference's pins and the decided corners through the host scalars that the DuckDB shim
registers (reached through libexon_tf_test.so), every error kind with its offset against tests/cigar_ref.py — a regular expression
and a left-to-right loop that share nothing with the library —, the C layout of the two new structs of include/exon_gpu.h, the
argument checks of the C-ABI that need no device, the stand-alone AddressSanitizer / UBSan driver of the host functions, and the
resource report of the kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cigar_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "exon_gpu.h")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def tf():
    from exon_duckdb_amd import table_function
    return table_function


def ops(*pairs):
    return [{"op": o, "len": n} for o, n in pairs]


def parse_error(s):
    from exon_duckdb_amd import ExgError, abi
    with pytest.raises(ExgError) as e:
        tf().parse_cigar(s)
    assert e.value.code == abi.EXG_E_PARSE and e.value.parse_code == abi.EXG_PE_CIGAR_INVALID
    text = str(e.value)
    assert text[text.index(": ") + 2:] == "Invalid CIGAR string: " + s.split(b"\0")[0].decode("latin-1")      # (a C string: a NUL ends it)
    return e.value.offset


def extract_error(seq, cigar):
    from exon_duckdb_amd import ExgError, abi
    with pytest.raises(ExgError) as e:
        tf().extract_from_cigar(seq, cigar)
    assert e.value.code == abi.EXG_E_PARSE
    text = str(e.value)
    return e.value.parse_code, e.value.offset, text[text.index(": ") + 2:]


def test_pins():
    """test_scalar_functions.test:91-116"""
    f, g = tf().parse_cigar, tf().extract_from_cigar
    assert f(b"1M2M123S") == ops(("M", 1), ("M", 2), ("S", 123))
    assert parse_error(b"MMM") == 0                                   # `Invalid CIGAR string: MMM`
    assert f(b"100M") == ops(("M", 100))
    assert g(b"AACCAA", b"2I2M2I") == {"sequence_start": 2, "sequence_end": 4, "sequence": b"CC"}
    assert g(b"AACCAAC", b"2I2M2I1M") == {"sequence_start": 2, "sequence_end": 7, "sequence": b"CCAAC"}


def test_decided_corners():
    from exon_duckdb_amd import abi
    f, g = tf().parse_cigar, tf().extract_from_cigar
    assert f(b"") == [] and f(b"*") == [] and f(None) is None
    assert g(b"ACGT", b"") == g(b"ACGT", b"*") == {"sequence_start": 0, "sequence_end": 4, "sequence": b"ACGT"}
    assert g(b"", b"*") == {"sequence_start": 0, "sequence_end": 0, "sequence": b""}
    assert g(None, b"1M") is None and g(b"A", None) is None and g(None, None) is None
    assert g(b"ACGT", b"4M") == {"sequence_start": 0, "sequence_end": 4, "sequence": b"ACGT"}          # neither
    assert g(b"ACGT", b"1I3M") == {"sequence_start": 1, "sequence_end": 4, "sequence": b"CGT"}         # first only
    assert g(b"ACGT", b"3M1I") == {"sequence_start": 0, "sequence_end": 3, "sequence": b"ACG"}         # last only
    assert g(b"ACGT", b"2I") == {"sequence_start": 2, "sequence_end": 2, "sequence": b""}              # one operation: first and last
    assert g(b"ACGT", b"2I1M2I") == {"sequence_start": 2, "sequence_end": 2, "sequence": b""}
    assert extract_error(b"ACGT", b"3I") == (abi.EXG_PE_CIGAR_RANGE, 0, "CIGAR insertions exceed the sequence")
    assert extract_error(b"ACGT", b"3I1M2I") == (abi.EXG_PE_CIGAR_RANGE, 0, "CIGAR insertions exceed the sequence")
    assert extract_error(b"", b"1I") == (abi.EXG_PE_CIGAR_RANGE, 0, "CIGAR insertions exceed the sequence")
    # the whole CIGAR is validated, and a syntax error comes before the range error
    assert extract_error(b"ACGT", b"1I2M1I?") == (abi.EXG_PE_CIGAR_INVALID, 6, "Invalid CIGAR string")
    assert extract_error(b"ACGT", b"9I1M9I5") == (abi.EXG_PE_CIGAR_INVALID, 7, "Invalid CIGAR string")
    assert extract_error(b"ACGT", b"1I2Q1I") == (abi.EXG_PE_CIGAR_INVALID, 3, "Invalid CIGAR string")


ERRORS = [
    (b"5M?3I", 2), (b"?", 0), (b"5M*", 2), (b"**", 0), (b"5m", 1), (b"5M 3I", 2), (b"5M\x003I", 2), (b"5M\xff", 2),   # a bad byte
    (b"MMM", 0), (b"5MM", 2), (b"M5", 0), (b"5M=", 2),                                                             # a letter without digits
    (b"12", 2), (b"5M12", 4), (b"7", 1), (b"0" * 40, 40),                                                          # digits up to the end
    (b"268435456M", 8), (b"2684354550M", 9), (b"5M999999999I", 10), (b"0000268435456M", 12), (b"4294967296M", 8),  # above the bound
    (b"99999999999999999999999M", 8), (b"268435456", 8), (b"268435456?", 8),
    (b"5?7?", 1), (b"5M300000000I?", 10),                                                                          # the leftmost wins
]


@pytest.mark.parametrize("row", ERRORS, ids=lambda r: repr(r[0][:24]))
def test_every_error_kind_with_its_offset(row):
    s, offset = row
    assert ref.error_offset(s) == offset                              # the table and the oracle say the same
    assert parse_error(s) == offset
    from exon_duckdb_amd import abi
    assert extract_error(b"ACGT", s)[:2] == (abi.EXG_PE_CIGAR_INVALID, offset)


def test_lengths():
    f = tf().parse_cigar
    assert f(b"268435455M") == ops(("M", 268435455)) and parse_error(b"268435456M") == 8
    assert f(b"0000000000001M") == ops(("M", 1)) and f(b"0M") == ops(("M", 0))
    assert f(b"0" * 5000 + b"17S") == ops(("S", 17))
    assert f(b"1M2I3D4N5S6H7P8=9X") == ops(*zip("MIDNSHP=X", range(1, 10)))


def test_host_scalar_against_the_oracle():
    """a few thousand random rows, valid and broken in one byte: the same operations, or the same offset"""
    from exon_duckdb_amd import ExgError
    rng = np.random.default_rng(5)
    f = tf().parse_cigar
    for it in range(3000):
        s = b"".join(b"0" * int(rng.integers(0, 3) == 0) + b"%d%c" % (int(rng.integers(0, 400)) if rng.integers(0, 4) else int(rng.integers(0, 1 << 29)),
                                                                  ref.OPS[int(rng.integers(0, 9))]) for _ in range(int(rng.integers(1, 9))))
        if it % 2:
            k = int(rng.integers(0, len(s)))
            s = s[:k] + bytes([b"MI09 *x\x00"[int(rng.integers(0, 8))]]) + s[k + 1:]
        want = ref.error_offset(s)
        if want is None:
            assert f(s) == ops(*ref.parse(s)), s
        else:
            with pytest.raises(ExgError) as e:
                f(s)
            assert e.value.offset == want, s


def test_new_structs_have_the_c_layout(tmp_path):
    from exon_duckdb_amd import abi
    structs = {"struct exg_cigar_result": abi.CigarResult, "exg_cigar_op_args": abi.CigarOpArgs}
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs.items():
        prog.append(f'printf("{cname.split()[-1]} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            prog.append(f'printf("{cname.split()[-1]}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    for name in ("EXG_PE_CIGAR_INVALID", "EXG_PE_CIGAR_RANGE", "EXG_CIGAR_PARSE", "EXG_CIGAR_EXTRACT", "EXG_ABI_VERSION"):
        prog.append(f'printf("{name} %d\\n", {name});')
    prog.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert got["exg_cigar_result"] == "64"
    for cname, cls in structs.items():
        cname = cname.split()[-1]
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert int(got["EXG_PE_CIGAR_INVALID"]) == abi.EXG_PE_CIGAR_INVALID == 44 and int(got["EXG_PE_CIGAR_RANGE"]) == abi.EXG_PE_CIGAR_RANGE == 45
    assert int(got["EXG_CIGAR_PARSE"]) == abi.EXG_CIGAR_PARSE == 1 and int(got["EXG_CIGAR_EXTRACT"]) == abi.EXG_CIGAR_EXTRACT == 2
    assert int(got["EXG_ABI_VERSION"]) == abi.EXG_ABI_VERSION == 9


def test_library_surface_of_the_cigar_op():
    from exon_duckdb_amd import abi, load_library
    lib = load_library()
    assert lib.exg_parse_error_string(abi.EXG_PE_CIGAR_INVALID) == b"invalid CIGAR string"
    assert lib.exg_parse_error_string(abi.EXG_PE_CIGAR_RANGE) == b"CIGAR insertions exceed the sequence"
    assert lib.exg_parse_error_string(43) == b"unknown parse error" and lib.exg_parse_error_string(46) == b"unknown parse error"
    assert lib.exg_abi_version() == 9
    for op in (abi.EXG_CIGAR_PARSE, abi.EXG_CIGAR_EXTRACT):
        last = 0
        for n in (0, 1, 63, 64, 65, 100000, 1 << 24, (1 << 32) - 2):
            b = lib.exg_cigar_workspace_bytes(op, n, 0)
            assert b >= last and b >= 64 + 28 * n                    # monotone in n_rows
            last = b
    # parse_cigar keeps a counter per 4 KiB of out-of-line CIGAR text; extract_from_cigar keeps none
    small, big = lib.exg_cigar_workspace_bytes(abi.EXG_CIGAR_PARSE, 1000, 0), lib.exg_cigar_workspace_bytes(abi.EXG_CIGAR_PARSE, 1000, 1 << 30)
    assert big - small >= 12 * (1 << 18) and big - small < 13 * (1 << 18) + 4096
    assert lib.exg_cigar_workspace_bytes(abi.EXG_CIGAR_EXTRACT, 1000, 0) == lib.exg_cigar_workspace_bytes(abi.EXG_CIGAR_EXTRACT, 1000, 1 << 30)
    # argument checks that need no device: they are made before anything is enqueued
    a = abi.CigarOpArgs()
    assert lib.exg_cigar_op(None) == abi.EXG_E_INVALID_ARG and lib.exg_last_error_message().startswith(b"exg_cigar_op: ")
    assert lib.exg_cigar_op(C.byref(a)) == abi.EXG_E_INVALID_ARG and lib.exg_last_error_message().startswith(b"exg_cigar_op: ")
    buf = (C.c_uint8 * 65536)()
    p = (C.addressof(buf) + 15) & ~15

    def complete(op):
        a = abi.CigarOpArgs()
        a.op, a.n_rows = op, 10
        a.d_cigar = a.d_sequence = a.d_out_entries = a.d_out_op = a.d_out_len = a.d_out_start = a.d_out_end = a.d_out_sequence = p
        a.d_workspace = a.d_result = p
        a.ops_capacity = 4
        a.workspace_bytes = lib.exg_cigar_workspace_bytes(op, 10, 4096)         # (everything in place: only the check under test fails)
        return a

    def refused(a, text):
        assert lib.exg_cigar_op(C.byref(a)) == abi.EXG_E_INVALID_ARG
        msg = lib.exg_last_error_message()
        assert msg.startswith(b"exg_cigar_op: ") and text in msg, msg

    for op in (abi.EXG_CIGAR_PARSE, abi.EXG_CIGAR_EXTRACT):
        a = complete(op)
        a.workspace_bytes = lib.exg_cigar_workspace_bytes(op, 10, 0) - 8
        refused(a, b"workspace too small")
        a = complete(op)
        a.d_cigar = p + 8
        refused(a, b"unaligned")
        a = complete(op)
        a.d_cigar = None
        refused(a, b"null")
        a = complete(op)
        a.d_workspace = p + 4
        refused(a, b"unaligned")
        a = complete(op)
        a.d_result = None
        refused(a, b"null")
        a = complete(op)
        a.n_rows = (1 << 32) - 1
        refused(a, b"rows")
    a = complete(0)
    refused(a, b"unknown op 0")
    a = complete(3)
    refused(a, b"unknown op 3")
    for field in ("d_out_op", "d_out_len", "d_out_entries"):
        a = complete(abi.EXG_CIGAR_PARSE)
        setattr(a, field, None)
        refused(a, b"output")
    a = complete(abi.EXG_CIGAR_PARSE)
    a.d_out_op = p + 8
    refused(a, b"output")
    for field in ("d_sequence", "d_out_start", "d_out_end", "d_out_sequence"):
        a = complete(abi.EXG_CIGAR_EXTRACT)
        setattr(a, field, None)
        refused(a, b"output")
    a = complete(abi.EXG_CIGAR_EXTRACT)
    a.d_out_sequence = p + 8
    refused(a, b"output")
    assert lib.exg_cigar_result(None, None, None) == abi.EXG_E_INVALID_ARG and b"exg_cigar_result" in lib.exg_last_error_message()


def test_host_functions_under_asan_ubsan(tmp_path):
    """tests/cigar_asan_driver.cpp: a stand-alone program over exg_cigarfn.hpp and the two host scalars of
    exon_table_function.hpp (exactly-sized heap rows, the pins, every error kind, random rows, the backward walker of the
    device's tiles against the left-to-right parser), built with AddressSanitizer + UBSan"""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "cigar_asan"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "exon_duckdb_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "cigar_asan_driver.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "cigarfn host functions ok" in res.stdout


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc is not installed")
def test_kernel_resources(tmp_path):
    """the code object's own report: no scratch anywhere.  A tile is one wave and its workgroup's LDS — the
    staged rows — is all that bounds how many tiles a CU holds: under 10 KiB a wave and at most 64 VGPRs keep at least four
    waves a SIMD (16 tiles a CU) in flight, which is what hides the byte loads and the walkers' dependent loads (a variant that
    also copied the tile's bytes to LDS fell to three waves and measured slower: DESIGN 4.15).  The kernels with a thread per
    row use no LDS and reach the full eight waves."""
    from exon_duckdb_amd import build as B
    src = os.path.join(B.CSRC, "exg_cigarfn.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + B._flags() + B.FILE_FLAGS.get("exg_cigarfn.hip", []) + [
        "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "exg_cigarfn.s")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    blocks = [b for b in re.split(r"(?=remark: [^\n]*Function Name:)", p.stderr) if "Function Name: " in b]
    seen = {}
    for b in blocks:
        name = re.search(r"Function Name: (\S+)", b).group(1)
        field = lambda f: int(re.search(re.escape(f) + r": (\d+)", b).group(1))      # noqa: E731
        seen[name] = dict(vgprs=field("VGPRs"), scratch=field("ScratchSize [bytes/lane]"), occupancy=field("Occupancy [waves/SIMD]"),
                          lds=field("LDS Size [bytes/block]"))
        print(name, seen[name])
    own = {k: v for k, v in seen.items() if "cigarfn" in k}
    tiles = [v for k, v in own.items() if "k_tiles" in k]
    rows = [v for k, v in own.items() if any(n in k for n in ("k_rows", "k_emit_rows", "k_extract"))]
    assert len(tiles) == 2 and len(rows) == 3
    assert all(v["scratch"] == 0 for v in seen.values())
    for v in tiles:
        assert v["vgprs"] <= 64 and v["lds"] <= 10240 and v["occupancy"] >= 4
    for v in rows:
        assert v["lds"] == 0 and v["occupancy"] == 8
