"""CPU checks of the alignment scores: the pins of the reference and the derived ones, the host scalar that the DuckDB shim
registers (reached through libexon_tf_test.so) against tests/align_ref.py — a plain Gotoh DP that shares nothing with the library
— bit for bit, every error text and parameter limit, the C layout of the two new structs of include/exon_gpu.h, the argument
checks of the C-ABI that need no device, the stand-alone AddressSanitizer / UBSan driver of the host functions, and the resource
report of the kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import align_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "exon_gpu.h")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def tf():
    from exon_duckdb_amd import table_function
    return table_function


def bits(x):
    return np.float32(x).tobytes()


def error_text(*args):
    from exon_duckdb_amd import ExgError, abi
    with pytest.raises(ExgError) as e:
        tf().alignment_score(*args)
    assert e.value.code == abi.EXG_E_INVALID_ARG
    text = str(e.value)
    return text[text.index(": ") + 2:]


def test_pins():
    f = tf().alignment_score
    assert bits(f(b"AACC", b"AACC")) == bits(0.0)                    # test_align.test:24-26; +0, not -0
    assert tf().alignment_score_wfa_gap_affine(b"AACC", b"AACC") == 0.0
    assert f(b"AACC", b"AAACC") == -8.0 and f(b"AACC", b"AAACC", 1, 1, 1, "memory_high") == -2.0
    assert f(b"", b"ACG") == -12.0 and bits(f(b"", b"")) == bits(0.0)
    assert f(b"AACC", b"AAACC", 0, 4, 6, 2, "memory_low") == -8.0    # match = 0 is the six-argument case
    assert f(None, b"ACG") is None and f(b"ACG", None) is None
    assert f(b"acgt", b"ACGT") == -16.0 and f(b"NNNN", b"NNNN") == 0.0        # bytes as bytes: case-sensitive, N equals N
    assert f(b"\x00\xff\x80A", b"\x00\xff\x80A") == 0.0 and f(b"\x00", b"\xff") == -4.0
    # arguments by position as the signatures name them: gap_opening is argument 3, gap_extension argument 4
    # (module.cpp:68-72 reads argument 4 for both)
    assert f(b"AACC", b"AAACC", 9, 5, 1, "memory_med") == -6.0 and f(b"AACC", b"AAACC", 9, 1, 5, "memory_med") == -6.0
    assert f(b"AACC", b"AAAACC", 9, 5, 1, "memory_med") == -7.0 and f(b"AACC", b"AAAACC", 9, 1, 5, "memory_med") == -11.0
    for prm in ref.PARAM_SETS:
        assert ref.penalty(b"AACC", b"AAACC", *prm) == prm[1] + prm[2]


def test_the_oracles_two_forms_agree():
    rng = np.random.default_rng(0)
    for prm in ref.PARAM_SETS:
        for it in range(40):
            a = ref.random_seq(rng, int(rng.integers(0, 25)), b"AC" if it % 2 else b"ACGT")
            b = ref.mutate(rng, a, 0.3) if it % 3 else ref.random_seq(rng, int(rng.integers(0, 25)))
            assert ref.penalty(a, b, *prm) == ref.penalty_scalar(a, b, *prm), (prm, a, b)


@pytest.mark.parametrize("prm", ref.PARAM_SETS, ids=str)
def test_host_scalar_against_the_oracle(prm):
    """random and mutated pairs of length 0..40, 500 a parameter set, bit for bit; text and pattern are symmetric"""
    rng = np.random.default_rng(sum(prm))
    f = tf().alignment_score
    for it in range(500):
        a = ref.random_seq(rng, int(rng.integers(0, 41)), b"AC" if it % 5 == 0 else b"ACGT")
        b = ref.mutate(rng, a, 0.2) if it % 2 else ref.random_seq(rng, int(rng.integers(0, 41)))
        want = ref.score(a, b, *prm)
        got = f(a, b, *prm, "memory_high") if prm != ref.DEFAULTS or it % 2 else f(a, b)
        assert bits(got) == bits(want), (prm, a, b, got, want)
        if it % 10 == 0:
            assert bits(f(b, a, *prm, "memory_low")) == bits(want)


def test_host_scalar_on_longer_pairs():
    rng = np.random.default_rng(3)
    f = tf().alignment_score
    for n, rate in ((150, 0.01), (150, 0.05), (700, 0.1), (2000, 0.02)):
        a = ref.random_seq(rng, n)
        b = ref.mutate(rng, a, rate)
        assert bits(f(a, b)) == bits(ref.score(a, b))
    a, b = ref.random_seq(rng, 300), ref.random_seq(rng, 10)
    assert bits(f(a, b)) == bits(ref.score(a, b)) and bits(f(a, b, 20, 2, 1, "memory_med")) == bits(ref.score(a, b, 20, 2, 1))


def test_error_texts_and_parameter_limits():
    assert error_text(b"A", b"A", 1, 4, 6, 2, "memory_high") == "Match score must be negative or zero."      # module.cpp:101
    assert "not supported" in error_text(b"A", b"A", -1, 4, 6, 2, "memory_high")
    assert error_text(b"A", b"A", 4, 6, 2, "memory") == "Invalid memory model: memory"                       # module.cpp:91
    assert error_text(b"A", b"A", 0, 4, 6, 2, "MEMORY_HIGH") == "Invalid memory model: MEMORY_HIGH"
    assert error_text(b"A", b"A", 4, 6, 2, "") == "Invalid memory model: "
    limits = "alignment_score: mismatch must be in 1..1023, gap_opening in 0..1023 and gap_extension in 1..1023"
    for x, o, e in ((0, 6, 2), (1024, 6, 2), (-4, 6, 2), (4, -1, 2), (4, 1024, 2), (4, 6, 0), (4, 6, 1024), (1 << 40, 6, 2)):
        assert error_text(b"A", b"A", x, o, e, "memory_high") == limits
        assert error_text(b"A", b"A", 0, x, o, e, "memory_high") == limits
    f = tf().alignment_score
    assert f(b"AC", b"AG", 1, 0, 1, "memory_high") == -1.0 and f(b"AC", b"AG", 1023, 1023, 1023, "memory_high") == -1023.0
    assert f(b"AC", b"A", 1023, 1023, 1023, "memory_low") == -2046.0
    assert error_text(b"A", b"A", 4) == "Invalid number of arguments for align function"                     # module.cpp:305
    # a NULL row does not hide a bind-time error: the checks run before any row
    assert error_text(None, b"A", 1, 4, 6, 2, "memory_high") == "Match score must be negative or zero."
    # the match score wins over the rest, the limits over the memory model
    assert error_text(b"A", b"A", 1, 0, 0, 0, "bogus") == "Match score must be negative or zero."
    assert error_text(b"A", b"A", 0, 0, 0, 0, "bogus") == limits


def test_new_structs_have_the_c_layout(tmp_path):
    from exon_duckdb_amd import abi
    structs = {"exg_align_score_result": abi.AlignScoreResult, "exg_align_score_args": abi.AlignScoreArgs}
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs.items():
        prog.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            prog.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    prog.append('printf("EXG_PE_ALIGN_TOO_LONG %d\\n", EXG_PE_ALIGN_TOO_LONG); printf("EXG_ABI_VERSION %d\\n", EXG_ABI_VERSION);')
    prog.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert got["exg_align_score_result"] == "64"
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert int(got["EXG_PE_ALIGN_TOO_LONG"]) == abi.EXG_PE_ALIGN_TOO_LONG == 33 and int(got["EXG_ABI_VERSION"]) == abi.EXG_ABI_VERSION == 9


def test_library_surface_of_the_alignment_op():
    from exon_duckdb_amd import abi, load_library
    lib = load_library()
    assert lib.exg_parse_error_string(abi.EXG_PE_ALIGN_TOO_LONG) == b"alignment pair too long"
    assert lib.exg_parse_error_string(29) == b"unknown parse error" and lib.exg_parse_error_string(34) == b"unknown parse error"
    last = 0
    for n in (0, 1, 63, 64, 65, 100000, 1 << 24, (1 << 32) - 2):
        b = lib.exg_align_workspace_bytes(n, 300, 4, 6, 2)
        assert b >= last and b >= 64 + 4 * n                   # monotone in n_rows
        last = b
    reads, long_rows = lib.exg_align_workspace_bytes(1000, 300, 4, 6, 2), lib.exg_align_workspace_bytes(1000, 30000, 4, 6, 2)
    assert reads < 64 + 4096 and long_rows >= 256 * 15 * 30001 * 4          # reads fit LDS: no slots; long pairs: 256 slots
    assert lib.exg_align_workspace_bytes(1000, 300, 5, 200, 1) > reads        # a ring too deep for LDS takes slots too
    for bad in ((1000, 300, 0, 6, 2), (1000, 300, 4, 1024, 2), (1000, 300, 4, 6, 0), (1000, (1 << 21) + 1, 4, 6, 2), ((1 << 32) - 1, 300, 4, 6, 2)):
        assert lib.exg_align_workspace_bytes(*bad) == 0
    # argument checks that need no device: they are made before anything is enqueued
    a = abi.AlignScoreArgs()
    assert lib.exg_align_score(None) == abi.EXG_E_INVALID_ARG
    assert lib.exg_align_score(C.byref(a)) == abi.EXG_E_INVALID_ARG and b"exg_align_score" in lib.exg_last_error_message()
    ws = (C.c_uint8 * 4096)()                                  # everything in place but the workspace 8 bytes short
    a.d_text = a.d_pattern = a.d_out_float = a.d_result = a.d_workspace = (C.addressof(ws) + 15) & ~15
    a.n_rows, a.mismatch, a.gap_opening, a.gap_extension, a.max_pair_bytes = 10, 4, 6, 2, 300
    a.workspace_bytes = lib.exg_align_workspace_bytes(10, 300, 4, 6, 2) - 8
    assert lib.exg_align_score(C.byref(a)) == abi.EXG_E_INVALID_ARG and b"workspace too small" in lib.exg_last_error_message()
    assert lib.exg_align_result(None, None, None) == abi.EXG_E_INVALID_ARG and b"exg_align_result" in lib.exg_last_error_message()


def test_workspace_sizes_are_pinned():
    """exg_align_workspace_bytes(n_rows, max_pair_bytes, mismatch, gap_opening, gap_extension) as the tree before the forward pass
    was stated once (exg_align_core.hpp) returned it: n_rows around the 16-byte rounding of the list, max_pair_bytes on both sides
    of the all-LDS threshold (lds_need(15, 526) = 16 360 <= 16 384 < lds_need(15, 527)) and of 30 000, and a ring too deep for LDS"""
    from exon_duckdb_amd import load_library
    ws = load_library().exg_align_workspace_bytes
    pins = {(0, 300, 4, 6, 2): 64, (1, 300, 4, 6, 2): 80, (3, 526, 4, 6, 2): 80, (3, 527, 4, 6, 2): 8110160,
            (1023, 526, 4, 6, 2): 4160, (1024, 527, 4, 6, 2): 8114240, (1025, 300, 4, 6, 2): 4176, (100000, 300, 4, 6, 2): 400064,
            (100000, 29999, 4, 6, 2): 461200064, (100000, 30000, 4, 6, 2): 461216448, (1025, 29999, 4, 6, 2): 460804176,
            (1, 30000, 4, 6, 2): 460816464, (1024, 300, 5, 200, 1): 63500352}
    for args, want in pins.items():
        assert ws(*args) == want, args


def test_host_functions_under_asan_ubsan(tmp_path):
    """tests/align_asan_driver.cpp: a stand-alone program over exg_alignfn.hpp and the host scalar of exon_table_function.hpp
    (exactly-sized heap strings, every parameter set, the limits and the bind-time errors), built with AddressSanitizer + UBSan"""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "align_asan"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "exon_duckdb_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "align_asan_driver.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "alignfn host functions ok" in res.stdout


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc is not installed")
def test_kernel_resources(tmp_path):
    """the code object's own report for the four instances of k_align with the score recorder (the string op's
    instances of the same template are held to their own bounds by test_alignstr_host.py): no scratch anywhere; the LDS policy's
    instances declare no static LDS (a pair's share is sized at launch) and keep at most 64 VGPRs = 8 waves a SIMD, so that
    LDS alone decides how many pairs a CU holds (16 of 150 bp reads: four waves a SIMD at 64 lanes a pair)"""
    from exon_duckdb_amd import build as B
    src = os.path.join(B.CSRC, "exg_alignfn.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + B._flags() + B.FILE_FLAGS.get("exg_alignfn.hip", []) + [
        "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "exg_alignfn.s")]
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
    assert not any("HistoryRec" in k for k in seen)
    lds = [v for k, v in seen.items() if "k_align" in k and "ScoreRec" in k and "LdsPolicy" in k]
    glob = [v for k, v in seen.items() if "k_align" in k and "ScoreRec" in k and "GlobalPolicy" in k]
    assert len(lds) == 3 and len(glob) == 1 and len(seen) == 6
    assert all(v["scratch"] == 0 for v in seen.values())
    for v in lds:
        assert v["vgprs"] <= 64 and v["occupancy"] >= 8 and v["lds"] == 0
    assert glob[0]["vgprs"] <= 80 and glob[0]["occupancy"] >= 6
