"""CPU checks of the alignment strings: the pins of the reference's test_align.test and the derived ones, every error text, the
host scalar that the DuckDB shim registers (reached through libexon_tf_test.so) against tests/alignstr_ref.py byte for byte —
whose own CIGARs are checked without wavefronts against the Gotoh matrix of tests/align_ref.py —, the match < 0 transform, the C
layout of the two new structs of include/exon_gpu.h, the workspace function, the argument checks of the C-ABI that need no
device, the stand-alone AddressSanitizer / UBSan driver and the resource report of the kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import align_ref
import alignstr_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "exon_gpu.h")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
TIE_SETS = align_ref.PARAM_SETS + [(2, 0, 1), (1, 0, 1)]      # in the last two a mismatch ties with an insertion plus a deletion
RANGE_TEXT = ("alignment_string: mismatch must be in 1..1023, gap_opening in 0..1023 and gap_extension in 1..1023, also after a match "
              "score below 0 is folded in (2 * mismatch - 2 * match, 2 * gap_opening, 2 * gap_extension - match)")


def tf():
    from exon_duckdb_amd import table_function
    return table_function


def error_text(*args):
    from exon_duckdb_amd import ExgError, abi
    with pytest.raises(ExgError) as e:
        tf().alignment_string(*args)
    assert e.value.code == abi.EXG_E_INVALID_ARG
    text = str(e.value)
    return text[text.index(": ") + 2:]


def tie_pairs(prm):
    """400 random pairs of lengths 0..24 over AC: low complexity makes ties the rule"""
    rng = np.random.default_rng(100 + sum(prm))
    return [(align_ref.random_seq(rng, int(rng.integers(0, 25)), b"AC"), align_ref.random_seq(rng, int(rng.integers(0, 25)), b"AC"))
            for _ in range(400)]


def mutated_pairs():
    """50 pairs of 150..300 bytes at 5 % and at 20 %"""
    rng = np.random.default_rng(7)
    out = []
    for it in range(50):
        a = align_ref.random_seq(rng, int(rng.integers(150, 301)))
        out.append((a, align_ref.mutate(rng, a, 0.05 if it % 2 else 0.2)))
    return out


def test_pins():
    f = tf().alignment_string
    # [PINNED] test_align.test
    assert f(b"AACC", b"AAACC") == b"2M1D2M"
    assert f(b"AACC", b"AAACC", 1, 1, 1, "memory_low") == b"2M1D2M"
    assert f(b"AACC", b"AAACC", -1, 1, 2, 3, "memory_low") == b"2M1D2M"
    assert error_text(b"AACC", b"AAACC", 1, 1, 1, 1, "memory_low") == "Match score must be negative or zero."
    assert tf().alignment_string_wfa_gap_affine(b"AACC", b"AAACC") == b"2M1D2M"
    # [DERIVED]
    assert f(b"AAA", b"AAAA") == b"3M1D"            # the greedy extend puts a gap in a run as far right as it goes
    assert f(b"", b"ACG") == b"3D" and f(b"ACG", b"") == b"3I"
    assert f(b"ACGT", b"AGGT") == b"1M1X2M"
    assert f(b"", b"") == b""
    assert f(None, b"ACG") is None and f(b"ACG", None) is None and f(None, None) is None
    assert ref.cigar(b"AACC", b"AAACC") == ref.cigar(b"AACC", b"AAACC", 1, 1, 1) == ref.cigar(b"AACC", b"AAACC", 1, 2, 3, match=-1) == b"2M1D2M"


def test_error_texts_and_parameter_limits():
    assert error_text(b"A", b"A", 1, 4, 6, 2, "memory_high") == "Match score must be negative or zero."
    assert error_text(b"A", b"A", 4, 6, 2, "memory") == "Invalid memory model: memory"
    assert error_text(b"A", b"A", 0, 4, 6, 2, "MEMORY_HIGH") == "Invalid memory model: MEMORY_HIGH"
    assert error_text(b"A", b"A", -1, 4, 6, 2, "") == "Invalid memory model: "
    for x, o, e in ((0, 6, 2), (1024, 6, 2), (-4, 6, 2), (4, -1, 2), (4, 1024, 2), (4, 6, 0), (4, 6, 1024), (1 << 40, 6, 2)):
        assert error_text(b"A", b"A", x, o, e, "memory_high") == RANGE_TEXT
        assert error_text(b"A", b"A", 0, x, o, e, "memory_high") == RANGE_TEXT
        assert error_text(b"A", b"A", -1, x, o, e, "memory_high") == RANGE_TEXT
    # in range before the transform, out of range after it: 2x - 2a, 2o, 2e - a
    assert error_text(b"A", b"A", -1, 511, 6, 2, "memory_high") == RANGE_TEXT          # x' = 1024
    assert error_text(b"A", b"A", -1, 4, 512, 2, "memory_high") == RANGE_TEXT          # o' = 1024
    assert error_text(b"A", b"A", -1, 4, 6, 512, "memory_high") == RANGE_TEXT          # e' = 1025
    assert error_text(b"A", b"A", -1022, 1, 0, 1, "memory_high") == RANGE_TEXT         # e' = 1024
    assert error_text(b"A", b"A", -(1 << 40), 1, 0, 1, "memory_high") == RANGE_TEXT
    f = tf().alignment_string
    assert f(b"AC", b"AG", -1, 510, 511, 511, "memory_high") == b"1M1X"                 # x' = 1022, o' = 1022, e' = 1023
    assert f(b"AC", b"AG", 1023, 1023, 1023, "memory_low") == b"1M1X" and f(b"AC", b"A", 1, 0, 1, "memory_med") == b"1M1I"
    assert error_text(b"A", b"A", 4) == "Invalid number of arguments for align function"
    # a NULL row does not hide a bind-time error; the match score wins over the rest, the limits over the memory model
    assert error_text(None, b"A", 1, 4, 6, 2, "memory_high") == "Match score must be negative or zero."
    assert error_text(b"A", b"A", 1, 0, 0, 0, "bogus") == "Match score must be negative or zero."
    assert error_text(b"A", b"A", 0, 0, 0, 0, "bogus") == RANGE_TEXT
    # pair too long: |text| + |pattern| <= 2^21
    half = b"A" * (1 << 20)
    assert error_text(half + b"A", half) == "alignment_string: the pair is longer than 2^21 bytes"
    assert f(half, half) == b"1048576M"


@pytest.mark.parametrize("prm", TIE_SETS, ids=str)
def test_oracle_is_an_optimal_alignment_and_the_host_scalar_equals_it(prm):
    """(a) passes (b), and the host scalar equals (a) byte for byte; no case is left out"""
    f = tf().alignment_string
    pairs = tie_pairs(prm) + mutated_pairs()
    assert len(pairs) == 450
    for t, p in pairs:
        want = ref.cigar(t, p, *prm)
        ref.check(t, p, want, *prm)
        got = f(t, p, *prm, "memory_high") if prm != align_ref.DEFAULTS else f(t, p)
        assert got == want, (prm, t, p, got, want)
        assert set(re.sub(rb"\d", b"", got)) <= set(b"MXID")


@pytest.mark.parametrize("match", [-1, -3])
def test_negative_match_is_the_transformed_call(match):
    f = tf().alignment_string
    rng = np.random.default_rng(-match)
    for x, o, e in ((4, 6, 2), (1, 1, 1), (2, 0, 1), (5, 40, 1)):
        folded = (2 * x - 2 * match, 2 * o, 2 * e - match)
        assert ref.fold(match, x, o, e) == folded
        for it in range(60):
            t = align_ref.random_seq(rng, int(rng.integers(0, 40)), b"AC" if it % 2 else b"ACGT")
            p = align_ref.mutate(rng, t, 0.2) if it % 3 else align_ref.random_seq(rng, int(rng.integers(0, 40)), b"AC")
            got = f(t, p, match, x, o, e, "memory_high")
            assert got == f(t, p, *folded, "memory_low") == ref.cigar(t, p, x, o, e, match=match), (t, p)
            ref.check(t, p, got, *folded)


def test_the_shim_registers_both_names():
    """duckdb_shim/exon_extension.cpp (compiled against the DuckDB stand-ins by test_host_logic.py) registers the two names as
    sets of the three signatures returning VARCHAR, on the host scalar tested here; the remark that they are missing is gone"""
    src = open(os.path.join(ROOT, "duckdb_shim", "exon_extension.cpp")).read()
    for name in ("alignment_string", "alignment_string_wfa_gap_affine"):
        assert f'RegisterAlignmentString(db, "{name}");' in src
    body = src[src.index("static void RegisterAlignmentString"):src.index("// sam_functions/module.cpp:32-77")]
    assert "{V, V}, {V, V, I, I, I, V}, {V, V, I, I, I, I, V}" in body and "LogicalType::VARCHAR," in body
    assert "exon_scan::AlignmentString(" in src and "exon_scan::AlignmentStringBindError(" in src
    assert "alignment_string* are not registered" not in src
    assert "Not built.**  `alignment_string" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_history_limit_of_the_host_scalar():
    """two unrelated 12 000-byte strings: about 50 000 steps over up to 24 001 diagonals pass 1 GiB long before the end"""
    rng = np.random.default_rng(5)
    a, b = align_ref.random_seq(rng, 12000), align_ref.random_seq(rng, 12000)
    assert error_text(a, b, 4, 6, 1, "memory_high") == "alignment_string: the alignment's wavefronts exceed 1 GiB"


def test_new_structs_have_the_c_layout(tmp_path):
    from exon_duckdb_amd import abi
    structs = {"struct exg_align_string_result": abi.AlignStringResult, "exg_align_string_args": abi.AlignStringArgs}
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs.items():
        key = cname.split()[-1]
        prog.append(f'printf("{key} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            prog.append(f'printf("{key}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    prog.append('printf("EXG_ABI_VERSION %d\\n", EXG_ABI_VERSION); return 0; }')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert got["exg_align_string_result"] == "64"
    for cname, cls in structs.items():
        key = cname.split()[-1]
        assert int(got[key]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{key}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    # the input side is exg_align_score_args's, unchanged
    for fname, _ in abi.AlignScoreArgs._fields_[:12]:
        assert getattr(abi.AlignStringArgs, fname).offset == getattr(abi.AlignScoreArgs, fname).offset
    assert int(got["EXG_ABI_VERSION"]) == abi.EXG_ABI_VERSION == 9


def history_entries(e, max_pair_bytes, steps):
    return sum(min(max_pair_bytes + 1, 2 * (s // e) + 3) for s in range(steps + 1))


def test_workspace_function():
    from exon_duckdb_amd import load_library
    ws = load_library().exg_align_string_workspace_bytes
    last = 0
    for n in (0, 1, 63, 64, 65, 1023, 1024, 100000, 1 << 24, (1 << 32) - 2):
        b = ws(n, 300, 4, 6, 2, 0, 1000)
        assert b >= last and b >= 64 + 24 * n + 1000                                   # monotone in n_rows
        last = b
    sizes = [ws(5000, mpb, 4, 6, 2, 0, 0) for mpb in (0, 1, 12, 150, 320, 1000, 29999, 30000)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)                    # ... in max_pair_bytes
    sizes = [ws(5000, 30000, 4, 6, 2, cap, 0) for cap in (1, 10, 100, 1000, 60012, 0)]  # 0 = no cap = the bound 2o + e * 30000
    assert sizes == sorted(sizes) and sizes[-1] == ws(5000, 30000, 4, 6, 2, 60012, 0) == ws(5000, 30000, 4, 6, 2, 70000, 0)
    assert ws(5000, 300, 4, 6, 2, 0, 1 << 20) - ws(5000, 300, 4, 6, 2, 0, 0) == 1 << 20     # ... and the staging area is out_capacity
    # one case by hand: 8 rows (8 slots), max_pair_bytes 10, (4,6,2), max_penalty 9 -> 10 steps of 3,3,5,5,7,7,9,9,11,11 = 70
    # diagonals; 16-bit entries.  counters 64 | list 32 | rowlen 32 | rowpos 64 | offs 80 (72) | scan scratch 32 (3 x 8) | no
    # ring slots (every pair fits LDS) | 8 x (directory 10 x 16 | history 3 x 70 x 2 -> 432 | text 2 x 10 + 16 -> 48) | staging 112 (100)
    assert history_entries(2, 10, 9) == 70
    assert ws(8, 10, 4, 6, 2, 9, 100) == 64 + 32 + 32 + 64 + 80 + 32 + 8 * (160 + 432 + 48) + 112
    # 1 024 resident pairs keep 150 bp reads (max_pair_bytes 320, defaults, no cap) below 1 GiB
    assert history_entries(2, 320, 652) == 158733
    reads = ws(3000000, 320, 4, 6, 2, 0, 0)
    assert 1024 * 3 * 158733 * 2 < reads < 1 << 30
    assert ws(100000, 320, 4, 6, 2, 100, 0) < 40 << 20
    for bad in ((1000, 300, 0, 6, 2, 0, 0), (1000, 300, 4, 1024, 2, 0, 0), (1000, 300, 4, 6, 0, 0, 0), (1000, (1 << 21) + 1, 4, 6, 2, 0, 0),
                ((1 << 32) - 1, 300, 4, 6, 2, 0, 0), (1000, 1 << 21, 4, 6, 2, 0, 0), (1000, 300, 4, 6, 2, 0, 1 << 49)):
        assert ws(*bad) == 0                                       # (the last two: a workspace above 2^48 bytes)


def test_workspace_sizes_are_pinned():
    """exg_align_string_workspace_bytes(n_rows, max_pair_bytes, mismatch, gap_opening, gap_extension, max_penalty, out_capacity) as
    the tree before the forward pass was stated once (exg_align_core.hpp) returned it: n_rows around kPairs = 1 024 slots,
    max_pair_bytes on both sides of the all-LDS threshold (526 | 527 at the defaults) and of the 16-bit history (29 999 | 30 000),
    max_penalty 0 and 100, a ring too deep for LDS, and a history above 2^48 bytes (0)"""
    from exon_duckdb_amd import load_library
    ws = load_library().exg_align_string_workspace_bytes
    pins = {(0, 300, 4, 6, 2, 0, 0): 96, (1, 300, 4, 6, 2, 100, 64): 136480, (3, 526, 4, 6, 2, 0, 1000): 10236336,
            (3, 527, 4, 6, 2, 0, 1000): 18384816, (1023, 526, 4, 6, 2, 100, 0): 35364960, (1024, 527, 4, 6, 2, 100, 0): 43475056,
            (1025, 300, 4, 6, 2, 0, 4096): 869724320, (100000, 300, 4, 6, 2, 100, 1 << 20): 38330416,
            (100000, 29999, 4, 6, 2, 100, 0): 558899248, (100000, 30000, 4, 6, 2, 100, 0): 591503408,
            (1025, 29999, 4, 6, 2, 0, 0): 8298301661344, (3, 30000, 4, 6, 2, 0, 0): 65287938112,
            (1024, 300, 5, 200, 1, 100, 100): 129745120, (1000, 1 << 21, 4, 6, 2, 0, 0): 0}
    for args, want in pins.items():
        assert ws(*args) == want, args


def test_argument_errors_that_need_no_device():
    from exon_duckdb_amd import abi, load_library
    lib = load_library()
    a = abi.AlignStringArgs()
    assert lib.exg_align_string(None) == abi.EXG_E_INVALID_ARG
    assert lib.exg_align_string(C.byref(a)) == abi.EXG_E_INVALID_ARG and b"exg_align_string: bad arguments" in lib.exg_last_error_message()
    buf = (C.c_uint8 * 4096)()
    at = (C.addressof(buf) + 15) & ~15
    a.d_text = a.d_pattern = a.d_out_strings = a.d_out_payload = a.d_result = a.d_workspace = at
    a.n_rows, a.mismatch, a.gap_opening, a.gap_extension, a.max_pair_bytes, a.out_capacity = 10, 4, 6, 2, 300, 64
    need = lib.exg_align_string_workspace_bytes(10, 300, 4, 6, 2, 0, 64)
    a.workspace_bytes = need - 8
    assert lib.exg_align_string(C.byref(a)) == abi.EXG_E_INVALID_ARG and b"workspace too small" in lib.exg_last_error_message()
    a.workspace_bytes = need

    def refused(what, **fields):
        saved = {k: getattr(a, k) for k in fields}
        for k, v in fields.items():
            setattr(a, k, v)
        rc, msg = lib.exg_align_string(C.byref(a)), lib.exg_last_error_message()
        for k, v in saved.items():
            setattr(a, k, v)
        assert rc == abi.EXG_E_INVALID_ARG and msg.startswith(b"exg_align_string: ") and what in msg, msg

    refused(b"mismatch 0", mismatch=0)
    refused(b"gap_opening 1024", gap_opening=1024)
    refused(b"gap_extension 0", gap_extension=0)
    refused(b"max_pair_bytes", max_pair_bytes=(1 << 21) + 1)
    refused(b"rows", n_rows=(1 << 32) - 1)
    refused(b"lanes 8", lanes=8)
    refused(b"reserved 1", reserved=1)
    refused(b"bad arguments", d_out_strings=at + 8)
    refused(b"bad arguments", d_out_payload=None)
    refused(b"bad arguments", d_text=None)
    refused(b"2^48", max_pair_bytes=1 << 21)
    assert lib.exg_align_string_result(None, None, None) == abi.EXG_E_INVALID_ARG and b"exg_align_string_result" in lib.exg_last_error_message()


def test_host_functions_under_asan_ubsan(tmp_path):
    """tests/alignstr_asan_driver.cpp: a stand-alone program over exg_alignfn.hpp and the host scalar of
    exon_table_function.hpp (exactly-sized heap strings, every parameter set, the pins, the limits and the bind-time errors),
    built with AddressSanitizer + UBSan and run as a program"""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "alignstr_asan"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "exon_duckdb_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "alignstr_asan_driver.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "alignstr host functions ok" in res.stdout


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc is not installed")
def test_kernel_resources(tmp_path):
    """the code object's own report for exg_alignstr.hip: no scratch in any kernel; the instances of k_align with
    the history recorder that use the LDS policy declare no static LDS (a pair's share is sized at launch).  Observed: 86 / 86 /
    77 VGPRs at 16 / 32 / 64 lanes, 108 in the two global instances, in the tree before the forward pass was stated once and in
    this one (profiles/strcol_refactor_ab.md).  1 024 resident pairs are four waves a CU at most, one a SIMD: the occupancy relied on is 1; the
    bounds below keep the instances away from the 128-VGPR step all the same."""
    from exon_duckdb_amd import build as B
    src = os.path.join(B.CSRC, "exg_alignstr.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + B._flags() + B.FILE_FLAGS.get("exg_alignstr.hip", []) + [
        "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "exg_alignstr.s")]
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
    assert not any("ScoreRec" in k for k in seen)
    lds = [v for k, v in seen.items() if "k_align" in k and "HistoryRec" in k and "LdsPolicy" in k]
    glob = [v for k, v in seen.items() if "k_align" in k and "HistoryRec" in k and "GlobalPolicy" in k]
    assert len(lds) == 3 and len(glob) == 2
    assert any("k_place" in k for k in seen) and any("k_finish" in k for k in seen)
    assert all(v["scratch"] == 0 for v in seen.values())
    for v in lds:
        assert v["lds"] == 0 and v["vgprs"] <= 96 and v["occupancy"] >= 4
    for v in glob:
        assert v["vgprs"] <= 112 and v["occupancy"] >= 4
