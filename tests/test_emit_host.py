"""AddressSanitizer + UBSan build of the emitter's host decisions that make no HIP call (tests/emit_host_driver.cpp): the region
layout of the nested VCF builder and its zero-skip decision, the key table the kernels probe (exg_nested_layout.hpp), and the
Arrow C data export of a batch's columns with its keep-alive (exg_arrow_export.hpp).  The driver is a program of its own: it
links no HIP library and is not loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exon_duckdb_amd", "csrc")


def build_driver(exe):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           "-I", "/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(exe),
           os.path.join(ROOT, "tests", "emit_host_driver.cpp")]
    subprocess.check_call(cmd)


def test_emit_host_decisions_under_asan_ubsan(tmp_path):
    exe = tmp_path / "emit_host"
    build_driver(exe)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "checks" in res.stdout
