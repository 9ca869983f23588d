"""AddressSanitizer + UBSan build of the host-only parsers of libexon_gpu (gzip member index, the BGZF member walk, zstd
frame / block walk, the VCF header parser, the shard planner, the `filters` grammar, next_batch's HIP-free decisions, the format table), driven over valid streams, truncations and random mutations (tests/host_asan_driver.cpp).  GPU
sanitizers do not exist on the pool; everything these parsers read is user input."""
import gzip
import os
import subprocess

import pytest

import gzip_members
from zstd_util import compress, fastq_text, skippable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exon_duckdb_amd", "csrc")


def bgzf(data, block):
    return gzip_members.bgzf(data, block, eof=False)


def build_driver(exe):
    """tests/host_asan_driver.cpp with the host parsers it drives, under AddressSanitizer + UBSan"""
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           "-I", "/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(exe),
           os.path.join(ROOT, "tests", "host_asan_driver.cpp"), os.path.join(CSRC, "exg_gzip.cpp"), os.path.join(CSRC, "exg_zstd_index.cpp"),
           os.path.join(CSRC, "exg_rd_bgzf.cpp"), os.path.join(CSRC, "exg_vcf_header.cpp"), os.path.join(CSRC, "exg_rd_plan.cpp"), os.path.join(CSRC, "exg_rd_fanout.cpp"), os.path.join(CSRC, "exg_map_guard.cpp"), "-lpthread"]
    subprocess.check_call(cmd)


def run_driver(exe, paths):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:handle_sigbus=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([str(exe)] + paths, env=env, capture_output=True, text=True)


def test_host_parsers_under_asan_ubsan(tmp_path):
    if not os.path.isdir("/opt/rocm/include"):
        pytest.skip("HIP headers not found")
    exe = tmp_path / "host_asan"
    build_driver(exe)
    text = fastq_text(3000, 4)
    files = {
        "a.gz": gzip.compress(text, 6, mtime=0),
        "b.gz": bgzf(text, 7000),
        "c.gz": gzip.compress(text[:5000], 6, mtime=0) + bgzf(text[5000:60000], 9000) + gzip.compress(b"", 6, mtime=0),
        "a.zst": compress(text, 3, True),
        "b.zst": compress(text[:40000], 19, True, window_log=12, content_size=False) + skippable(b"meta") + compress(text[40000:], 1, False),
        "c.zst": b"".join(compress(text[i:i + 5001], 1 + i % 5, i % 2 == 0) for i in range(0, 60000, 5001)),
    }
    paths = []
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
        paths.append(str(tmp_path / name))
    res = run_driver(exe, paths)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "runs" in res.stdout
