"""Seven workgroups of the lean FASTQ scan, k_fused<FastqFormat, kLean>, per CU (profiles/fastq_seven_waves_ab.md),
checked on the compiler's own resource report.  No GPU needed: hipcc cross-compiles for gfx950.

    VGPRs <= 72       512 registers per SIMD lane / 7 waves, in the allocation granule of 8
    scratch 0         a register spilled in the hot path makes the wave wait for all its column stores at every reload
    occupancy >= 7    waves per SIMD, as the compiler computes it from the above
    LDS <= 23 405 B   160 KiB / 7 workgroups (half 0's newline masks wait in the byte buffer: FusedLdsT PARK)

It prints the scalar registers spilled and the static count of the lane moves that spilling them costs.  Every other FASTQ and
VCF instance of k_fused keeps what it had before the lean FASTQ scan went to seven waves: VGPRs, scratch and occupancy no worse
than the figures of profiles/fastq_input_end_ab.md.
"""
import os
import re
import shutil
import subprocess

import pytest

from exon_duckdb_amd import build as B

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LEAN = ("exg::FastqFormat", 0)

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc is not installed")

# (format, mode) -> (VGPRs, scratch bytes per lane, occupancy) at the parent commit; modes: 0 lean, 1 any-shape, 2 redo, 3 index
PARENT = {
    ("exg::FastqFormat", 1): (94, 0, 5),
    ("exg::FastqFormat", 2): (96, 44, 5),
    ("exg::VcfFormat", 0): (96, 16, 5),
    ("exg::VcfFormat", 1): (96, 48, 5),
    ("exg::VcfFormat", 2): (128, 20, 4),
    ("exg::VcfFormat", 3): (60, 0, 6),  # (its LDS, not its registers, bounds it)
}
SOURCES = ["exg_fastq_fused.hip", "exg_vcf.hip"]


def demangle(names):
    tool = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "llvm", "bin", "llvm-cxxfilt")
    tool = tool if os.path.exists(tool) else (shutil.which("llvm-cxxfilt") or shutil.which("c++filt"))
    assert tool, "no demangler (llvm-cxxfilt / c++filt)"
    out = subprocess.run([tool] + names, capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def reports(tmp_path, name):
    """{(format, mode): {field: value}} of every k_fused instance of one source, and the path of its assembly"""
    src = os.path.join(B.CSRC, name)
    asm = str(tmp_path / (name + ".s"))
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + B._flags() + B.FILE_FLAGS.get(name, []) + [
        "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", asm]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    blocks = {}
    for b in re.split(r"(?=remark: [^\n]*Function Name:)", p.stderr):
        m = re.search(r"Function Name: (\S+)", b)
        if m and "7k_fused" in m.group(1):
            blocks[m.group(1)] = b
    plain = demangle(sorted(blocks))
    out = {}
    for mangled, b in blocks.items():
        m = re.match(r"void exg::k_fused<(.+), (\d+)>\(", plain[mangled])
        assert m, plain[mangled]
        fields = {k: int(v) for k, v in re.findall(r"remark: [^\n]*?    ([A-Za-z][^:\n]*): (\d+)", b)}
        fields["mangled"] = mangled
        out[(m.group(1), int(m.group(2)))] = fields
    return out, asm


@pytest.fixture(scope="module")
def all_reports(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("seven_waves")
    found, asms = {}, {}
    for name in SOURCES:
        r, asm = reports(tmp, name)
        found.update(r)
        for key in r:
            asms[key] = asm
    return found, asms


def test_lean_fastq_scan_keeps_seven_workgroups_per_cu(all_reports):
    found, asms = all_reports
    assert LEAN in found, "no resource report for the lean FASTQ scan"
    f = found[LEAN]
    text = open(asms[LEAN]).read()
    m = re.search(r"^" + re.escape(f["mangled"]) + r":[^\n]*\n(.*?)\.Lfunc_end", text, re.S | re.M)
    assert m, "the lean FASTQ scan is not in the assembly"
    lane_moves = len(re.findall(r"\bv_readlane_b32\b", m.group(1))) + len(re.findall(r"\bv_writelane_b32\b", m.group(1)))
    vgprs, scratch = f["VGPRs"], f["ScratchSize [bytes/lane]"]
    occupancy, lds = f["Occupancy [waves/SIMD]"], f["LDS Size [bytes/block]"]
    print(f"k_fused<FastqFormat, kLean>: VGPRs {vgprs}, scratch {scratch} B/lane, occupancy {occupancy}, LDS {lds} B, "
          f"SGPRs Spill {f['SGPRs Spill']}, v_readlane + v_writelane {lane_moves}")
    assert vgprs <= 72
    assert scratch == 0
    assert occupancy >= 7
    assert lds <= 23405


@pytest.mark.parametrize("key", sorted(PARENT), ids=lambda k: f"{k[0].split('::')[-1]}-{k[1]}")
def test_other_instances_keep_their_resources(all_reports, key):
    found, _ = all_reports
    assert key in found, f"no resource report for k_fused<{key[0]}, {key[1]}>"
    f = found[key]
    vgprs, scratch, occupancy = f["VGPRs"], f["ScratchSize [bytes/lane]"], f["Occupancy [waves/SIMD]"]
    want = PARENT[key]
    print(f"k_fused<{key[0]}, {key[1]}>: VGPRs {vgprs} (parent {want[0]}), scratch {scratch} B/lane ({want[1]}), "
          f"occupancy {occupancy} ({want[2]}), LDS {f['LDS Size [bytes/block]']} B, SGPRs Spill {f['SGPRs Spill']}")
    assert vgprs <= want[0]
    assert scratch <= want[1]
    assert occupancy >= want[2]


def test_every_fastq_and_vcf_instance_is_listed(all_reports):
    found, _ = all_reports
    assert set(found) == set(PARENT) | {LEAN}, sorted(found)
