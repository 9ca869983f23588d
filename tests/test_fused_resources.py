"""What the compiler makes of the lean FASTQ scan, k_fused<FastqFormat, kLean>: the conditions DESIGN 4.1 gives for six
workgroups of it per CU (6 x 48 KiB of input in flight), checked on the code object's own resource report.  No GPU needed:
hipcc cross-compiles for gfx950.

    VGPRs <= 80       512 registers per SIMD lane / 6 waves, in the allocation granule of 8
    scratch 0         a register spilled in the hot path makes the wave wait for all its column stores at every reload
    occupancy >= 6    waves per SIMD, as the compiler computes it from the above
    LDS <= 27 306 B   160 KiB / 6 workgroups

It also prints the scalar registers spilled and the static count of the lane moves that spilling them costs (v_readlane +
v_writelane): 52 and 248 at the commit before this file existed.
"""
import os
import re
import shutil
import subprocess

import pytest

from exon_duckdb_amd import build as B

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LEAN = "_ZN3exg7k_fusedINS_11FastqFormatELi0E"  # k_fused<exg::FastqFormat, 0 = kLean>

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc is not installed")


def test_lean_fastq_scan_keeps_six_workgroups_per_cu(tmp_path):
    src = os.path.join(B.CSRC, "exg_fastq_fused.hip")
    asm = str(tmp_path / "exg_fastq_fused.s")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + B._flags() + B.FILE_FLAGS.get("exg_fastq_fused.hip", []) + [
        "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", asm]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    blocks = [b for b in re.split(r"(?=remark: [^\n]*Function Name:)", p.stderr) if "Function Name: " + LEAN in b]
    assert len(blocks) == 1, "no resource report for the lean FASTQ scan"

    def field(name):
        m = re.search(re.escape(name) + r": (\d+)", blocks[0])
        assert m, name
        return int(m.group(1))

    vgprs, scratch = field("VGPRs"), field("ScratchSize [bytes/lane]")
    occupancy, lds = field("Occupancy [waves/SIMD]"), field("LDS Size [bytes/block]")
    text = open(asm).read()
    m = re.search(r"^" + LEAN + r"\w*:[^\n]*\n(.*?)\.Lfunc_end", text, re.S | re.M)
    assert m, "the lean FASTQ scan is not in the assembly"
    lane_moves = len(re.findall(r"\bv_readlane_b32\b", m.group(1))) + len(re.findall(r"\bv_writelane_b32\b", m.group(1)))
    print(f"k_fused<FastqFormat, kLean>: VGPRs {vgprs}, scratch {scratch} B/lane, occupancy {occupancy}, LDS {lds} B, "
          f"SGPRs Spill {field('SGPRs Spill')}, v_readlane + v_writelane {lane_moves}")
    assert vgprs <= 80
    assert scratch == 0
    assert occupancy >= 6
    assert lds <= 27306
