"""What the compiler makes of the line-row driver (csrc/exg_line_rows.hpp) for each of its formats, BED and SAM, checked on the
code object's own resource report.  No GPU needed: hipcc cross-compiles for gfx950.

k_fused<LineRowsFormat<R>, kFullPrimary>, the scan a reader runs (four waves per SIMD is the build because
it is the occupancy without scratch in the emission loop):

    scratch 0         a scratch reload in the emission loop waits for every column store the wave has in flight
    occupancy >= 4    waves per SIMD
    VGPRs <= 128      the four-wave budget: 512 registers per SIMD lane / 4
    LDS <= 23 768 B   the staged half, its line list and the window: what the register file, not LDS, lets six workgroups share

k_line_rows<R> (general path) and k_line_far<R, 2> (the lines that begin in front of a half's window): scratch 0 and
occupancy >= 5.  It prints the measured rows.
"""
import os
import re
import shutil
import subprocess

import pytest

from exon_duckdb_amd import build as B

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc is not installed")


@pytest.mark.parametrize("unit,rows", [("exg_bed.hip", "BedRows"), ("exg_sam.hip", "SamRows")])
def test_line_row_kernels_keep_their_occupancy(tmp_path, unit, rows):
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + B._flags() + B.FILE_FLAGS.get(unit, []) + [
        "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", os.path.join(B.CSRC, unit), "-o", str(tmp_path / "unit.s")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    tag = "%d%s" % (len(rows), rows)  # the traits struct in an Itanium-mangled name
    kernels = {"fused": "_ZN3exg7k_fusedINS_14LineRowsFormatINS_%sEEELi1E" % tag,  # k_fused<LineRowsFormat<R>, 1 = kFullPrimary>
               "lines": "_ZN3exg11k_line_rowsINS_%sEEE" % tag,
               "far": "_ZN3exg10k_line_farINS_%sELj2EEE" % tag}
    got = {}
    for name, mangled in kernels.items():
        blocks = [b for b in re.split(r"(?=remark: [^\n]*Function Name:)", p.stderr) if "Function Name: " + mangled in b]
        assert len(blocks) == 1, "no resource report for %s of %s" % (name, rows)

        def field(label):
            m = re.search(re.escape(label) + r": (\d+)", blocks[0])
            assert m, label
            return int(m.group(1))

        got[name] = {"vgprs": field("VGPRs"), "scratch": field("ScratchSize [bytes/lane]"), "occupancy": field("Occupancy [waves/SIMD]"),
                     "sgpr_spill": field("SGPRs Spill"), "lds": field("LDS Size [bytes/block]")}
        print("%s %s: VGPRs %d, scratch %d B/lane, occupancy %d, SGPRs Spill %d, LDS %d B" % (
            rows, name, got[name]["vgprs"], got[name]["scratch"], got[name]["occupancy"], got[name]["sgpr_spill"], got[name]["lds"]))
    assert got["fused"]["scratch"] == 0
    assert got["fused"]["occupancy"] >= 4
    assert got["fused"]["vgprs"] <= 128
    assert got["fused"]["lds"] <= 23768
    for name in ("lines", "far"):
        assert got[name]["scratch"] == 0
        assert got[name]["occupancy"] >= 5
