"""The hot path of the lean FASTQ scan, k_fused<FastqFormat, kLean>, as the compiler emits it: the kernel is bound by
instruction issue as much as by bandwidth, so what every workgroup executes per chunk is checked on the assembly.  No GPU needed:
hipcc cross-compiles for gfx950.

    twelve `global_load_dwordx4 ... nt` before the first `s_waitcnt vmcnt`      all of a super-tile's input in flight at once
    the waits that follow count 11, 10, ... 0                                   each chunk is classified when it arrives
    no v_cndmask on a loaded register between them                              the end of the input is not the loop's business: the
                                                                                one workgroup that holds it masks behind the loop
    static v_* instructions < 2 041                                             the count before the end-of-input work left the loop
                                                                                (profiles/fastq_prefix_wait_ab.md)
"""
import os
import re
import shutil
import subprocess

import pytest

from exon_duckdb_amd import build as B

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LEAN = "_ZN3exg7k_fusedINS_11FastqFormatELi0E"  # k_fused<exg::FastqFormat, 0 = kLean>
N_CHUNKS = 12                                   # kFastqHalves x kRows 16-byte chunks per thread
PARENT_STATIC_VALU = 2041

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc is not installed")


def _registers(operands):
    """the vector registers an operand string names: v7 -> {7}, v[38:41] -> {38 .. 41}"""
    regs = set()
    for lo, hi in re.findall(r"\bv\[(\d+):(\d+)\]", operands):
        regs.update(range(int(lo), int(hi) + 1))
    regs.update(int(r) for r in re.findall(r"\bv(\d+)\b", operands))
    return regs


def test_lean_fastq_scan_hot_path(tmp_path):
    src = os.path.join(B.CSRC, "exg_fastq_fused.hip")
    asm = str(tmp_path / "exg_fastq_fused.s")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + B._flags() + B.FILE_FLAGS.get("exg_fastq_fused.hip", []) + [
        "--cuda-device-only", "-S", src, "-o", asm]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    m = re.search(r"^" + LEAN + r"\w*:[^\n]*\n(.*?)\.Lfunc_end", open(asm).read(), re.S | re.M)
    assert m, "the lean FASTQ scan is not in the assembly"
    ins = []  # (mnemonic, operands) of every instruction of the kernel, in program order
    for line in m.group(1).splitlines():
        line = line.split(";")[0].strip()
        if not line or line.startswith(".") or line.endswith(":"):
            continue
        parts = line.split(None, 1)
        ins.append((parts[0], parts[1] if len(parts) > 1 else ""))

    waits = [(i, int(re.search(r"vmcnt\((\d+)\)", ops).group(1))) for i, (op, ops) in enumerate(ins)
             if op == "s_waitcnt" and "vmcnt(" in ops]
    assert waits, "no vmcnt wait in the kernel"
    first_wait = waits[0][0]
    nt_loads = [(i, ops) for i, (op, ops) in enumerate(ins) if op == "global_load_dwordx4" and re.search(r"\bnt\b", ops)]
    ahead = [x for x in nt_loads if x[0] < first_wait]
    loaded = set()
    for _, ops in ahead:
        loaded |= _registers(ops.split(",")[0])
    countdown = [w for w in waits[:N_CHUNKS]]
    cndmask_on_loaded = [(i, ins[i]) for i in range(first_wait, countdown[-1][0]) if ins[i][0].startswith("v_cndmask")
                         and _registers(ins[i][1]) & loaded]
    static_valu = sum(1 for op, _ in ins if op.startswith("v_"))
    print(f"k_fused<FastqFormat, kLean>: {len(ahead)} of {len(nt_loads)} nt loads before the first vmcnt wait, waits "
          f"{[n for _, n in countdown]}, {countdown[-1][0] - first_wait} instructions from the first to the last of them, "
          f"{sum(1 for i in range(first_wait, countdown[-1][0]) if ins[i][0].startswith('v_'))} of them v_*, "
          f"v_cndmask on a loaded register among them: {len(cndmask_on_loaded)}; static v_* {static_valu} (before: {PARENT_STATIC_VALU}), "
          f"v_cndmask {sum(1 for op, _ in ins if op.startswith('v_cndmask'))}, s_cbranch {sum(1 for op, _ in ins if op.startswith('s_cbranch'))}")
    assert len(nt_loads) == N_CHUNKS and len(ahead) == N_CHUNKS, "the twelve input loads do not all precede the first vmcnt wait"
    assert len(loaded) == 4 * N_CHUNKS, "the twelve loads do not have 48 registers of their own"
    assert [n for _, n in countdown] == list(range(N_CHUNKS - 1, -1, -1)), "the waits do not count down 11 .. 0"
    assert not cndmask_on_loaded, f"v_cndmask on a loaded register inside the classification: {cndmask_on_loaded[:4]}"
    assert static_valu < PARENT_STATIC_VALU
