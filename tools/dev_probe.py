"""Dev probes (GPU box): MALL residency of a re-read stream; cost split of the fused kernel (EXG_CXXFLAGS=-DEXG_DEV_PROBE).
    python tools/dev_probe.py [--gb 4] [--hist] [--launches N]
--hist      one more run of the full kernel with flags bit 12: the wait histogram of wait_prefix (exg_fused_core.hpp note_wait)
--launches  only N launches of the full kernel (what a counter pass of rocprofv3 is run over)"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from exon_duckdb_amd import abi, device, load_library

lib = load_library()
torch.cuda.set_device(0)


def time_ms(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    evs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    t = sorted(x.elapsed_time(y) for x, y in evs)
    return t[len(t) // 2]


ap = argparse.ArgumentParser()
ap.add_argument("--gb", type=float, default=4.0)
ap.add_argument("--hist", action="store_true")
ap.add_argument("--launches", type=int, default=0)
opt = ap.parse_args()
out = {}
n = int(opt.gb * 10**9)
d_in = device.synth_fastq(n)
if opt.launches:
    scan = device.FastqScan(n, capacity_records=n // 332 + 16)
    for _ in range(opt.launches):
        scan.launch(d_in, n_bytes=n, flags=abi.EXG_F_BOF | abi.EXG_F_EOF, algo=abi.EXG_ALGO_FUSED)
    r = scan.fetch()
    print(f"{opt.launches} launches: n_records={r.n_records} err={r.error_code} flags={r.flags}")
    sys.exit(0)
cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
# 1. streaming count of the same X bytes, back to back: does the second pass come from the Infinity Cache?
for mb in (int(opt.gb * 1000),):
    x = mb * 10**6 // 16 * 16
    ms = time_ms(lambda: lib.exg_count_newlines(C.c_void_p(d_in.data_ptr()), 0, x, C.c_void_p(cnt.data_ptr()),
                                                device.stream_ptr()), reps=20, warm=3)
    out[f"count_rereads_{mb}MB_GBps"] = x / ms / 1e6
print(json.dumps(out, indent=1))

# 2. fused kernel with dev modes (flags bits 8..): see exg_fastq_fused.hip
scan = device.FastqScan(n, capacity_records=n // 332 + 16)
for mode in (0, 1, 2, 3, 4):
    fl = abi.EXG_F_BOF | abi.EXG_F_EOF
    os.environ["EXG_FASTQ_DEV_MODE"] = str(mode)  # (read by run_fastq_fused at every launch; the C ABI refuses unknown flag bits)
    ms = time_ms(lambda: scan.launch(d_in, n_bytes=n, flags=fl, algo=abi.EXG_ALGO_FUSED), reps=10, warm=2)
    r = scan.fetch()
    print(f"fused dev_mode={mode}: {ms:.3f} ms  {n / ms / 1e6:.0f} GB/s  n_records={r.n_records} err={r.error_code} flags={r.flags}")


if opt.hist:
    # flags bit 12: every workgroup of the lean scan leaves its wait in the FarRec of its half 0 (exg_fused_core.hpp): 10 ns ticks
    # wave 0 stood in wait_prefix, ticks from the count's publish to the prefix, polls looked at.  Workspace layout: exg_fastq_ws.hpp
    import numpy as np
    os.environ["EXG_FASTQ_DEV_MODE"] = "16"
    fl = abi.EXG_F_BOF | abi.EXG_F_EOF
    ms = time_ms(lambda: scan.launch(d_in, n_bytes=n, flags=fl, algo=abi.EXG_ALGO_FUSED), reps=10, warm=2)
    scan.fetch()
    up = lambda v, a: (v + a - 1) // a * a
    n_mp = (n + 16383) // 16384 + 1
    off_desc = up(up(256 + n_mp * 4, 256) + n_mp * 8, 256)
    n_fused = ((n + 16383) // 16384 + 5) & ~3
    n_super = (n + 49151) // 49152
    far = scan.ws.view(torch.int32)[(off_desc + n_fused * 48) // 4:][: n_super * 3 * 8].cpu().numpy().reshape(n_super, 3, 8)[1:, 0, :3]
    wait_us, lat_us, polls = far[:, 0] / 100.0, far[:, 1] / 100.0, far[:, 2]
    edges = [0, 0.5, 1, 1.5, 2, 3, 4, 5, 6, 8, 12, 16, 1e9]
    hist = lambda x: {f"<{e}" if e < 1e9 else ">=16": int(c) for e, c in zip(edges[1:], np.histogram(x, bins=edges)[0])}
    print(json.dumps({"ms_per_launch_with_wait_records": round(ms, 3), "waits": int(len(far)),
                      "wait_us": {"mean": round(float(wait_us.mean()), 3), "median": round(float(np.median(wait_us)), 3),
                                  "p90": round(float(np.percentile(wait_us, 90)), 3), "hist": hist(wait_us)},
                      "publish_to_prefix_us": {"mean": round(float(lat_us.mean()), 3), "median": round(float(np.median(lat_us)), 3),
                                               "p90": round(float(np.percentile(lat_us, 90)), 3), "hist": hist(lat_us)},
                      "polls_per_wait": round(float(polls.mean()), 3)}))
