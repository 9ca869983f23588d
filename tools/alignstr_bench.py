#!/usr/bin/env python3
"""The alignment strings (exg_align_string) beside the alignment scores (exg_align_score) on the same pairs in the same run, on
one GPU, with the inputs of tools/align_bench.py:

  reads   the `sequence` column exg_fastq_scan leaves for synthetic FASTQ-150 (--pairs records) against a mutated copy of it
          at about 1 % and about 5 % divergence
  long    --long-pairs pairs of --long-bp bases at about 1 %, with a max_penalty that fits: the largest penalty the score op
          found, times 1.25, rounded up to a multiple of 256 (no row is capped; the workspace grows with its square)
  host    exon_scan::AlignmentString on one core over the first --host-reads / --host-long pairs; its CIGARs are compared
          with the device's, byte for byte

    python tools/alignstr_bench.py [--pairs 3000000] [--long-pairs 1000] [--long-bp 15000] [--repeats 9] [--warmup 3] [--out FILE]

Each figure is the median of --repeats launches after --warmup, with the spread.  Writes profiles/alignstr_bench.json: the
string op's time, its ratio to the score op (both at 64 lanes a pair, the default of both) and the workspace it took.  The
backtrace runs inside the alignment kernel, so its share is not a kernel's time; what the placement kernels (scan, k_place,
k_finish) take is in a kernel trace of this script."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: the library binds to torch's HIP runtime)

import align_bench as AB  # noqa: E402
from exon_duckdb_amd import abi, device, load_library  # noqa: E402
from exon_duckdb_amd._lib import load_test_library  # noqa: E402

BASE_T, BASE_P, PARAMS = AB.BASE_T, AB.BASE_P, AB.PARAMS
OUT_BASE = device.ALIGN_OUT_BASE


class StringOp:
    """one exg_align_string call with its buffers allocated once: launch() only enqueues"""

    def __init__(self, text, d_tpay, pattern, d_ppay, n, max_pair_bytes, max_penalty, out_capacity, lanes=0):
        self.lib = load_library()
        self.strings = torch.empty((max(n, 1), 2), dtype=torch.int64, device="cuda")
        self.payload = torch.empty(max(out_capacity, 16), dtype=torch.uint8, device="cuda")
        self.ws_bytes = int(self.lib.exg_align_string_workspace_bytes(n, max_pair_bytes, *PARAMS, max_penalty, out_capacity))
        assert self.ws_bytes, "the workspace function refused the arguments"
        self.ws = torch.empty(self.ws_bytes // 8 + 2, dtype=torch.int64, device="cuda")
        self.d_result = torch.zeros(8, dtype=torch.int64, device="cuda")
        a = self.args = abi.AlignStringArgs()
        a.d_text, a.d_text_payload, a.text_payload_base = text.data_ptr(), d_tpay.data_ptr(), BASE_T
        a.d_pattern, a.d_pattern_payload, a.pattern_payload_base = pattern.data_ptr(), d_ppay.data_ptr(), BASE_P
        a.n_rows, a.max_pair_bytes, a.max_penalty, a.lanes = n, max_pair_bytes, max_penalty, lanes
        a.mismatch, a.gap_opening, a.gap_extension = PARAMS
        a.d_out_strings, a.d_out_payload, a.out_capacity, a.out_payload_base = self.strings.data_ptr(), self.payload.data_ptr(), out_capacity, OUT_BASE
        a.d_workspace, a.workspace_bytes, a.d_result = self.ws.data_ptr(), self.ws_bytes, self.d_result.data_ptr()
        a.stream = device.stream_ptr().value

    def launch(self):
        device.check(self.lib.exg_align_string(C.byref(self.args)))

    def result(self):
        r = abi.AlignStringResult()
        device.check(self.lib.exg_align_string_result(C.c_void_p(self.d_result.data_ptr()), device.stream_ptr(), C.byref(r)))
        return r

    def rows(self, k):
        """the first k CIGARs as bytes"""
        c = self.strings[:k].cpu().numpy()
        raw = c.view(np.uint8).reshape(k, 16)
        lens = (c[:, 0] & 0xFFFFFFFF).astype(np.int64)
        longs = lens > 12
        data = b""
        lo = 0
        if longs.any():
            ptrs = c[:, 1][longs] - OUT_BASE
            lo, hi = int(ptrs.min()), int((ptrs + lens[longs]).max())
            data = self.payload[lo:hi].cpu().numpy().tobytes()
        return [data[int(c[i, 1]) - OUT_BASE - lo:int(c[i, 1]) - OUT_BASE - lo + int(lens[i])] if longs[i] else raw[i, 4:4 + int(lens[i])].tobytes()
                for i in range(k)]


def bench_case(text, d_tpay, pattern, d_ppay, n, max_pair_bytes, host_pairs, repeats, warmup, cap_from_scores):
    case = {"pairs": n, "max_pair_bytes": max_pair_bytes}
    score = AB.Op(text, d_tpay, pattern, d_ppay, n, max_pair_bytes, 64)
    case["score_op"] = AB.timed(score.launch, n, repeats, warmup)
    pens = -score.out.double()
    case["mean_penalty"], case["max_penalty_seen"] = float(pens.mean()), int(pens.max())
    max_penalty = (int(case["max_penalty_seen"] * 1.25) + 255) // 256 * 256 if cap_from_scores else 0
    total = int(((text[:n, 0] & 0xFFFFFFFF) + (pattern[:n, 0] & 0xFFFFFFFF)).sum())
    op = StringOp(text, d_tpay, pattern, d_ppay, n, max_pair_bytes, max_penalty, 2 * total)
    case["string_op"] = AB.timed(op.launch, n, repeats, warmup)
    r = op.result()
    assert (r.flags, r.error_code, r.n_capped) == (0, 0, 0), (r.flags, r.error_code, r.n_capped)
    case["string_op"].update(max_penalty=max_penalty, workspace_bytes=op.ws_bytes, out_capacity=2 * total, out_bytes=int(r.out_bytes),
                             n_global=int(r.n_global), lanes=64)
    case["string_over_score"] = case["string_op"]["median_ms"] / case["score_op"]["median_ms"]
    k = min(host_pairs, n)
    got = op.rows(k)
    t_bytes, t_off = AB.host_rows(text, d_tpay, BASE_T, k)
    p_bytes, p_off = AB.host_rows(pattern, d_ppay, BASE_P, k)
    cap = 2 * (len(t_bytes) + len(p_bytes)) + 16
    out, out_off = np.zeros(cap, np.uint8), np.zeros(k + 1, np.uint64)
    ms = []
    for rep in range(3):
        t0 = time.perf_counter()
        rc = load_test_library().exon_tf_alignment_string_batch(t_bytes, t_off.ctypes.data, p_bytes, p_off.ctypes.data, k, *PARAMS, out.ctypes.data,
                                                                cap, out_off.ctypes.data)
        ms.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0
    host = [out[int(out_off[i]):int(out_off[i + 1])].tobytes() for i in range(k)]
    assert host == got, "device and host scalar disagree"
    med = statistics.median(ms[1:])
    case["host_one_core"] = {"pairs": k, "median_ms": med, "pairs/s": k / med * 1e3}
    case["device_over_16_host_cores"] = case["string_op"]["pairs/s"] / (16 * case["host_one_core"]["pairs/s"])
    case["device_and_host_agree_on"] = k
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3_000_000)
    ap.add_argument("--long-pairs", type=int, default=1000)
    ap.add_argument("--long-bp", type=int, default=15000)
    ap.add_argument("--host-reads", type=int, default=100_000)
    ap.add_argument("--host-long", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alignstr_bench.json"))
    a = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "parameters": {"mismatch": 4, "gap_opening": 6, "gap_extension": 2},
              "unit": "median of %d launches after %d warm-ups; _min / _max: the slowest and the fastest launch" % (a.repeats, a.warmup)}

    n_text = a.pairs * abi.EXG_SYNTH_FASTQ_RECORD_BYTES
    d_in = device.synth_fastq(n_text)
    scan = device.FastqScan(n_text, capacity_records=a.pairs + 64)
    scan.launch(d_in, payload_base=BASE_T)
    res = scan.fetch()
    assert res.error_code == 0 and res.n_records == a.pairs, (res.n_records, res.error_code)
    text = scan.cols[2]
    starts = text[:a.pairs, 1] - BASE_T
    rows = torch.empty((a.pairs, 150), dtype=torch.uint8, device="cuda")
    step = 1 << 20
    for at in range(0, a.pairs, step):
        rows[at:at + step] = d_in[starts[at:at + step, None] + torch.arange(150, device="cuda")[None, :]]
    for label, d in (("reads_150bp_1pct", 0.01), ("reads_150bp_5pct", 0.05)):
        payload, offsets = AB.mutated_copy(rows, d, seed=int(d * 1000))
        pattern = AB.column_of(payload, offsets, BASE_P)
        longest = 150 + int((offsets[1:] - offsets[:-1]).max())
        result[label] = bench_case(text, d_in, pattern, payload, a.pairs, longest, a.host_reads, a.repeats, a.warmup, False)
        result[label]["divergence"] = d
        del payload, offsets, pattern
        torch.cuda.empty_cache()
    del scan, d_in, rows, text
    torch.cuda.empty_cache()

    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    rows = letters[torch.randint(0, 4, (a.long_pairs, a.long_bp), device="cuda")]
    t_pay = torch.cat([rows.reshape(-1), torch.zeros(64, dtype=torch.uint8, device="cuda")])
    t_off = torch.arange(a.long_pairs + 1, device="cuda", dtype=torch.int64) * a.long_bp
    text = AB.column_of(t_pay, t_off, BASE_T)
    payload, offsets = AB.mutated_copy(rows, 0.01, seed=7)
    pattern = AB.column_of(payload, offsets, BASE_P)
    longest = a.long_bp + int((offsets[1:] - offsets[:-1]).max())
    label = "long_%dbp_1pct" % a.long_bp
    result[label] = bench_case(text, t_pay, pattern, payload, a.long_pairs, longest, a.host_long, a.repeats, a.warmup, True)
    result[label]["divergence"] = 0.01

    out = json.dumps(result, indent=1)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
