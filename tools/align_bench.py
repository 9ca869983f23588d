#!/usr/bin/env python3
"""Rates of the alignment scores (exg_align_score) on one GPU beside the host scalar on one core, in one run:

  reads   the `sequence` column exg_fastq_scan leaves for synthetic FASTQ-150 (--pairs records) against a mutated copy of it
          at about 1 % and about 5 % divergence (four fifths substitutions, one tenth deleted and one tenth inserted bases)
  long    --long-pairs pairs of --long-bp bases at about 1 %
  host    exon_scan::AlignmentScore (what the DuckDB shim registers) on one core over the first --host-reads / --host-long pairs
          of the same columns; its scores are compared with the device's, bit for bit

    python tools/align_bench.py [--pairs 3000000] [--long-pairs 1000] [--long-bp 15000] [--repeats 9] [--warmup 3] [--out FILE]

Prints one JSON document: pairs/s as the median of --repeats launches after --warmup, with the spread (min, max), for 16, 32
and 64 lanes a pair, and the device's rate over 16 times the one-core host rate (sixteen cores with no loss)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: the library binds to torch's HIP runtime)

from exon_duckdb_amd import abi, device, load_library  # noqa: E402
from exon_duckdb_amd._lib import load_test_library  # noqa: E402

BASE_T, BASE_P = 1 << 40, 1 << 41
PARAMS = (4, 6, 2)


def mutated_copy(rows, divergence, seed):
    """rows: uint8 [n, L] on the device -> (payload uint8, offsets int64 [n + 1]): every base substituted with probability
    0.8 d, deleted with 0.1 d, followed by an inserted random base with 0.1 d"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    n, L = rows.shape
    flat = rows.reshape(-1)
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    r = torch.rand(flat.shape, device="cuda", generator=g)
    code = (flat.to(torch.int64) >> 1) & 3                      # A 0, C 1, T 2, G 3
    other = torch.tensor(list(b"ACTG"), dtype=torch.uint8, device="cuda")[(code + 1 + torch.randint(0, 3, flat.shape, device="cuda", generator=g)) % 4]
    flat = torch.where(r < 0.8 * divergence, other, flat)
    counts = torch.ones(flat.shape, dtype=torch.int64, device="cuda")
    counts[(r >= 0.8 * divergence) & (r < 0.9 * divergence)] = 0
    counts[(r >= 0.9 * divergence) & (r < divergence)] = 2
    ends = torch.cumsum(counts, 0)
    out = torch.repeat_interleave(flat, counts)
    second = (ends - 1)[counts == 2]
    out[second] = letters[torch.randint(0, 4, second.shape, device="cuda", generator=g)]
    offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    offsets[1:] = ends.reshape(n, L)[:, -1]
    return torch.cat([out, torch.zeros(64, dtype=torch.uint8, device="cuda")]), offsets


def column_of(payload, offsets, base):
    """string_t [n, 2] int64 for rows payload[offsets[i] .. offsets[i + 1]) (every row longer than 12 bytes)"""
    lens = offsets[1:] - offsets[:-1]
    assert int(lens.min()) > 12
    idx = offsets[:-1, None] + torch.arange(4, device="cuda")[None, :]
    prefix = (payload[idx].to(torch.int64) << (8 * torch.arange(4, device="cuda"))[None, :]).sum(1)
    col = torch.empty((len(lens), 2), dtype=torch.int64, device="cuda")
    col[:, 0] = lens | (prefix << 32)
    col[:, 1] = base + offsets[:-1]
    return col


class Op:
    """one exg_align_score call with its buffers allocated once: launch() only enqueues"""

    def __init__(self, text, d_tpay, pattern, d_ppay, n, max_pair_bytes, lanes):
        self.lib = load_library()
        self.out = torch.empty(max(n, 1), dtype=torch.float32, device="cuda")
        ws_bytes = int(self.lib.exg_align_workspace_bytes(n, max_pair_bytes, *PARAMS))
        self.ws = torch.empty(ws_bytes // 8 + 2, dtype=torch.int64, device="cuda")
        self.d_result = torch.zeros(8, dtype=torch.int64, device="cuda")
        a = self.args = abi.AlignScoreArgs()
        a.d_text, a.d_text_payload, a.text_payload_base = text.data_ptr(), d_tpay.data_ptr(), BASE_T
        a.d_pattern, a.d_pattern_payload, a.pattern_payload_base = pattern.data_ptr(), d_ppay.data_ptr(), BASE_P
        a.n_rows, a.max_pair_bytes, a.lanes = n, max_pair_bytes, lanes
        a.mismatch, a.gap_opening, a.gap_extension = PARAMS
        a.d_out_float = self.out.data_ptr()
        a.d_workspace, a.workspace_bytes, a.d_result = self.ws.data_ptr(), ws_bytes, self.d_result.data_ptr()
        a.stream = device.stream_ptr().value

    def launch(self):
        device.check(self.lib.exg_align_score(C.byref(self.args)))

    def result(self):
        r = abi.AlignScoreResult()
        device.check(self.lib.exg_align_result(C.c_void_p(self.d_result.data_ptr()), device.stream_ptr(), C.byref(r)))
        return r


def timed(fn, n_pairs, repeats, warmup):
    ms = []
    for k in range(warmup + repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        if k >= warmup:
            ms.append(t0.elapsed_time(t1))
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "n": len(ms), "pairs/s": n_pairs / med * 1e3,
            "pairs/s_min": n_pairs / max(ms) * 1e3, "pairs/s_max": n_pairs / min(ms) * 1e3}


def host_rows(col, payload, base, k):
    """the first k rows of a string_t column as (bytes, offsets uint64 [k + 1]) on the host"""
    c = col[:k].cpu().numpy()
    lens, ptrs = c[:, 0] & 0xFFFFFFFF, c[:, 1] - base
    lo, hi = int(ptrs.min()), int((ptrs + lens).max())
    data = payload[lo:hi].cpu().numpy()
    parts = [data[p - lo:p - lo + n].tobytes() for p, n in zip(ptrs, lens)]
    off = np.zeros(k + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return b"".join(parts), off


def bench_case(name, text, d_tpay, pattern, d_ppay, n, max_pair_bytes, host_pairs, repeats, warmup):
    case = {"pairs": n, "max_pair_bytes": max_pair_bytes, "device": {}}
    scores = None
    for lanes in (16, 32, 64):
        op = Op(text, d_tpay, pattern, d_ppay, n, max_pair_bytes, lanes)
        case["device"][f"lanes_{lanes}"] = timed(op.launch, n, repeats, warmup)
        r = op.result()
        case["device"][f"lanes_{lanes}"].update(n_global=int(r.n_global), n_capped=int(r.n_capped), flags=int(r.flags))
        got = op.out[:host_pairs].cpu().numpy()
        assert scores is None or np.array_equal(scores, got), "the lane widths disagree"
        scores = got
        case["mean_penalty"] = float(-op.out.double().mean())
        del op
        torch.cuda.empty_cache()
    tl = load_test_library()
    k = min(host_pairs, n)
    t_bytes, t_off = host_rows(text, d_tpay, BASE_T, k)
    p_bytes, p_off = host_rows(pattern, d_ppay, BASE_P, k)
    out = np.zeros(k, np.float32)
    ms = []
    for rep in range(4):
        t0 = time.perf_counter()
        rc = tl.exon_tf_alignment_score_batch(t_bytes, t_off.ctypes.data, p_bytes, p_off.ctypes.data, k, *PARAMS, out.ctypes.data)
        ms.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0
    assert np.array_equal(out.view(np.uint32), scores[:k].view(np.uint32)), "device and host scalar disagree"
    med = statistics.median(ms[1:])
    case["host_one_core"] = {"pairs": k, "median_ms": med, "min_ms": min(ms[1:]), "max_ms": max(ms[1:]), "pairs/s": k / med * 1e3}
    best = max(v["pairs/s"] for v in case["device"].values())
    case["device_over_16_host_cores"] = best / (16 * case["host_one_core"]["pairs/s"])
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"))
    a = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "parameters": {"mismatch": 4, "gap_opening": 6, "gap_extension": 2},
              "unit": "pairs/s: median of %d launches after %d warm-ups; _min / _max: the slowest and the fastest launch" % (a.repeats, a.warmup)}

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
        payload, offsets = mutated_copy(rows, d, seed=int(d * 1000))
        pattern = column_of(payload, offsets, BASE_P)
        longest = 150 + int((offsets[1:] - offsets[:-1]).max())
        result[label] = bench_case(label, text, d_in, pattern, payload, a.pairs, longest, a.host_reads, a.repeats, a.warmup)
        result[label]["divergence"] = d
        del payload, offsets, pattern
        torch.cuda.empty_cache()
    del scan, d_in, rows, text
    torch.cuda.empty_cache()

    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    rows = letters[torch.randint(0, 4, (a.long_pairs, a.long_bp), device="cuda")]
    t_pay = torch.cat([rows.reshape(-1), torch.zeros(64, dtype=torch.uint8, device="cuda")])
    t_off = torch.arange(a.long_pairs + 1, device="cuda", dtype=torch.int64) * a.long_bp
    text = column_of(t_pay, t_off, BASE_T)
    payload, offsets = mutated_copy(rows, 0.01, seed=7)
    pattern = column_of(payload, offsets, BASE_P)
    longest = a.long_bp + int((offsets[1:] - offsets[:-1]).max())
    label = "long_%dbp_1pct" % a.long_bp
    result[label] = bench_case(label, text, t_pay, pattern, payload, a.long_pairs, longest, a.host_long, a.repeats, a.warmup)
    result[label]["divergence"] = 0.01

    out = json.dumps(result, indent=1)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
