#!/usr/bin/env python3
"""Rates of the CIGAR scalars (exg_cigar_op: parse_cigar, extract_from_cigar) on one GPU, in one run on one device:

  yardstick  the read-only stream rate (exg_count_newlines) over the buffer the CIGAR text lies in
  short      both ops on the `cigar` (and `sequence`) column exg_sam_scan leaves for --lines alignment lines of 150 bp with
             mixed CIGARs: 60 % `150M`, 25 % of the `75M2I73M` kind (inlined), 15 % of 13 bytes and more (out of line)
  long       both ops on a column of --long-rows rows of --long-mb MB of CIGAR text each (about 3.9 bytes an operation)
  host       the host scalar loop of the DuckDB shim (parse_cigar) on one core over both inputs

    python tools/cigar_bench.py [--lines 2000000] [--long-rows 16] [--long-mb 4] [--repeats 9] [--warmup 3] [--out FILE]

Prints one JSON document.  Rates are GB/s of CIGAR text (10^9; what the op parses) and operations per second, with the
fraction of the yardstick measured on the same buffer in the same run, the bytes the op moves (columns read, children written),
the per-byte time of the long shape against the short one, and the device against sixteen host cores (the one-core time / 16)."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: the library binds to torch's HIP runtime)

from exon_duckdb_amd import abi, device, load_library  # noqa: E402
from exon_duckdb_amd._lib import load_test_library  # noqa: E402

BASE, SEQ_BASE = 1 << 40, 1 << 41
LETTERS = b"MIDNSHP=X"


def timed(fn, repeats, warmup):
    ms = []
    for k in range(warmup + repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        if k >= warmup:
            ms.append(t0.elapsed_time(t1))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


class Op:
    """one op with its buffers allocated once: launch() only enqueues"""

    def __init__(self, op, cigar, sequence, n_rows, payload_bytes, ops_capacity=0):
        self.lib = load_library()
        parse = op == abi.EXG_CIGAR_PARSE
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")      # noqa: E731
        self.entries = new((n_rows if parse else 1, 2), torch.int64)
        self.out_op = new((max(ops_capacity, 1), 2), torch.int64)
        self.out_len = new(max(ops_capacity, 1), torch.int32)
        self.start, self.end = new(1 if parse else n_rows, torch.int32), new(1 if parse else n_rows, torch.int32)
        self.slices = new((1 if parse else n_rows, 2), torch.int64)
        ws_bytes = int(self.lib.exg_cigar_workspace_bytes(op, n_rows, payload_bytes))
        self.ws = new(ws_bytes // 8 + 1, torch.int64)
        self.d_result = torch.zeros(8, dtype=torch.int64, device="cuda")
        a = self.args = abi.CigarOpArgs()
        a.op, a.n_rows = op, n_rows
        a.d_cigar, a.d_cigar_payload, a.cigar_payload_base = cigar[0].data_ptr(), cigar[1].data_ptr(), cigar[2]
        if parse:
            a.d_out_entries, a.ops_capacity = self.entries.data_ptr(), ops_capacity
            if ops_capacity:
                a.d_out_op, a.d_out_len = self.out_op.data_ptr(), self.out_len.data_ptr()
        else:
            a.d_sequence, a.d_sequence_payload, a.sequence_payload_base = sequence[0].data_ptr(), sequence[1].data_ptr(), sequence[2]
            a.d_out_start, a.d_out_end, a.d_out_sequence = self.start.data_ptr(), self.end.data_ptr(), self.slices.data_ptr()
        a.d_workspace, a.workspace_bytes, a.d_result = self.ws.data_ptr(), ws_bytes, self.d_result.data_ptr()
        a.stream = device.stream_ptr().value

    def launch(self):
        device.check(self.lib.exg_cigar_op(C.byref(self.args)))

    def result(self):
        r = abi.CigarResult()
        device.check(self.lib.exg_cigar_result(C.c_void_p(self.d_result.data_ptr()), device.stream_ptr(), C.byref(r)))
        return r


def stream_rate(d_buf, n, repeats, warmup):
    lib = load_library()
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    t = timed(lambda: device.check(lib.exg_count_newlines(C.c_void_p(d_buf.data_ptr()), 0, n, C.c_void_p(d_count.data_ptr()), device.stream_ptr())),
              repeats, warmup)
    return dict(t, bytes=n, **{"GB/s": n / t["median_ms"] / 1e6})


def bench_column(cigar, sequence, n_rows, cigar_bytes, long_bytes, repeats, warmup):
    """both ops on one column; cigar_bytes: all CIGAR text, long_bytes: that of the rows of 13 bytes and more"""
    count = Op(abi.EXG_CIGAR_PARSE, cigar, None, n_rows, long_bytes)
    count.launch()
    total = int(count.result().total_ops)
    out = {"rows": n_rows, "cigar_bytes": cigar_bytes, "out_of_line_cigar_bytes": long_bytes, "operations": total}
    for name, op in (("parse_cigar", abi.EXG_CIGAR_PARSE), ("extract_from_cigar", abi.EXG_CIGAR_EXTRACT)):
        run = Op(op, cigar, sequence, n_rows, long_bytes, total)
        t = timed(run.launch, repeats, warmup)
        r = run.result()
        assert r.error_code == 0 and r.flags == 0, (name, r.error_code, r.flags)
        moved = 16 * n_rows + long_bytes + (16 * n_rows + 20 * total if op == abi.EXG_CIGAR_PARSE else 16 * n_rows + 24 * n_rows)
        t.update({"GB/s": cigar_bytes / t["median_ms"] / 1e6, "moved_bytes": moved, "moved_GB/s": moved / t["median_ms"] / 1e6})
        if op == abi.EXG_CIGAR_PARSE:
            t["Gops/s"] = total / t["median_ms"] / 1e6
        out[name] = t
        del run
        torch.cuda.empty_cache()
    if n_rows:
        t = timed(count.launch, repeats, warmup)          # the counting call of the two-call protocol
        out["parse_cigar_counting_call"] = dict(t, **{"GB/s": cigar_bytes / t["median_ms"] / 1e6})
    return out


def bench_host(cigars, repeats):
    """exon_scan::ParseCigar over `cigars` (list of bytes) in one call, on one core"""
    tl = load_test_library()
    data = b"".join(cigars)
    off = np.zeros(len(cigars) + 1, np.uint64)
    off[1:] = np.cumsum(np.fromiter((len(s) for s in cigars), np.uint64, len(cigars)))
    total, len_sum = C.c_uint64(0), C.c_uint64(0)
    ms = []
    for k in range(1 + repeats):
        t0 = time.perf_counter()
        rc = tl.exon_tf_parse_cigar_batch(data, off.ctypes.data, len(cigars), C.byref(total), C.byref(len_sum))
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0
        if k:
            ms.append(dt)
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "n": len(ms), "cigar_bytes": len(data), "operations": int(total.value),
            "GB/s": len(data) / med / 1e6, "Gops/s": total.value / med / 1e6}


def short_cigar(rng):
    shape = rng.random()
    if shape < 0.60:
        return b"150M"
    if shape < 0.85:
        a = rng.randrange(20, 120)
        k = rng.randrange(1, 4)
        return rng.choice((b"%dM%dI%dM" % (a, k, 150 - a - k), b"%dM%dD%dM" % (a, k, 150 - a), b"%dS%dM" % (k, 150 - k)))
    a, b = rng.randrange(5, 30), rng.randrange(10, 50)
    return b"%dS%dM1I%dM2D%dM%dH" % (a, b, rng.randrange(5, 40), 150 - a - b - 1 - 30, rng.randrange(1, 50))


def sam_lines(n_lines, seed=7, distinct=4096):
    """n_lines alignment lines of 150 bp drawn from `distinct` different ones -> (text, the lines' cigars in order)"""
    rng = random.Random(seed)
    pool = []
    for _ in range(distinct):
        seq = bytes(rng.choice(b"ACGT") for _ in range(150))
        cigar = short_cigar(rng)
        pool.append((b"\t".join([b"A00%03d:%d:HXX:%d" % (rng.randrange(1000), rng.randrange(400), rng.randrange(10 ** 6)), b"%d" % rng.randrange(4096),
                                 b"chr%d" % rng.randrange(1, 23), b"%d" % rng.randrange(1, 10 ** 8), b"60", cigar, b"=", b"%d" % rng.randrange(1, 10 ** 8),
                                 b"%d" % rng.randrange(-500, 500), seq, bytes(rng.randrange(35, 75) for _ in range(150))]) + b"\n", cigar))
    pick = np.random.default_rng(seed).integers(0, distinct, n_lines).tolist()
    return b"".join(pool[i][0] for i in pick), [pool[i][1] for i in pick]


def long_rows(n_rows, row_bytes, seed=9, blocks=32, block_ops=4000):
    """rows of about row_bytes of CIGAR text: blocks of block_ops random operations (lengths 1..999) in random order"""
    rng = random.Random(seed)
    pool = [b"".join(b"%d%c" % (rng.randrange(1, 1000), rng.choice(LETTERS)) for _ in range(block_ops)) for _ in range(blocks)]
    rows = []
    for _ in range(n_rows):
        parts, n = [], 0
        while n < row_bytes:
            parts.append(rng.choice(pool))
            n += len(parts[-1])
        rows.append(b"".join(parts))
    return rows


def column_of(rows, base):
    """string_t rows pointing into one payload buffer, one row behind the other -> (d_col, d_payload, base)"""
    col = np.zeros((len(rows), 16), np.uint8)
    at = 0
    for r, s in enumerate(rows):
        assert len(s) > 12
        col[r, :4] = np.frombuffer(np.uint32(len(s)).tobytes(), np.uint8)
        col[r, 4:8] = np.frombuffer(s[:4], np.uint8)
        col[r, 8:16] = np.frombuffer(np.uint64(base + at).tobytes(), np.uint8)
        at += len(s)
    return torch.from_numpy(col).cuda(), device.upload(b"".join(rows)), base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=2_000_000)
    ap.add_argument("--long-rows", type=int, default=16)
    ap.add_argument("--long-mb", type=float, default=4.0)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "unit": "GB/s of CIGAR text (10^9); Gops/s = 10^9 operations a second"}

    # short rows: the cigar and sequence columns of a SAM scan
    text, cigars = sam_lines(a.lines)
    d_text = device.upload(text)
    scan = device.SamScan(len(text), capacity_records=a.lines + 64)
    scan.launch(d_text, payload_base=BASE)
    res = scan.fetch()
    assert res.error_code == 0 and res.n_records == a.lines, (res.n_records, res.error_code)
    cigar_bytes, out_of_line = sum(map(len, cigars)), sum(len(s) for s in cigars if len(s) > 12)
    short = {"text_bytes": len(text), "stream_read_only_text": stream_rate(d_text, len(text), a.repeats, a.warmup)}
    short.update(bench_column((scan.cols[6], d_text, BASE), (scan.cols[8], d_text, BASE), a.lines, cigar_bytes, out_of_line, a.repeats, a.warmup))
    result["short_rows_sam150"] = short
    host_short = bench_host(cigars, max(3, a.repeats // 3))
    del scan, d_text, text, cigars
    torch.cuda.empty_cache()

    # long rows: a few rows of MBs of CIGAR text in one payload buffer, and a sequence of 10 kb for each
    rows = long_rows(a.long_rows, int(a.long_mb * 1e6))
    n = sum(map(len, rows))
    cigar = column_of(rows, BASE)
    sequence = column_of([bytes(b"ACGT"[(r + k) & 3] for k in range(10000)) for r in range(a.long_rows)], SEQ_BASE)
    long = {"stream_read_only": stream_rate(cigar[1], n, a.repeats, a.warmup)}
    long.update(bench_column(cigar, sequence, a.long_rows, n, n, a.repeats, a.warmup))
    result["long_rows"] = long
    host_long = bench_host(rows[:2], max(3, a.repeats // 3))
    result["host_scalar_loop_one_core"] = {"short_rows_sam150": host_short, "long_rows": host_long}

    summary = {}
    for name in ("parse_cigar", "extract_from_cigar"):
        s, l = short[name], long[name]
        summary[name] = {"short_GB/s": s["GB/s"], "long_GB/s": l["GB/s"],
                         "short_fraction_of_stream": s["GB/s"] / short["stream_read_only_text"]["GB/s"],
                         "long_fraction_of_stream": l["GB/s"] / long["stream_read_only"]["GB/s"],
                         "short_moved_fraction_of_stream": s["moved_GB/s"] / short["stream_read_only_text"]["GB/s"],
                         "long_moved_fraction_of_stream": l["moved_GB/s"] / long["stream_read_only"]["GB/s"],
                         "long_over_short_time_per_byte": (l["median_ms"] / n) / (s["median_ms"] / cigar_bytes)}
    p = summary["parse_cigar"]
    p.update({"short_Gops/s": short["parse_cigar"]["Gops/s"], "long_Gops/s": long["parse_cigar"]["Gops/s"],
              "short_device_over_16_host_cores": short["parse_cigar"]["GB/s"] / (16 * host_short["GB/s"]),
              "long_device_over_16_host_cores": long["parse_cigar"]["GB/s"] / (16 * host_long["GB/s"])})
    result["summary"] = summary
    out = json.dumps(result, indent=1)
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
