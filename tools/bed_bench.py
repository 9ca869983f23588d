#!/usr/bin/env python3
"""Rates of read_bed_file on one GPU, for three generated shapes: BED3 (~25-byte lines), BED6 (~45) and BED12 (~90).

  scan   exg_bed_scan alone (EXG_ALGO_FUSED_FULL, the single-pass scan) on text resident in HBM, timed with device events:
         all twelve columns, `start, end` only, and EXG_F_NO_STORE (tokenise + validate: COUNT(*)'s share); beside two
         yardsticks measured in the same run on the same device — the read-only stream rate (exg_count_newlines over the same
         buffer) and the any-shape VCF-8 scan (the same skeleton with fewer output columns); the general path
         (EXG_ALGO_MULTIPASS) for comparison
  file   a generated file (one block of lines repeated) through the reader to host DataChunks, PCIe inclusive: COUNT(*), all
         columns, and reference_sequence_name / start / end

    python tools/bed_bench.py [--scan-gb 1] [--file-gb 2] [--file-shape bed6] [--repeats 9] [--out profiles/bed_bench.json]

Prints one JSON document.  Rates are GB/s of input text (10^9)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (first: the library binds to torch's HIP runtime)

import bed_files as B  # noqa: E402
from exon_duckdb_amd import abi, device, load_library  # noqa: E402
from exon_duckdb_amd._lib import load_test_library  # noqa: E402
from exon_duckdb_amd.reader import ShardReader  # noqa: E402

SHAPES = {"bed3": (3,), "bed6": (6,), "bed12": (12,)}


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def timed(fn, n_bytes, repeats, warmup):
    ms = []
    for k in range(warmup + repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        if k >= warmup:
            ms.append(t0.elapsed_time(t1))
    return dict(spread(ms), **{"GB/s": n_bytes / statistics.median(ms) / 1e6})


def resident(block, target_bytes):
    """`block` repeated in HBM up to target_bytes -> (tensor, n_bytes, copies)"""
    times = max(1, target_bytes // len(block))
    n = times * len(block)
    d_block = device.upload(block, pad=0)[:len(block)]
    d_in = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    d_in[:n].copy_(d_block.repeat(times))
    return d_in, n, times


def bench_scan(block, target_bytes, repeats, warmup):
    lib = load_library()
    rows_block = len(B.read(block)[0])
    d_in, n, times = resident(block, target_bytes)
    rows = rows_block * times
    scan = device.BedScan(n, capacity_records=rows + 64)
    out = {"input_bytes": n, "rows": rows, "line_bytes_mean": len(block) / rows_block}
    modes = (("all_columns", abi.EXG_ALGO_FUSED_FULL, 0, None), ("start_end", abi.EXG_ALGO_FUSED_FULL, 0, [1, 2]),
             ("no_store", abi.EXG_ALGO_FUSED_FULL, abi.EXG_F_NO_STORE, None), ("general_path_all_columns", abi.EXG_ALGO_MULTIPASS, 0, None))
    for label, algo, extra, project in modes:
        flags = abi.EXG_F_BOF | abi.EXG_F_EOF | extra
        out[label] = timed(lambda: scan.launch(d_in, flags=flags, algo=algo, project=project), n, repeats, warmup)
        res = scan.fetch()
        assert res.error_code == 0 and res.n_records == rows and not (res.flags & abi.EXG_RF_CAPACITY), (label, res.n_records, res.error_code, res.flags)
    # yardstick 1: the read-only stream rate over the same buffer
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    out["stream_read_only"] = timed(lambda: device.check(lib.exg_count_newlines(C.c_void_p(d_in.data_ptr()), 0, n, C.c_void_p(d_count.data_ptr()), device.stream_ptr())),
                                    n, repeats, warmup)
    assert int(d_count.item()) == rows
    return out


def bench_vcf8(target_bytes, repeats, warmup):
    """yardstick 2: the any-shape VCF-8 scan, all columns"""
    n_lines = target_bytes // 52
    d_in, n = device.synth_vcf(n_lines)
    scan = device.VcfScan(n, capacity_records=n_lines + 64)
    header = bytes(d_in[:4096].cpu().numpy())
    lead = 0
    while header[lead:lead + 1] == b"#":
        lead = header.index(b"\n", lead) + 1
    out = timed(lambda: scan.launch(d_in, n_bytes=n, lead=lead, algo=abi.EXG_ALGO_FUSED_FULL), n, repeats, warmup)
    res = scan.fetch()
    assert res.error_code == 0 and res.n_records == n_lines, (res.n_records, res.error_code)
    return dict(out, input_bytes=n, rows=n_lines)


def bench_file(path, n_bytes, rows, repeats):
    tl = load_test_library()
    out = {"file_bytes": n_bytes, "rows": rows}

    def run(columns, count):
        ms = []
        for k in range(1 + repeats):        # (the first run warms the page cache and the pools)
            t0 = time.perf_counter()
            r = ShardReader(path, "bed", columns=columns, expect_chunks=not count)
            if count:
                got = r.count()
            else:
                n, chunks = C.c_uint64(0), C.c_uint64(0)
                rc = tl.exon_tf_drain_chunks(r._r, C.byref(n), C.byref(chunks))
                assert rc == 0, r._l.exg_reader_error(r._r)
                got = n.value
            st = r.stats()
            r.close()
            dt = (time.perf_counter() - t0) * 1e3
            assert got == rows, (got, rows)
            if k:
                ms.append(dt)
        return dict(spread(ms), **{"GB/s": n_bytes / statistics.median(ms) / 1e6, "host_vector_bytes": st["host_vector_bytes"]})
    out["count"] = run(None, True)
    out["all_columns"] = run(None, False)
    out["reference_start_end"] = run([0, 1, 2], False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scan-gb", type=float, default=1.0)
    ap.add_argument("--file-gb", type=float, default=2.0)
    ap.add_argument("--file-shape", default="bed6", choices=sorted(SHAPES))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    target = int(a.scan_gb * (1 << 30))
    result = {"device": torch.cuda.get_device_name(0), "scan": {}}
    blocks = {name: B.mixed(B.rng(21 + k), (4 << 20) // (25, 45, 90)[k], counts=counts) for k, (name, counts) in enumerate(SHAPES.items())}
    for name, block in blocks.items():
        result["scan"][name] = bench_scan(block, target, a.repeats, a.warmup)
        torch.cuda.empty_cache()
    result["scan"]["vcf8_any_shape_all_columns"] = bench_vcf8(target, a.repeats, a.warmup)
    torch.cuda.empty_cache()
    if a.file_gb > 0:
        block = blocks[a.file_shape]
        times = max(1, int(a.file_gb * 1e9) // len(block) + 1)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, a.file_shape + ".bed")
            with open(path, "wb") as f:
                for _ in range(times):
                    f.write(block)
            result["file"] = dict(bench_file(path, times * len(block), len(B.read(block)[0]) * times, max(3, a.repeats // 2)), shape=a.file_shape)
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
