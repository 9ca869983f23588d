#!/usr/bin/env python3
"""Rates of read_bam_file_records on one GPU, for two shapes of input: 150 bp paired reads and 15 kb long reads.

  scan   exg_bam_scan alone on decoded records resident in HBM (record discovery + validation + all ten columns into device
         buffers; the call synchronises, so wall time around it is device time + two host round trips): warm-up, then
         repeats — median, min and max; also with EXG_F_NO_STORE (discovery + validation only: COUNT(*)'s share)
  file   a generated BAM file (one pre-compressed run of whole records repeated, tests/bam_files.py: seconds to write)
         through the reader, PCIe inclusive: COUNT(*), all columns into chunks, and name / flag / start alone

    python tools/bam_bench.py [--scan-gb 1] [--file-gb 4] [--repeats 7] [--out profiles/bam_bench.json]

Prints one JSON document.  Rates are GB/s of DECODED bytes (10^9)."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (first: the library binds to torch's HIP runtime)

import bam_files as B  # noqa: E402
from exon_duckdb_amd import abi, device  # noqa: E402
from exon_duckdb_amd._lib import load_test_library  # noqa: E402
from exon_duckdb_amd.reader import ShardReader  # noqa: E402

REFS = [(b"chr%d" % i, 250_000_000) for i in range(1, 23)] + [(b"chrX", 156_000_000), (b"chrY", 57_000_000)]


def long_reads(n, length, seed=1):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        ln = int(length * rng.uniform(0.5, 1.5))
        ops, left = [], ln
        while left > 0:                     # a long-read CIGAR: a match run, then an indel, a few hundred operations a read
            m = min(left, rng.randrange(20, 120))
            ops.append((m, "M"))
            left -= m
            if left > 0:
                ops.append((rng.randrange(1, 4), "D"))
        out.append(B.record(b"m64011_190830_220126/%d/ccs" % rng.randrange(10 ** 8), 0 if i & 1 else 16, rng.randrange(len(REFS)), rng.randrange(10 ** 8),
                            60, ops, -1, -1, 0, rng.randbytes(ln).translate(B._TO_BASES), rng.randbytes(ln).translate(B._TO_QUAL),
                            B.aux_z(b"RG", b"movie1") + b"NMi" + (ln // 50).to_bytes(4, "little")))
    return out


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def bench_scan(run, target_bytes, repeats, warmup):
    times = max(1, target_bytes // len(run))
    n = times * len(run)
    d_run = device.upload(run, pad=0)[:len(run)]
    d_in = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    d_in[:n].copy_(d_run.repeat(times))
    rows_run = len(B.parse_decoded(B.header(REFS) + run).rows)
    scan = device.BamScan(n, REFS, capacity_records=rows_run * times + 64, side_capacity=2 * n + 64)
    out = {"decoded_bytes": n, "rows": rows_run * times}
    for label, flags in (("all_columns", abi.EXG_F_EOF), ("no_store", abi.EXG_F_EOF | abi.EXG_F_NO_STORE)):
        ms = []
        for k in range(warmup + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scan.launch(d_in, flags=flags)
            dt = (time.perf_counter() - t0) * 1e3
            if k >= warmup:
                ms.append(dt)
        res = scan.fetch()
        assert res.error_code == 0 and res.n_records == out["rows"] and not (res.flags & abi.EXG_RF_CAPACITY), (res.n_records, res.error_code, res.flags)
        out[label] = dict(spread(ms), **{"GB/s": n / statistics.median(ms) / 1e6})
        out["tiles"], out["tiles_rewalked"], out["side_bytes"] = res.tiles, res.tiles_rewalked, max(res.side_bytes, out.get("side_bytes", 0))
    return out


def bench_file(path, decoded, rows, repeats):
    tl = load_test_library()
    out = {"decoded_bytes": decoded, "file_bytes": os.path.getsize(path), "rows": rows}

    def run(columns, count):
        ms = []
        for k in range(1 + repeats):        # (the first run warms the page cache and the pools)
            t0 = time.perf_counter()
            r = ShardReader(path, "bam", columns=columns, expect_chunks=not count)
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
        return dict(spread(ms), **{"GB/s": decoded / statistics.median(ms) / 1e6, "host_vector_bytes": st["host_vector_bytes"],
                                   "tiles": st["bam_tiles"], "tiles_rewalked": st["bam_tiles_rewalked"]})
    out["count"] = run(None, True)
    out["all_columns"] = run(None, False)
    out["name_flag_start"] = run([0, 1, 3], False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scan-gb", type=float, default=1.0)
    ap.add_argument("--file-gb", type=float, default=4.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = {"reads_150bp": b"".join(B.illumina_pairs(12_000, REFS, seed=1)), "reads_15kb": b"".join(long_reads(400, 15_000))}
    result = {"device": torch.cuda.get_device_name(0), "tile_bytes": 32768}
    with tempfile.TemporaryDirectory() as tmp:
        for name, run in shapes.items():
            entry = {"record_bytes_mean": len(run) / len(B.parse_decoded(B.header(REFS) + run).rows)}
            entry["scan"] = bench_scan(run, int(a.scan_gb * (1 << 30)), a.repeats, a.warmup)
            if a.file_gb > 0:
                path = os.path.join(tmp, name + ".bam")
                times = max(1, int(a.file_gb * 1e9) // len(run) + 1)
                decoded = B.write_repeated(path, B.header(REFS), run, times)
                entry["file"] = bench_file(path, decoded, len(B.parse_decoded(B.header(REFS) + run).rows) * times, max(3, a.repeats // 2))
                os.remove(path)
            result[name] = entry
            torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
