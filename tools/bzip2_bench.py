#!/usr/bin/env python3
"""bzip2 measurement: ~1 GB of synthetic FASTQ-150 (oracle.synth_fastq) compressed at level 9 with Python's bz2, then

  * exg_bzip2_decode GB/s of decoded output, the compressed bytes resident in HBM (best of --reps after a warm call);
  * reader COUNT(*) and all columns into DataChunks (ShardReader.digest, checked against the plain file's digest) GB/s of
    decoded FASTQ, the .bz2 in the page cache;
  * libbz2 single-core GB/s (bz2.decompress of the file's first stream, in this process).

One JSON line on stdout.  The file is compressed once, in 64 MiB pieces on 16 processes (each piece a stream of its own, as
pbzip2 writes them: the decoder reads every concatenated stream), and kept under --cache.

    python tools/bzip2_bench.py [--gb 1.0] [--reps 3] [--decode-only]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bzip2_bench.py --decode-only   # per-stage kernel times
"""
import argparse
import bz2
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PIECE = 64 << 20


def _compress(piece):
    return bz2.compress(piece, 9)


def make_input(gb, cache):
    from oracle import pyoracle
    pyoracle.lib()
    os.makedirs(cache, exist_ok=True)
    plain = os.path.join(cache, f"synth_{gb:g}.fastq")
    comp = plain + ".bz2"
    if not (os.path.exists(plain) and os.path.exists(comp)):
        data = bytes(pyoracle.synth_fastq(int(gb * 1e9) // 332 * 332))  # (whole 332-byte records)
        with open(plain, "wb") as f:
            f.write(data)
        with ProcessPoolExecutor(16) as ex:
            parts = list(ex.map(_compress, [data[i:i + PIECE] for i in range(0, len(data), PIECE)]))
        with open(comp + ".tmp", "wb") as f:
            for p in parts:
                f.write(p)
        os.replace(comp + ".tmp", comp)
    return plain, comp


def decode_rate(comp_bytes, reps):
    import torch
    from exon_duckdb_amd import device, load_library
    lib = load_library()
    d = device.upload(comp_bytes)
    out, produced = C.c_void_p(), C.c_uint64(0)
    best, n = None, 0
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.exg_bzip2_decode(C.c_void_p(d.data_ptr()), len(comp_bytes), C.byref(out), C.byref(produced), device.stream_ptr())
        dt = time.perf_counter() - t0
        if rc != 0:
            raise RuntimeError(lib.exg_last_error_message().decode())
        n = produced.value
        lib.exg_free_device(out, n + 64)
        if i and (best is None or dt < best):
            best = dt
    return n, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cache", default=os.environ.get("EXG_BENCH_CACHE", "/tmp/exg_bzip2_bench"))
    ap.add_argument("--decode-only", action="store_true")
    a = ap.parse_args()
    plain, comp = make_input(a.gb, a.cache)
    comp_bytes = open(comp, "rb").read()
    n_out, t_dec = decode_rate(comp_bytes, a.reps)
    res = {"bench": "bzip2", "fastq_bytes": os.path.getsize(plain), "bz2_bytes": len(comp_bytes), "decoded": n_out,
           "exg_bzip2_decode_gbps": round(n_out / t_dec / 1e9, 3)}
    if not a.decode_only:
        from exon_duckdb_amd.reader import ShardReader
        best_c = best_d = None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = ShardReader(comp, "fastq", compression="bzip2")
            rows = r.count()
            r.close()
            dt = time.perf_counter() - t0
            best_c = dt if best_c is None or dt < best_c else best_c
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = ShardReader(comp, "fastq", compression="bzip2", expect_chunks=True)
            dig = r.digest()
            r.close()
            dt = time.perf_counter() - t0
            best_d = dt if best_d is None or dt < best_d else best_d
        r = ShardReader(plain, "fastq")
        want = r.digest()
        r.close()
        assert dig == want and dig[0] == rows, (dig, want, rows)
        # libbz2, one core, this process: the file's first stream (64 MiB of FASTQ)
        first = bz2.BZ2Decompressor()
        t0 = time.perf_counter()
        got = first.decompress(comp_bytes)
        t_lib = time.perf_counter() - t0
        lib_gbps = len(got) / t_lib / 1e9
        res.update({"rows": rows, "reader_count_gbps": round(n_out / best_c / 1e9, 3), "reader_datachunks_gbps": round(n_out / best_d / 1e9, 3),
                    "libbz2_single_core_gbps": round(lib_gbps, 4), "count_vs_16_libbz2_cores": round(n_out / best_c / 1e9 / (16 * lib_gbps), 2)})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
