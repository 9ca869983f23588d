#!/usr/bin/env python3
"""Rates of read_sam_file_records on one GPU, for two generated shapes: 150 bp pairs (the records of
bam_files.illumina_pairs as text, ~400-byte lines) and 15 kb long reads (~30 kB lines, every one of them k_line_far's).

  scan   exg_sam_scan alone (EXG_ALGO_FUSED_FULL, the single-pass scan) on text resident in HBM, timed with device events:
         all ten columns, `name, flag, start` only, and EXG_F_NO_STORE (tokenise + validate: COUNT(*)'s share); the general path
         (EXG_ALGO_MULTIPASS) for comparison; beside three yardsticks measured in the same run on the same device — the
         read-only stream rate (exg_count_newlines over the same buffer), the any-shape VCF-8 scan (the same skeleton) and
         exg_bam_scan over the same records in BAM's packing
  file   a generated file (a header and one block of lines repeated) through the reader to host DataChunks, PCIe inclusive:
         COUNT(*), `name, flag, start`, and all columns

    python tools/sam_bench.py [--scan-gb 1] [--file-gb 2] [--file-shape pairs150] [--repeats 9] [--out profiles/sam_bench.json]

Prints one JSON document.  Rates are GB/s of input text (10^9); BAM's are GB/s of decoded BAM bytes, with the rows beside them."""
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

import bam_files as BAM  # noqa: E402
import sam_files as S  # noqa: E402
from exon_duckdb_amd import abi, device, load_library  # noqa: E402
from exon_duckdb_amd._lib import load_test_library  # noqa: E402
from exon_duckdb_amd.reader import ShardReader  # noqa: E402

BLOCK_BYTES = 4 << 20


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


def as_text(records, aux):
    """packed BAM records -> the lines `samtools view` prints for them (columns from the independent BAM reader; PNEXT / TLEN,
    which no column shows, are 0)"""
    rows = BAM.parse_decoded(BAM.header(S.REFS) + b"".join(records)).rows
    out = []
    for r in rows:
        mate = b"*" if r[7] is None else b"=" if r[7] == r[2] else r[7]
        f = [r[0], b"%d" % r[1], r[2] or b"*", b"%d" % (r[3] or 0), r[5] or b"255", r[6] or b"*", mate, b"0", b"0", r[8] or b"*", r[9] or b"*"]
        out.append(b"\t".join(f + aux) + b"\n")
    return b"".join(out), rows


def shape_blocks():
    """{shape: (SAM text block, BAM record block, rows)} of about BLOCK_BYTES of text each"""
    pairs = BAM.illumina_pairs(BLOCK_BYTES // 2 // 420, S.REFS, seed=31)
    rng = random.Random(32)
    long_reads = []
    for i in range(BLOCK_BYTES // 30100):
        n = 15000
        seq = rng.randbytes(n).translate(BAM._TO_BASES)
        long_reads.append(BAM.record(b"m64011_%d/%d/ccs" % (rng.randrange(10 ** 6), i), 0 if i % 2 else 16, rng.randrange(len(S.REFS)), rng.randrange(10 ** 8), 60,
                                     [(n - 200, "M"), (100, "I"), (50, "D"), (100, "S")], seq=seq, qual=rng.randbytes(n).translate(BAM._TO_QUAL)))
    out = {}
    for name, recs, aux in (("pairs150", pairs, [b"NM:i:1", b"MD:Z:150", b"RG:Z:grp1"]), ("long15k", long_reads, [b"NM:i:150", b"RG:Z:hifi"])):
        text, rows = as_text(recs, aux)
        assert S.read(text) == (rows, None)
        out[name] = (text, b"".join(recs), len(rows))
    return out


def bench_scan(text, bam, rows_block, target_bytes, repeats, warmup):
    lib = load_library()
    d_in, n, times = resident(text, target_bytes)
    rows = rows_block * times
    scan = device.SamScan(n, capacity_records=rows + 64)
    out = {"input_bytes": n, "rows": rows, "line_bytes_mean": len(text) / rows_block}
    modes = (("all_columns", abi.EXG_ALGO_FUSED_FULL, 0, None), ("name_flag_start", abi.EXG_ALGO_FUSED_FULL, 0, [0, 1, 3]),
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
    del scan, d_in
    torch.cuda.empty_cache()
    # yardstick 3: exg_bam_scan over the same records (its bytes are BAM's: the rows are what compares)
    d_bam, nb, times_b = resident(bam, len(bam) * times)
    assert times_b == times
    bscan = device.BamScan(nb, S.REFS, capacity_records=rows + 64)
    out["bam_scan_same_records"] = dict(timed(lambda: bscan.launch(d_bam, flags=abi.EXG_F_EOF), nb, repeats, warmup), input_bytes=nb)
    res = bscan.fetch()
    assert res.error_code == 0 and res.n_records == rows, (res.n_records, res.error_code)
    for label in ("all_columns", "bam_scan_same_records"):
        out[label]["Mrows/s"] = rows / out[label]["median_ms"] / 1e3
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
            r = ShardReader(path, "sam", columns=columns, expect_chunks=not count)
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
    out["name_flag_start"] = run([0, 1, 3], False)
    out["all_columns"] = run(None, False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scan-gb", type=float, default=1.0)
    ap.add_argument("--file-gb", type=float, default=2.0)
    ap.add_argument("--file-shape", default="pairs150", choices=["pairs150", "long15k"])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    target = int(a.scan_gb * (1 << 30))
    result = {"device": torch.cuda.get_device_name(0), "scan": {}}
    blocks = shape_blocks()
    for name, (text, bam, rows) in blocks.items():
        result["scan"][name] = bench_scan(text, bam, rows, target, a.repeats, a.warmup)
        torch.cuda.empty_cache()
    result["scan"]["vcf8_any_shape_all_columns"] = bench_vcf8(target, a.repeats, a.warmup)
    torch.cuda.empty_cache()
    if a.file_gb > 0:
        text, _, rows = blocks[a.file_shape]
        times = max(1, int(a.file_gb * 1e9) // len(text) + 1)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, a.file_shape + ".sam")
            head = S.header()
            with open(path, "wb") as f:
                f.write(head)
                for _ in range(times):
                    f.write(text)
            result["file"] = dict(bench_file(path, len(head) + times * len(text), rows * times, max(3, a.repeats // 2)), shape=a.file_shape)
    out = json.dumps(result, indent=1)
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
