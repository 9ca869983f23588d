#!/usr/bin/env python3
"""Rates of read_gtf on one GPU, on generated Ensembl-shaped lines (tests/gtf_files.py: ~300-byte lines, a `#!` line in 200).

  scan        exg_gtf_scan alone (EXG_ALGO_FUSED_FULL, the single-pass scan) on text resident in HBM, timed with device events:
              EXG_F_NO_STORE (tokenise + validate), `seqname, start, end`, and all nine columns (column 8: the raw ninth field);
              beside yardsticks measured in the same run on the same device — the read-only stream rate (exg_count_newlines over
              the same buffer) and exg_sam_scan on its own 150 bp lines
  attributes  exg_gtf_attributes alone over the scan's column 8 (count + prefix sums + emit), in GB/s of attribute text and
              entries/s (exg_cigar_op PARSE on rows of similar length is not measured here: tools/cigar_bench.py has its rates)
  file        a generated file (one block of lines repeated) through the reader to host DataChunks, PCIe inclusive: COUNT(*),
              `seqname, start, end`, and all columns

    python tools/gtf_bench.py [--scan-gb 1] [--file-gb 2] [--repeats 9] [--out profiles/gtf_bench.json]

Prints one JSON document.  Rates are GB/s (10^9) of input text unless a row says otherwise; every figure is the median of
`repeats` runs after `warmup` warm-ups, with its min and max beside it."""
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

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: the library binds to torch's HIP runtime)

import bam_files as BAM  # noqa: E402
import gtf_files as G  # noqa: E402
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


def gtf_block():
    rng = G.rng(41)
    text = b""
    while len(text) < BLOCK_BYTES:
        text += G.mixed(rng, 2000, comment_every=200)
    rows, keep, err = G.read(text, attributes=False)
    assert err is None
    return text, len(keep), len(rows), sum(len(r[8]) for r in rows), sum(len(G.parse_attributes(r[8])) for r in rows)


def bench_scan(text, lines_block, rows_block, attr_bytes_block, entries_block, target_bytes, repeats, warmup):
    lib = load_library()
    d_in, n, times = resident(text, target_bytes)
    lines, rows = lines_block * times, rows_block * times
    scan = device.GtfScan(n, capacity_records=lines + 64)
    out = {"input_bytes": n, "lines": lines, "rows": rows, "line_bytes_mean": len(text) / lines_block}
    modes = (("no_store", abi.EXG_ALGO_FUSED_FULL, abi.EXG_F_NO_STORE, None), ("seqname_start_end", abi.EXG_ALGO_FUSED_FULL, 0, [0, 3, 4]),
             ("general_path_all_columns", abi.EXG_ALGO_MULTIPASS, 0, None), ("all_columns", abi.EXG_ALGO_FUSED_FULL, 0, None))
    for label, algo, extra, project in modes:
        flags = abi.EXG_F_BOF | abi.EXG_F_EOF | extra
        out[label] = timed(lambda: scan.launch(d_in, flags=flags, algo=algo, project=project), n, repeats, warmup)
        res = scan.fetch()
        assert res.error_code == 0 and res.n_records == lines and not (res.flags & abi.EXG_RF_CAPACITY), (label, res.n_records, res.error_code, res.flags)
    out["all_columns"]["Mrows/s"] = rows / out["all_columns"]["median_ms"] / 1e3
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    out["stream_read_only"] = timed(lambda: device.check(lib.exg_count_newlines(C.c_void_p(d_in.data_ptr()), 0, n, C.c_void_p(d_count.data_ptr()), device.stream_ptr())),
                                    n, repeats, warmup)
    # exg_gtf_attributes over the column the last launch left (all columns), through the row map of the feature lines
    keep = torch.from_numpy(np.flatnonzero(scan.kept(lines)).astype(np.int32)).cuda()
    assert len(keep) == rows
    attr_bytes, entries = attr_bytes_block * times, entries_block * times
    cap = entries + 64
    # (the C entry with buffers made once: device.gtf_attributes allocates and zero-fills its outputs on every call)
    ws_bytes = int(lib.exg_gtf_attributes_workspace_bytes(rows))
    bufs = [torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device="cuda"), torch.empty(8, dtype=torch.int64, device="cuda"),
            torch.empty((rows, 2), dtype=torch.int64, device="cuda"), torch.empty((cap, 2), dtype=torch.int64, device="cuda"),
            torch.empty((cap, 2), dtype=torch.int64, device="cuda")]
    a = abi.GtfAttributesArgs()
    a.d_strings, a.d_payload, a.payload_base, a.d_row_map, a.n_rows = scan.cols[8].data_ptr(), d_in.data_ptr(), scan.PAYLOAD_BASE, keep.data_ptr(), rows
    a.d_workspace, a.workspace_bytes, a.d_result = bufs[0].data_ptr(), ws_bytes, bufs[1].data_ptr()
    a.d_out_entries, a.d_out_keys, a.d_out_values, a.entries_capacity = bufs[2].data_ptr(), bufs[3].data_ptr(), bufs[4].data_ptr(), cap
    a.stream = device.stream_ptr().value
    at = timed(lambda: device.check(lib.exg_gtf_attributes(C.byref(a))), attr_bytes, repeats, warmup)
    r = abi.GtfAttributesResult()
    device.check(lib.exg_gtf_attributes_result(C.c_void_p(bufs[1].data_ptr()), device.stream_ptr(), C.byref(r)))
    assert r.total_entries == entries and r.error_code == 0 and not r.flags, (r.total_entries, entries, r.flags)
    out["attributes"] = dict(at, attribute_bytes=attr_bytes, entries=entries, field_bytes_mean=attr_bytes / rows,
                             **{"Gentries/s": entries / at["median_ms"] / 1e6})
    return out


def bench_sam(target_bytes, repeats, warmup):
    """yardstick: exg_sam_scan on its own 150 bp lines, all columns"""
    recs = BAM.illumina_pairs(BLOCK_BYTES // 2 // 420, S.REFS, seed=31)
    rows = BAM.parse_decoded(BAM.header(S.REFS) + b"".join(recs)).rows
    lines = []
    for r in rows:
        mate = b"*" if r[7] is None else b"=" if r[7] == r[2] else r[7]
        lines.append(b"\t".join([r[0], b"%d" % r[1], r[2] or b"*", b"%d" % (r[3] or 0), r[5] or b"255", r[6] or b"*", mate, b"0", b"0", r[8] or b"*",
                                 r[9] or b"*", b"NM:i:1", b"MD:Z:150", b"RG:Z:grp1"]) + b"\n")
    text = b"".join(lines)
    d_in, n, times = resident(text, target_bytes)
    scan = device.SamScan(n, capacity_records=len(rows) * times + 64)
    out = timed(lambda: scan.launch(d_in, algo=abi.EXG_ALGO_FUSED_FULL), n, repeats, warmup)
    res = scan.fetch()
    assert res.error_code == 0 and res.n_records == len(rows) * times
    return dict(out, input_bytes=n, rows=len(rows) * times)


def bench_file(path, n_bytes, rows, repeats):
    tl = load_test_library()
    out = {"file_bytes": n_bytes, "rows": rows}

    def run(columns, count):
        ms = []
        for k in range(1 + repeats):        # (the first run warms the page cache and the pools)
            t0 = time.perf_counter()
            r = ShardReader(path, "gtf", columns=columns, expect_chunks=not count)
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
    out["seqname_start_end"] = run([0, 3, 4], False)
    out["all_columns"] = run(None, False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scan-gb", type=float, default=1.0)
    ap.add_argument("--file-gb", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    target = int(a.scan_gb * (1 << 30))
    result = {"device": torch.cuda.get_device_name(0)}
    text, lines, rows, attr_bytes, entries = gtf_block()
    result["scan"] = bench_scan(text, lines, rows, attr_bytes, entries, target, a.repeats, a.warmup)
    torch.cuda.empty_cache()
    result["sam_scan_150bp_all_columns"] = bench_sam(target, a.repeats, a.warmup)
    torch.cuda.empty_cache()
    if a.file_gb > 0:
        times = max(1, int(a.file_gb * 1e9) // len(text) + 1)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "genes.gtf")
            with open(path, "wb") as f:
                for _ in range(times):
                    f.write(text)
            result["file"] = bench_file(path, times * len(text), rows * times, max(3, a.repeats // 2))
    out = json.dumps(result, indent=1)
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
