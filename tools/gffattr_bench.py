#!/usr/bin/env python3
"""Rate of exg_gff_attributes (gff_parse_attributes on a column that is still in HBM) on one GPU, beside two yardsticks taken in
the same run on the same device:

  gff_attributes   count + prefix sums + emit over generated NCBI-shaped ninth fields
                   (`ID=...;Parent=...;Dbxref=...;gbkey=...;gene=...;product=...`: about 130 bytes and six entries a row), the text
                   resident in HBM as one payload and a string_t column that points into it; also the counting call alone
  gtf_attributes   exg_gtf_attributes over tests/gtf_files.py's Ensembl-shaped ninth fields, the same number of bytes
  stream_read_only exg_count_newlines over the GFF payload: what reading the bytes once costs

    python tools/gffattr_bench.py [--gb 0.77] [--repeats 9] [--warmup 3] [--out profiles/gffattr_bench.json]

Prints one JSON document.  Rates are GB/s (10^9) of attribute text; every figure is the median of `repeats` runs after `warmup`
warm-ups on device events, with its min and max beside it.  A measurement, not a gate: nothing here asserts a rate."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: the library binds to torch's HIP runtime)

import gff_attr_ref as R  # noqa: E402
import gtf_files as G  # noqa: E402
from exon_duckdb_amd import abi, device, load_library  # noqa: E402

BLOCK_ROWS = 32768
BASE = 1 << 44


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


def ncbi_fields(n, seed=17):
    """ninth fields as NCBI's GFF3 writes them for a CDS: six entries, about 130 bytes"""
    rng = random.Random(seed)
    products = [b"hypothetical protein", b"DNA-directed RNA polymerase subunit beta", b"ATP synthase F0 sector subunit c", b"50S ribosomal protein L7/L12",
                b"transcriptional regulator%2C LysR family", b"ABC transporter permease"]
    out = []
    for _ in range(n):
        k = rng.randrange(10 ** 6)
        out.append(b"ID=cds-NP_%06d.1;Parent=rna-NM_%06d.%d;Dbxref=GeneID:%d,Genbank:NP_%06d.1;gbkey=CDS;gene=%s%d;product=%s" % (
            k, rng.randrange(10 ** 6), rng.randrange(1, 9), rng.randrange(10 ** 7), k, rng.choice([b"rpo", b"atp", b"LOC", b"abc"]), rng.randrange(999),
            rng.choice(products)))
    return out


def gtf_fields(n, seed=41):
    rng = G.rng(seed)
    return [G.attributes(rng) for _ in range(n)]


def resident_column(fields, target_bytes):
    """the block of fields repeated in HBM up to target_bytes -> (string_t column [rows, 2] int64, payload tensor, rows, bytes, copies)"""
    assert all(len(f) > 12 for f in fields)
    block = b"".join(fields)
    lens = np.array([len(f) for f in fields], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    prefix = np.array([int.from_bytes(f[:4], "little") for f in fields], dtype=np.int64)
    times = max(1, target_bytes // len(block))
    n_bytes, rows = times * len(block), times * len(fields)
    d_block = device.upload(block, pad=0)[:len(block)]
    payload = torch.zeros(n_bytes + 64, dtype=torch.uint8, device="cuda")
    payload[:n_bytes].copy_(d_block.repeat(times))
    col = torch.empty((times, len(fields), 2), dtype=torch.int64, device="cuda")
    col[:, :, 0] = torch.from_numpy(lens | (prefix << 32)).cuda()
    col[:, :, 1] = torch.from_numpy(offs + BASE).cuda()[None, :] + (torch.arange(times, dtype=torch.int64, device="cuda") * len(block))[:, None]
    return col.reshape(rows, 2).contiguous(), payload, rows, n_bytes, times


def bench_op(name, fields, entries_block, target_bytes, repeats, warmup):
    """exg_<name>_attributes with buffers made once (device.*_attributes allocates and zero-fills its outputs on every call)"""
    lib = load_library()
    col, payload, rows, n_bytes, times = resident_column(fields, target_bytes)
    entries = entries_block * times
    cap = entries + 64
    ws_bytes = int(getattr(lib, f"exg_{name}_attributes_workspace_bytes")(rows))
    bufs = [torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device="cuda"), torch.empty(8, dtype=torch.int64, device="cuda"),
            torch.empty((rows, 2), dtype=torch.int64, device="cuda"), torch.empty((cap, 2), dtype=torch.int64, device="cuda"),
            torch.empty((cap, 2), dtype=torch.int64, device="cuda")]
    a = (abi.GffAttributesArgs if name == "gff" else abi.GtfAttributesArgs)()
    a.d_strings, a.d_payload, a.payload_base, a.n_rows = col.data_ptr(), payload.data_ptr(), BASE, rows
    a.d_workspace, a.workspace_bytes, a.d_result = bufs[0].data_ptr(), ws_bytes, bufs[1].data_ptr()
    a.stream = device.stream_ptr().value
    op, fetch = getattr(lib, f"exg_{name}_attributes"), getattr(lib, f"exg_{name}_attributes_result")
    r = (abi.GffAttributesResult if name == "gff" else abi.GtfAttributesResult)()
    counting = timed(lambda: device.check(op(C.byref(a))), n_bytes, repeats, warmup)
    device.check(fetch(C.c_void_p(bufs[1].data_ptr()), device.stream_ptr(), C.byref(r)))
    assert r.total_entries == entries and r.error_code == 0, (r.total_entries, entries, r.error_code)
    a.d_out_entries, a.d_out_keys, a.d_out_values, a.entries_capacity = bufs[2].data_ptr(), bufs[3].data_ptr(), bufs[4].data_ptr(), cap
    full = timed(lambda: device.check(op(C.byref(a))), n_bytes, repeats, warmup)
    device.check(fetch(C.c_void_p(bufs[1].data_ptr()), device.stream_ptr(), C.byref(r)))
    assert r.total_entries == entries and r.error_code == 0 and not r.flags, (r.total_entries, entries, r.flags)
    out = dict(full, attribute_bytes=n_bytes, rows=rows, entries=entries, field_bytes_mean=n_bytes / rows, entries_per_row=entries / rows,
               **{"Gentries/s": entries / full["median_ms"] / 1e6, "Mrows/s": rows / full["median_ms"] / 1e3})
    out["counting_call"] = counting
    stream = None
    if name == "gff":
        d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
        stream = timed(lambda: device.check(lib.exg_count_newlines(C.c_void_p(payload.data_ptr()), 0, n_bytes, C.c_void_p(d_count.data_ptr()), device.stream_ptr())),
                       n_bytes, repeats, warmup)
    return out, stream


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=0.77)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    target = int(a.gb * 1e9)
    result = {"device": torch.cuda.get_device_name(0)}
    gff = ncbi_fields(BLOCK_ROWS)
    result["gff_attributes"], result["stream_read_only"] = bench_op("gff", gff, sum(len(R.spans(f)) for f in gff), target, a.repeats, a.warmup)
    torch.cuda.empty_cache()
    gtf = gtf_fields(BLOCK_ROWS // 2)
    result["gtf_attributes"], _ = bench_op("gtf", gtf, sum(len(G.parse_attributes(f)) for f in gtf), target, a.repeats, a.warmup)
    result["gff_over_gtf_per_byte"] = result["gff_attributes"]["GB/s"] / result["gtf_attributes"]["GB/s"]
    result["gff_over_stream"] = result["gff_attributes"]["GB/s"] / result["stream_read_only"]["GB/s"]
    out = json.dumps(result, indent=1)
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
