#!/usr/bin/env python3
"""Rates of read_bcf_file_records on one GPU, for three shapes of record: sites (no samples), 100 samples and 2 504 samples.

  transcoder  exg_bcf_to_vcf alone on decoded records resident in HBM (discovery, count, scan, emit; the call synchronises, so
              wall time around it is device time + a host round trip): GB/s of BCF in and of text out, beside the read-only
              stream rate (exg_count_newlines) over the text the same call wrote
  file        a generated BCF file (one pre-compressed run of whole records repeated: records are position independent)
              through the reader, PCIe inclusive: COUNT(*), `chrom, pos, ref`, all columns — and THE SAME RECORDS as bgzip'd VCF
              through read_vcf in the same run, with the ratio of the two (rows per second: BCF inflates fewer bytes)

    python tools/bcf_bench.py [--scan-gb 1] [--file-gb 1] [--repeats 7] [--out profiles/bcf_bench.json]

Prints one JSON document.  Rates are GB/s (10^9)."""
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
import bcf_files as B  # noqa: E402
from exon_duckdb_amd import abi, device, load_library  # noqa: E402
from exon_duckdb_amd._lib import load_test_library  # noqa: E402
from exon_duckdb_amd.reader import ShardReader  # noqa: E402

INFOS = [("DP", "1", "Integer"), ("AF", "A", "Float"), ("DB", "0", "Flag"), ("AC", "A", "Integer"), ("AN", "1", "Integer"), ("MQ", "1", "Float")]
FORMATS = [("GT", "1", "String"), ("GQ", "1", "Integer"), ("DP", "1", "Integer"), ("PL", "G", "Integer")]


def records(text, n, n_sample, seed):
    rng = random.Random(seed)
    k = {name.decode(): i for i, name in enumerate(B.dictionaries(text)[0]) if name}
    out = []
    for i in range(n):
        n_alt = rng.choice((1, 1, 1, 2))
        info = [(k["DP"], B.ints([rng.randrange(20000)])), (k["AF"], B.floats([rng.random() for _ in range(n_alt)])),
                (k["AC"], B.ints([rng.randrange(5000) for _ in range(n_alt)])), (k["AN"], B.ints([5008])), (k["MQ"], B.floats([rng.random() * 60]))]
        if i % 3 == 0:
            info.append((k["DB"], B.flag()))
        fmt = ()
        if n_sample:
            fmt = [(k["GT"], [B.ints(rng.choice(([2, 2], [2, 4], [4, 4], [2, 5]))) for _ in range(n_sample)]),
                   (k["GQ"], [B.ints([rng.randrange(100)], width=1) for _ in range(n_sample)]),
                   (k["DP"], [B.ints([rng.randrange(60)], width=1) for _ in range(n_sample)]),
                   (k["PL"], [B.ints([0, rng.randrange(255), rng.randrange(2000)], width=2) for _ in range(n_sample)])]
        out.append(B.record(chrom=i % 24, pos=1000 + 37 * i, id_=b"rs%d" % rng.randrange(10 ** 8) if i % 2 else b"", qual=rng.random() * 1000,
                            alleles=[rng.choice((b"A", b"C", b"GT"))] + [rng.choice((b"G", b"T", b"<DEL>")) for _ in range(n_alt)],
                            filters=[0] if i % 4 else None, info=info, fmt=fmt, n_sample=n_sample))
    return out


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def timed(fn, repeats, warmup):
    ms = []
    for k in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def bench_transcoder(text, run, rows_run, text_run, target_bytes, repeats, warmup):
    lib = load_library()
    strings, contigs, n_samples = B.dictionaries(text)
    times = max(1, target_bytes // len(run))
    n = times * len(run)
    d_run = device.upload(run, pad=0)[:len(run)]
    d_in = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    d_in[:n].copy_(d_run.repeat(times))
    t = device.BcfToVcf(n, strings, contigs, n_samples, output_capacity=int(text_run * times * 1.05) + 4096)
    ms = timed(lambda: t.launch(d_in), repeats, warmup)
    res = t.launch(d_in)
    assert res.error_code == 0 and res.n_records == rows_run * times and res.flags == 0, (res.n_records, res.error_code, res.flags)
    med = statistics.median(ms)
    out = dict(spread(ms), bcf_bytes=n, text_bytes=res.text_bytes, rows=res.n_records, tiles_rewalked=res.tiles_rewalked)
    out["GB/s_bcf_in"], out["GB/s_text_out"] = n / med / 1e6, res.text_bytes / med / 1e6
    d_count = torch.zeros(8, dtype=torch.int64, device="cuda")
    padded = (res.text_bytes + 15) // 16 * 16
    sm = timed(lambda: device.check(lib.exg_count_newlines(C.c_void_p(t.out.data_ptr()), 0, min(padded, t.output_capacity) // 16 * 16, C.c_void_p(d_count.data_ptr()),
                                                            device.stream_ptr())), repeats, warmup)
    out["stream_read_only_of_the_text"] = dict(spread(sm), **{"GB/s": res.text_bytes / statistics.median(sm) / 1e6})
    return out


def bench_file(path, fmt, rows, repeats, sizes):
    tl = load_test_library()

    def run(columns, count):
        ms = []
        for k in range(1 + repeats):        # (the first run warms the page cache and the pools)
            t0 = time.perf_counter()
            r = ShardReader(path, fmt, columns=columns, expect_chunks=not count)
            if count:
                got = r.count()
            else:
                n, chunks = C.c_uint64(0), C.c_uint64(0)
                rc = tl.exon_tf_drain_chunks(r._r, C.byref(n), C.byref(chunks))
                assert rc == 0, r._l.exg_reader_error(r._r)
                got = n.value
            r.close()
            dt = (time.perf_counter() - t0) * 1e3
            assert got == rows, (got, rows)
            if k:
                ms.append(dt)
        med = statistics.median(ms)
        return dict(spread(ms), **{"Mrows/s": rows / med / 1e3, "GB/s_of_text": sizes["text_bytes"] / med / 1e6})
    return dict(sizes, file_bytes=os.path.getsize(path), rows=rows, count=run(None, True), chrom_pos_ref=run([0, 1, 3], False), all_columns=run(None, False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scan-gb", type=float, default=1.0)
    ap.add_argument("--file-gb", type=float, default=1.0, help="text bytes of the generated file, 10^9")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "tile_bytes": 32768}
    with tempfile.TemporaryDirectory() as tmp:
        for name, n_sample, n_rec in (("sites", 0, 30_000), ("samples_100", 100, 1_500), ("samples_2504", 2504, 60)):
            text = B.header_text(contigs=tuple(f"chr{i}" for i in range(1, 25)), infos=INFOS, formats=FORMATS, samples=tuple(f"S{i}" for i in range(n_sample)), idx=True)
            recs = records(text, n_rec, n_sample, seed=n_sample + 1)
            run = b"".join(recs)
            strings, contigs, ns = B.dictionaries(text)
            lines = B.Rendered(run, strings, contigs, ns).text
            entry = {"record_bytes_mean": len(run) / n_rec, "line_bytes_mean": len(lines) / n_rec}
            entry["transcoder"] = bench_transcoder(text, run, n_rec, len(lines), int(a.scan_gb * (1 << 30)), a.repeats, a.warmup)
            if a.file_gb > 0 and name != "samples_2504":
                times = max(1, int(a.file_gb * 1e9) // len(lines) + 1)
                sizes = {"text_bytes": len(lines) * times, "bcf_bytes": len(run) * times}
                bcf, vcf = os.path.join(tmp, name + ".bcf"), os.path.join(tmp, name + ".vcf.gz")
                BAM.write_repeated(bcf, B.file_header(text), run, times)
                BAM.write_repeated(vcf, text, lines, times)
                reps = max(3, a.repeats // 2)
                entry["file_bcf"] = bench_file(bcf, "bcf", n_rec * times, reps, sizes)
                entry["file_same_records_as_bgzip_vcf"] = bench_file(vcf, "vcf", n_rec * times, reps, sizes)
                entry["bcf_over_vcf_rows_per_second"] = {q: entry["file_bcf"][q]["Mrows/s"] / entry["file_same_records_as_bgzip_vcf"][q]["Mrows/s"]
                                                         for q in ("count", "chrom_pos_ref", "all_columns")}
                os.remove(bcf), os.remove(vcf)
            result[name] = entry
            torch.cuda.empty_cache()
    out = json.dumps(result, indent=1)
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
