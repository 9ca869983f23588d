#!/usr/bin/env python3
"""vcf_query against the full filtered scan, on one GPU and one generated file.

A bgzipped VCF of about --text-gb GB of text (one contig, single-base records at fixed-width positions from 100 000 000 on, evenly
spread; 65 280 bytes of text a member) is written with its tabix index (tests/tabix_files.py: the members by bgzf_member, the index
by build_index_snps + serialize_index).  Then, in the same run, each the median of --repeats after one warm-up, wall time from open
to the last row (PCIe inclusive):

  vcf_query   exg_open_region over a 1 Mb window in the middle of the file, `chrom, pos, ref` to host DataChunks, and COUNT(*)
  read_vcf    the same file through exg_open with the equivalent pushed-down filter (chrom = '1' AND pos >= s AND pos <= e)

and region_members, the bytes inflated for the region (its members' inflated sizes), and the share of the predicate kernel in a
batch: the exg_vcf_region_keep launch alone (buffers made once) timed with device events on the window's own rows, beside
exg_vcf_scan of the same text.

    python tools/region_bench.py [--text-gb 1] [--repeats 9] [--out profiles/region_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: the library binds to torch's HIP runtime)

import tabix_files as T  # noqa: E402
from exon_duckdb_amd import abi, device, load_library  # noqa: E402
from exon_duckdb_amd._lib import load_test_library  # noqa: E402
from exon_duckdb_amd.reader import ShardReader  # noqa: E402

MEMBER_BYTES = 65280
BASE = 100_000_000      # (nine digits from here to 2^29: every line has the same length)
SPAN = 400_000_000


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def generate(path, text_bytes):
    """-> (lines, positions, text length): the file and its index at path / path.tbi, written member by member"""
    line = b"1\t%09d\t.\tA\tC\t30\tPASS\tDP=17;AF=0.25;MQ=60\n" % 0
    n = max(1000, (text_bytes - len(T.HEADER)) // len(line))
    step = max(1, SPAN // n)
    positions = BASE + np.arange(n, dtype=np.int64) * step
    rows = np.tile(np.frombuffer(line, np.uint8), (n, 1))
    for d in range(9):      # the nine digits of POS, column 2 .. 10 of every line
        rows[:, 2 + d] = 48 + (positions // 10 ** (8 - d)) % 10
    text = T.HEADER + rows.tobytes()
    members, out = [], 0
    with open(path, "wb") as f:
        for pos in range(0, len(text), MEMBER_BYTES):
            piece = text[pos:pos + MEMBER_BYTES]
            m = T.bgzf_member(piece) if pos == 0 else fast_member(piece)
            members.append((out, pos, len(piece)))
            f.write(m)
            out += len(m)
        f.write(T.EOF_MEMBER)
    offsets = len(T.HEADER) + np.arange(n, dtype=np.int64) * len(line)
    idx = T.build_index_snps(b"1", positions, offsets, len(text), members)
    with open(path + ".tbi", "wb") as f:
        f.write(T.bgzip(T.serialize_index(idx), MEMBER_BYTES)[0])
    return n, positions, len(text), members, text


def fast_member(data):
    """tabix_files.bgzf_member at zlib level 1 (a GB of text at level 6 is minutes of one core)"""
    import struct
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25)
    return head + body + struct.pack("<II", zlib.crc32(data), len(data))


def run(make, want_rows, count, repeats):
    tl = load_test_library()
    ms, st = [], None
    for k in range(1 + repeats):       # (the first run warms the page cache and the pools)
        t0 = time.perf_counter()
        r = make()
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
        assert got == want_rows, (got, want_rows)
        if k:
            ms.append(dt)
    return dict(spread(ms), region_members=st["region_members"], device_batches=st["device_batches"], host_vector_bytes=st["host_vector_bytes"])


def kernel_share(text, positions, lo, hi, line_len, repeats):
    """the window's own lines resident in HBM: exg_vcf_scan and exg_vcf_region_keep, device events"""
    a = len(T.HEADER) + int(np.searchsorted(positions, lo)) * line_len
    b = len(T.HEADER) + int(np.searchsorted(positions, hi, side="right")) * line_len
    chunk = text[a:b]
    d_in = device.upload(chunk)
    scan = device.VcfScan(len(chunk))
    out = {}

    def timed(fn):
        ms = []
        for k in range(3 + repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if k >= 3:
                ms.append(t0.elapsed_time(t1))
        return spread(ms)
    out["vcf_scan"] = timed(lambda: scan.launch(d_in, payload_base=1 << 40))
    rows = int(scan.fetch().n_records)
    # the launch alone, like scan.launch: the keep words and the name are made once, outside the timed calls
    lib = load_library()
    keep = torch.zeros((rows + 63) // 64 + 1, dtype=torch.int64, device="cuda")
    d_name = device.upload(b"1")
    args = abi.VcfRegionArgs()
    args.d_chrom, args.d_ref, args.d_info = scan.cols[0].data_ptr(), scan.cols[3].data_ptr(), scan.cols[7].data_ptr()
    args.d_pos, args.d_payload, args.payload_base, args.n_rows = scan.pos.data_ptr(), d_in.data_ptr(), 1 << 40, rows
    args.d_name, args.name_len, args.start, args.end = d_name.data_ptr(), 1, int(lo), int(hi)
    args.d_keep, args.stream = keep.data_ptr(), device.stream_ptr().value
    out["region_keep"] = timed(lambda: device.check(lib.exg_vcf_region_keep(C.byref(args))))
    kept = int(np.unpackbits(keep.cpu().numpy().view(np.uint8), bitorder="little")[:rows].sum())
    assert kept == rows, (kept, rows)      # (the text is the window's own lines)
    out["rows"], out["text_bytes"] = rows, len(chunk)
    out["region_keep_share_of_scan_plus_keep"] = out["region_keep"]["median_ms"] / (out["region_keep"]["median_ms"] + out["vcf_scan"]["median_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-gb", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.vcf.gz")
        t0 = time.perf_counter()
        n, positions, text_len, members, text = generate(path, int(a.text_gb * 1e9))
        line_len = (text_len - len(T.HEADER)) // n
        result["file"] = {"text_bytes": text_len, "file_bytes": os.path.getsize(path), "index_bytes": os.path.getsize(path + ".tbi"), "lines": n,
                          "members": len(members), "generate_s": time.perf_counter() - t0}
        mid = BASE + SPAN // 2
        lo, hi = mid, mid + 1_000_000 - 1
        want = int(np.count_nonzero((positions >= lo) & (positions <= hi)))
        region = "1:%d-%d" % (lo, hi)
        filters = "chrom = '1' AND pos >= %d AND pos <= %d" % (lo, hi)
        result["window"] = {"region": region, "rows": want}
        q = lambda count: run(lambda: ShardReader(path, "vcf", region=region, columns=[0, 1, 3], expect_chunks=not count), want, count, a.repeats)  # noqa: E731
        f = lambda count: run(lambda: ShardReader(path, "vcf", compression="gzip", filters=filters, columns=[0, 1, 3], expect_chunks=not count),  # noqa: E731
                              want, count, a.repeats)
        result["vcf_query"] = {"chrom_pos_ref": q(False), "count": q(True)}
        result["read_vcf_filtered"] = {"chrom_pos_ref": f(False), "count": f(True)}
        rm = result["vcf_query"]["count"]["region_members"]
        result["vcf_query"]["inflated_bytes"] = rm * MEMBER_BYTES     # (an upper bound: the header's member and the last one may be shorter)
        result["speedup"] = {k: result["read_vcf_filtered"][k]["median_ms"] / result["vcf_query"][k]["median_ms"] for k in ("chrom_pos_ref", "count")}
        result["predicate"] = kernel_share(text, positions, lo, hi, line_len, a.repeats)
    out = json.dumps(result, indent=1)
    print(out)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(out + "\n")


if __name__ == "__main__":
    main()
