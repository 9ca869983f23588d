#!/usr/bin/env python3
"""Rates of the sequence scalars (exg_sequence_op) on one GPU, in one run on one device:

  yardstick  the read-only stream rate (exg_count_newlines) over the buffer the sequences lie in
  short      every op on the `sequence` column exg_fastq_scan leaves for synthetic FASTQ-150 (--fastq-gb of text)
  long       every op on a column of --long-rows rows of --long-mb MB each (a genome's chromosomes as read_fasta returns
             them: string_t rows pointing into one payload buffer of random A, C, G, T)
  host       the host scalar loop of the DuckDB shim on one core, over one long row

    python tools/seqfn_bench.py [--fastq-gb 1] [--long-rows 16] [--long-mb 64] [--repeats 9] [--warmup 3] [--out FILE]

Prints one JSON document.  Rates are GB/s of SEQUENCE bytes (10^9; the op's input), with the fraction of the yardstick
measured on the same buffer, and the per-byte time of the long shape against the short one for every op."""
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

OPS = {"complement": abi.EXG_SEQ_COMPLEMENT, "reverse_complement": abi.EXG_SEQ_REVERSE_COMPLEMENT, "transcribe": abi.EXG_SEQ_TRANSCRIBE,
       "reverse_transcribe": abi.EXG_SEQ_REVERSE_TRANSCRIBE, "translate_dna_to_aa": abi.EXG_SEQ_TRANSLATE, "gc_content": abi.EXG_SEQ_GC_CONTENT}
BASE = 1 << 40


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
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "n": len(ms), "GB/s": n_bytes / med / 1e6}


class Op:
    """one op with its buffers allocated once: launch() only enqueues"""

    def __init__(self, op, d_col, n_rows, d_payload, payload_base, out_capacity):
        self.lib = load_library()
        gc = op == abi.EXG_SEQ_GC_CONTENT
        self.out_col = torch.empty((1 if gc else max(n_rows, 1), 2), dtype=torch.int64, device="cuda")
        self.out_payload = torch.empty(16 if gc else out_capacity + 16, dtype=torch.uint8, device="cuda")
        self.out_float = torch.empty(max(n_rows, 1) if gc else 1, dtype=torch.float32, device="cuda")
        ws_bytes = int(self.lib.exg_sequence_workspace_bytes(op, n_rows))
        self.ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device="cuda")
        self.d_result = torch.zeros(8, dtype=torch.int64, device="cuda")
        a = self.args = abi.SequenceOpArgs()
        a.op, a.n_rows, a.d_strings = op, n_rows, d_col.data_ptr()
        a.d_payload, a.payload_base = d_payload.data_ptr(), payload_base
        a.d_out_strings, a.d_out_payload, a.out_capacity, a.out_base = self.out_col.data_ptr(), self.out_payload.data_ptr(), out_capacity, device.SEQ_OUT_BASE
        a.d_out_float = self.out_float.data_ptr()
        a.d_workspace, a.workspace_bytes, a.d_result = self.ws.data_ptr(), ws_bytes, self.d_result.data_ptr()
        a.stream = device.stream_ptr().value

    def launch(self):
        device.check(self.lib.exg_sequence_op(C.byref(self.args)))

    def result(self):
        r = abi.SeqResult()
        self.lib.exg_sequence_result(C.c_void_p(self.d_result.data_ptr()), device.stream_ptr(), C.byref(r))
        return r


def stream_rate(d_buf, n, repeats, warmup):
    lib = load_library()
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    return timed(lambda: device.check(lib.exg_count_newlines(C.c_void_p(d_buf.data_ptr()), 0, n, C.c_void_p(d_count.data_ptr()), device.stream_ptr())),
                 n, repeats, warmup)


def bench_column(d_col, n_rows, d_payload, payload_base, seq_bytes, repeats, warmup):
    out = {}
    for name, op in OPS.items():
        run = Op(op, d_col, n_rows, d_payload, payload_base, seq_bytes)
        out[name] = timed(run.launch, seq_bytes, repeats, warmup)
        r = run.result()
        out[name].update(error_code=r.error_code, output_payload_bytes=int(r.total_bytes))
        assert not (r.flags & abi.EXG_RF_CAPACITY)
        del run
        torch.cuda.empty_cache()
    return out


def bench_host(n_bytes, repeats):
    tl = load_test_library()
    rng = np.random.default_rng(3)
    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n_bytes - n_bytes % 3)].tobytes()
    out_buf, n_out, err = C.create_string_buffer(len(s)), C.c_uint64(0), C.create_string_buffer(128)
    res = {}
    for name, op in OPS.items():
        if op == abi.EXG_SEQ_REVERSE_TRANSCRIBE:
            continue        # (its alphabet has no T: the loop would stop at the first one)
        ms = []
        for k in range(1 + repeats):
            t0 = time.perf_counter()
            rc = tl.exon_tf_sequence_fn(op, s, len(s), out_buf, len(out_buf), C.byref(n_out), err, len(err))
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0, err.value
            if k:
                ms.append(dt)
        res[name] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms), "GB/s": len(s) / statistics.median(ms) / 1e6}
    return dict(res, input_bytes=len(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fastq-gb", type=float, default=1.0)
    ap.add_argument("--long-rows", type=int, default=16)
    ap.add_argument("--long-mb", type=float, default=64.0)
    ap.add_argument("--host-mb", type=float, default=64.0)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "unit": "GB/s of sequence bytes (10^9)"}

    # short rows: the sequence column of a FASTQ-150 scan
    n_text = int(a.fastq_gb * (1 << 30)) // abi.EXG_SYNTH_FASTQ_RECORD_BYTES * abi.EXG_SYNTH_FASTQ_RECORD_BYTES
    n_rec = n_text // abi.EXG_SYNTH_FASTQ_RECORD_BYTES
    d_in = device.synth_fastq(n_text)
    scan = device.FastqScan(n_text, capacity_records=n_rec + 64)
    scan.launch(d_in, payload_base=BASE)
    res = scan.fetch()
    assert res.error_code == 0 and res.n_records == n_rec, (res.n_records, res.error_code)
    seq_bytes = 150 * n_rec
    short = {"rows": n_rec, "sequence_bytes": seq_bytes, "text_bytes": n_text, "stream_read_only_text": stream_rate(d_in, n_text, a.repeats, a.warmup)}
    short["ops"] = bench_column(scan.cols[2], n_rec, d_in, BASE, seq_bytes, a.repeats, a.warmup)
    result["short_rows_fastq150"] = short
    del scan, d_in
    torch.cuda.empty_cache()

    # long rows: a few rows of tens of MB in one payload buffer
    row_bytes = int(a.long_mb * 1e6) // 48 * 48
    n = a.long_rows * row_bytes
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    d_payload = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    step = 1 << 26
    for at in range(0, n, step):
        m = min(step, n - at)
        d_payload[at:at + m] = letters[torch.randint(0, 4, (m,), device="cuda")]
    prefix = d_payload[:n].view(a.long_rows, row_bytes)[:, :4].cpu().numpy()
    col = np.zeros((a.long_rows, 16), np.uint8)
    for r in range(a.long_rows):
        col[r, :4] = np.frombuffer(np.uint32(row_bytes).tobytes(), np.uint8)
        col[r, 4:8] = prefix[r]
        col[r, 8:16] = np.frombuffer(np.uint64(BASE + r * row_bytes).tobytes(), np.uint8)
    d_col = torch.from_numpy(col).cuda()
    long = {"rows": a.long_rows, "row_bytes": row_bytes, "sequence_bytes": n, "stream_read_only": stream_rate(d_payload, n, a.repeats, a.warmup)}
    long["ops"] = bench_column(d_col, a.long_rows, d_payload, BASE, n, a.repeats, a.warmup)
    result["long_rows"] = long
    del d_payload
    torch.cuda.empty_cache()

    yard_short = short["stream_read_only_text"]["GB/s"]
    yard_long = long["stream_read_only"]["GB/s"]
    summary = {}
    for name in OPS:
        s, l = short["ops"][name], long["ops"][name]
        summary[name] = {"short_GB/s": s["GB/s"], "long_GB/s": l["GB/s"], "short_fraction_of_stream": s["GB/s"] / yard_short,
                         "long_fraction_of_stream": l["GB/s"] / yard_long,
                         "long_over_short_time_per_byte": (l["median_ms"] / n) / (s["median_ms"] / seq_bytes)}
    result["summary"] = summary
    if a.host_mb > 0:
        result["host_scalar_loop_one_core"] = bench_host(int(a.host_mb * 1e6), max(3, a.repeats // 3))
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
