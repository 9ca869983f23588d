"""bench.py --dump-outputs: the helper that writes what the timed launch computed, run on host tensors shaped like a
FastqScan's outputs (no GPU needed)."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Scan:
    def __init__(self, torch, n):
        g = torch.Generator().manual_seed(7)
        self.cols = [torch.randint(-2 ** 62, 2 ** 62, (n + 16, 2), dtype=torch.int64, generator=g) for _ in range(4)]
        self.validity = torch.randint(-2 ** 62, 2 ** 62, ((n + 16 + 63) // 64,), dtype=torch.int64, generator=g)
        self.validity[0] = -1


def _result(n):
    from exon_duckdb_amd import abi
    r = abi.ScanResult()
    r.n_records, r.n_lines, r.consumed_bytes, r.flags = n, 4 * n, 332 * n, 0
    return r


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _check_rows(torch, scan, got):
    rows = got["rows"].astype(np.int64)
    for k, name in enumerate(["name", "description", "sequence", "quality_scores"]):
        a = got[name]
        assert a.dtype == np.float64 and a.shape == (len(rows), 4)
        want = scan.cols[k][torch.from_numpy(rows)].numpy().view(np.uint32).reshape(-1, 4)
        assert np.array_equal(a.astype(np.uint32), want)
    words = scan.validity.numpy().view(np.uint64)
    bits = (words[rows >> 6] >> (rows & 63).astype(np.uint64)) & np.uint64(1)
    assert np.array_equal(got["description_validity"], bits.astype(np.float64))


def test_small_output_is_dumped_whole(tmp_path):
    import torch
    b = _bench()
    n = 1000
    scan = _Scan(torch, n)
    b.dump_fastq_outputs(torch, scan, _result(n), n, str(tmp_path))
    got = _load(tmp_path)
    assert set(got) == {"rows", "result", "name", "description", "sequence", "quality_scores", "description_validity"}
    assert np.array_equal(got["rows"], np.arange(n, dtype=np.float64))
    assert got["result"].dtype == np.float64 and got["result"][0] == n and got["result"][1] == 4 * n
    assert got["description_validity"][:64].sum() == 64
    _check_rows(torch, scan, got)


def test_large_output_is_a_fixed_sample_under_64_mb(tmp_path):
    import torch
    b = _bench()
    n = b.DUMP_ROWS * 3 + 5
    scan = _Scan(torch, n)
    a, c = tmp_path / "a", tmp_path / "c"
    b.dump_fastq_outputs(torch, scan, _result(n), n, str(a))
    b.dump_fastq_outputs(torch, scan, _result(n), n, str(c))
    got = _load(a)
    rows = got["rows"]
    assert len(rows) == b.DUMP_ROWS and rows[0] == 0 and rows[-1] == n - 1 and np.all(np.diff(rows) > 0)
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= 64 * 10 ** 6
    again = _load(c)
    assert all(np.array_equal(got[k], again[k]) for k in got)
    _check_rows(torch, scan, got)
