"""The ordered prefix of the fused FASTQ scan (counts published per 48 KiB super-tile, the central scanner's 64-lane batches
and 512-descriptor probes, a workgroup's wait for its own word) on inputs whose per-tile counts differ.

Bit-exact against the oracle, like tests/test_fastq_gpu.py::check_against_oracle, for the lean scan (EXG_ALGO_FUSED) and the
any-shape scan (EXG_ALGO_FUSED_FULL): buffers of n x 49 152 bytes - 1, + 0, + 1 around the scanner's batch and probe sizes, a
shard with a nonzero lead / first_line_index, and 20 launches on one workspace.  Nothing here tries to make the scanner's
help path or a workgroup's timeout run.
"""
import numpy as np
import pytest

from exon_duckdb_amd import abi

pytestmark = pytest.mark.gpu

BASE = 0x7F0000000000
SUPER = 49152  # bytes per super-tile (3 halves of 16 KiB)
FUSED = (abi.EXG_ALGO_FUSED, abi.EXG_ALGO_FUSED_FULL)
NAMES = ["name", "description", "sequence", "quality_scores"]
TILES = [1, 2, 63, 64, 65, 511, 512, 513, 1024, 1025, 4097]


@pytest.fixture(scope="module")
def ragged(oracle):
    """Ragged reads (names, descriptions and read lengths vary: no two tiles hold the same number of lines), a little more than
    the largest buffer."""
    n_bytes = max(TILES) * SUPER + 1
    data = oracle.synth_fastq_ragged(n_bytes // 300)
    assert len(data) >= n_bytes, "the ragged generator's records became shorter: ask it for more"
    return data


def compare(exp, res, cols, words, n_data, algo):
    assert not (res.flags & abi.EXG_RF_FALLBACK), "a fused launch asked for the general path"
    assert res.error_code == exp.error_code, (res.error_code, exp.error_code, exp.error_message)
    assert res.n_records == exp.n_rows
    if exp.error_code:
        assert res.error_record == exp.error_record
        assert res.error_offset == exp.error_offset
    for k, name in enumerate(NAMES):
        want, want_words = exp.string_t[name]
        assert np.array_equal(cols[k], want), f"column {name} differs (algo {algo})"
        if name == "description":
            nw = (exp.n_rows + 63) // 64
            got = words[:nw].copy()
            if exp.n_rows % 64:
                got[-1] &= np.uint64((1 << (exp.n_rows % 64)) - 1)  # bits of rows past an error are unspecified
            assert np.array_equal(got, want_words[:nw]), "description validity differs"
    if not exp.error_code:
        assert res.consumed_bytes == n_data


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("tiles", TILES)
def test_buffer_sizes_around_batches_and_probes(gpu, oracle, ragged, tiles, delta):
    from exon_duckdb_amd import device

    data = bytes(ragged[: tiles * SUPER + delta])  # cut anywhere: mostly inside a record (UnexpectedEof on it, like the oracle)
    exp = oracle.fastq_parse(data, payload_base=BASE)
    assert exp.n_rows >= tiles * SUPER // 720
    d_in = device.upload(data)
    scan = device.FastqScan(len(data))
    for algo in FUSED:
        scan.launch(d_in, payload_base=BASE, algo=algo)
        res = scan.fetch()
        cols, words = scan.columns_host(int(res.n_records))
        compare(exp, res, cols, words, len(data), algo)


@pytest.mark.parametrize("algo", FUSED)
def test_shards_with_lead_and_first_line_index(gpu, oracle, ragged, algo):
    """Byte-range shards of several hundred super-tiles each, cut at 16-byte (not record) boundaries, each with a halo in front
    as `lead` and the line index of its first byte: the rows reassemble to the oracle's."""
    from exon_duckdb_amd import device

    n = 700 * SUPER + 4096
    data = bytes(ragged[:n])
    data = data[: data.rfind(b"\n@") + 1]  # ('@' after a newline may be a quality line's: then the oracle reports it, too)
    n = len(data)
    exp = oracle.fastq_parse(data, payload_base=BASE)
    assert exp.error_code == 0, "the cut fell on a quality line that begins with '@': move it"
    nl = np.flatnonzero(np.frombuffer(data, np.uint8) == 10)
    cuts = [0, 16 * 1021, 65 * SUPER + 16 * 77, 66 * SUPER, 578 * SUPER - 16, n]
    got_cols, got_valid, total = [[] for _ in range(4)], [], 0
    for s, e in zip(cuts[:-1], cuts[1:]):
        h = min(2048, s)
        buf = data[s - h:e]
        d_in = device.upload(buf)
        scan = device.FastqScan(len(buf))
        flags = (abi.EXG_F_BOF if s - h == 0 else 0) | (abi.EXG_F_EOF if e == n else 0)
        scan.launch(d_in, lead=h, first_line_index=int(np.searchsorted(nl, s)), payload_base=BASE + s - h, flags=flags, algo=algo)
        res = scan.fetch()
        assert res.error_code == 0 and not (res.flags & (abi.EXG_RF_HEAD_UNRESOLVED | abi.EXG_RF_FALLBACK))
        k = int(res.n_records)
        cols, words = scan.columns_host(k)
        for c in range(4):
            got_cols[c].append(cols[c])
        got_valid.append(np.unpackbits(words.view(np.uint8), bitorder="little")[:k])
        total += k
    assert total == exp.n_rows
    for c, name in enumerate(NAMES):
        assert np.array_equal(np.concatenate(got_cols[c]), exp.string_t[name][0]), name
    assert np.array_equal(np.concatenate(got_valid), exp.columns["description"].valid)


@pytest.mark.parametrize("algo", FUSED)
def test_twenty_launches_on_one_workspace(gpu, oracle, ragged, algo):
    """Two inputs of one size take turns on ONE workspace, 20 launches queued without a host wait between them: a prefix word
    left over from the launch before belongs to the other input and would move rows.  Every launch of an input must give what
    its first launch gave, and that is the oracle's."""
    import torch

    from exon_duckdb_amd import device

    n = 600 * SUPER + 48
    whole = bytes(ragged[: 1000 * SUPER])
    s1 = whole.index(b"\n@", 300 * SUPER + 7) + 1  # the second input begins at a record ('@' after a newline may be a quality
    inputs = [whole[:n], whole[s1:s1 + n]]          # line's: then every row of it is an error, here and in the oracle)
    d_in = [device.upload(b) for b in inputs]
    scan = device.FastqScan(n)
    kept = []
    for i in range(20):
        scan.launch(d_in[i % 2], payload_base=BASE, flags=abi.EXG_F_BOF, algo=algo)  # (no EOF: the open record at the end is left)
        kept.append(([c.clone() for c in scan.cols], scan.validity.clone(), scan.result.clone()))
    torch.cuda.synchronize()
    for i in range(2, 20):  # (rows past n_records belong to whatever was launched before: only the launch's own rows count)
        assert torch.equal(kept[i][2], kept[i % 2][2]), f"launch {i}: the result block differs from launch {i % 2}'s"
        k = int(kept[i][2][0].item())
        for a, b in zip(kept[i][0], kept[i % 2][0]):
            assert torch.equal(a[:k], b[:k]), f"launch {i}: a column differs from launch {i % 2}'s"
        assert torch.equal(kept[i][1][: k // 64], kept[i % 2][1][: k // 64]), f"launch {i}: description validity"
    for which in (0, 1):
        exp = oracle.fastq_parse(inputs[which], payload_base=BASE)
        k = int(kept[which][2][0].item())  # exg_scan_result.n_records
        assert exp.n_rows - 1 <= k <= exp.n_rows and k > n // 720  # (the oracle reads the cut record at the end as far as it goes)
        for c, name in enumerate(NAMES):
            got = kept[which][0][c][:k].cpu().numpy().view(np.uint8).reshape(k, 16)
            assert np.array_equal(got, exp.string_t[name][0][:k]), name
