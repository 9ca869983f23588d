"""The end of the input inside a super-tile of the fused scans (exg_fused_core.hpp).

The classification loop of k_fused knows nothing of the end of the input: a chunk that lies past it is loaded from the input's
last 16-byte chunk and stays a copy of it, and the one workgroup that holds the end takes the newline (and tab) bits past it out of
its maps behind the loop.  So the rows must not depend on what lies behind `n_bytes`: every buffer here is LONGER than the
`n_bytes` it is launched with — the file's own next records follow, the most tempting bytes there are — and for a third of the
cases the 64 bytes from round_up(n, 16) on (which the API does not even promise to be readable) are '\\n', '\\t', '@' and 0xFF.

FASTQ: bit-exact against oracle.fastq_parse(data[:n]), compared the way tests/test_fastq_prefix_gpu.py::compare does, for the lean
scan (EXG_ALGO_FUSED) and the any-shape scan (EXG_ALGO_FUSED_FULL), n = k x 49 152 + d around every chunk, half and super-tile
seam, with and without EXG_F_EOF (without it the open record at the end is left: the rows are the oracle's first ones).
VCF (the instance that also keeps a tab map): the same grid through device.VcfScan with the header as `lead`, compared as
tests/test_vcf_gpu.py::check compares a launch with the oracle.
"""
import numpy as np
import pytest

from exon_duckdb_amd import abi

pytestmark = pytest.mark.gpu

BASE = 0x7F0000000000
SUPER = 49152  # bytes per FASTQ super-tile (3 halves of 16 KiB; a VCF super-tile is 2 halves)
FUSED = (abi.EXG_ALGO_FUSED, abi.EXG_ALGO_FUSED_FULL)
NAMES = ["name", "description", "sequence", "quality_scores"]
KS = [0, 1, 2]
DS = [1, 15, 16, 17, 16383, 16384, 16385, 32767, 32768, 32769, 49135, 49136, 49151, 49152]
GRID = [(k, d) for k in KS for d in DS]
BEHIND = 4096  # bytes of the file kept in the buffer behind n_bytes
SCRIBBLE = np.frombuffer(b"\n\t@\xff" * 16, np.uint8)


def scribbled(k, d):
    return GRID.index((k, d)) % 3 == 0


def upload_longer(data, n, scribble):
    """data[:n] and what follows it in the file; optionally [round_up(n, 16), + 64) overwritten: never to be looked at"""
    from exon_duckdb_amd import device

    buf = np.frombuffer(bytes(data[: n + BEHIND]), np.uint8).copy()
    assert len(buf) == n + BEHIND
    if scribble:
        up = (n + 15) // 16 * 16
        buf[up:up + 64] = SCRIBBLE
    return device.upload(buf.tobytes())


@pytest.fixture(scope="module")
def ragged(oracle):
    data = bytes(oracle.synth_fastq_ragged(600))
    assert len(data) >= 3 * SUPER + BEHIND, "the ragged generator's records became shorter: ask it for more"
    assert max(data) < 0x80
    return data


@pytest.fixture(scope="module")
def vcf(oracle):
    data = bytes(oracle.synth_vcf(3600))
    assert len(data) >= 3 * SUPER + BEHIND
    return data


def compare_fastq(exp, res, cols, words, n_data, algo):
    """tests/test_fastq_prefix_gpu.py::compare"""
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


def compare_fastq_open_end(exp, data, res, cols, words, algo):
    """Without EXG_F_EOF: the rows are the records whose four lines are complete — the oracle's first ones (it reads the open
    record at the end as far as it goes, or reports it) —, no error, consumed_bytes = where the open record begins."""
    nl = np.flatnonzero(np.frombuffer(data, np.uint8) == 10)
    k = len(nl) // 4
    assert not (res.flags & abi.EXG_RF_FALLBACK), "a fused launch asked for the general path"
    assert res.error_code == 0
    assert res.n_records == k
    for c, name in enumerate(NAMES):
        want, want_words = exp.string_t[name]
        assert np.array_equal(cols[c], want[:k]), f"column {name} differs (algo {algo})"
        if name == "description":
            got = np.unpackbits(words.view(np.uint8), bitorder="little")[:k]
            assert np.array_equal(got, np.unpackbits(want_words.view(np.uint8), bitorder="little")[:k]), "description validity differs"
    assert res.consumed_bytes == (int(nl[4 * k - 1]) + 1 if k else 0)


def run_fastq(oracle, data, n, scribble, flag_sets=(abi.EXG_F_BOF | abi.EXG_F_EOF, abi.EXG_F_BOF), d_in=None):
    from exon_duckdb_amd import device

    head = bytes(data[:n])
    exp = oracle.fastq_parse(head, payload_base=BASE)
    if d_in is None:
        d_in = upload_longer(data, n, scribble)
    scan = device.FastqScan(n)
    results = []
    for flags in flag_sets:
        for algo in FUSED:
            scan.launch(d_in, n_bytes=n, payload_base=BASE, flags=flags, algo=algo)
            res = scan.fetch()
            cols, words = scan.columns_host(int(res.n_records))
            if flags & abi.EXG_F_EOF:
                compare_fastq(exp, res, cols, words, n, algo)
            else:
                compare_fastq_open_end(exp, head, res, cols, words, algo)
            results.append(res)
    return exp, results


@pytest.mark.parametrize("k,d", GRID)
def test_fastq_input_ends_anywhere_in_a_super_tile(gpu, oracle, ragged, k, d):
    run_fastq(oracle, ragged, k * SUPER + d, scribbled(k, d))


def complete_records(data, limit):
    """the longest prefix of `data` of whole records (it begins with one) that is no longer than `limit`"""
    nl = np.flatnonzero(np.frombuffer(data[:limit], np.uint8) == 10)
    k = len(nl) // 4
    return data[: int(nl[4 * k - 1]) + 1] if k else b""


@pytest.mark.parametrize("high", [True, False])
@pytest.mark.parametrize("k,d", [(0, 16384), (1, 15), (2, 32779)])
def test_fastq_bytes_above_0x7f_in_the_last_chunk(gpu, oracle, ragged, k, d, high):
    """The last real 16-byte chunk of the input (the one every chunk past the end is a copy of) holds a two-byte UTF-8 character,
    or holds none while 0xFF follows right behind the input: EXG_RF_NON_ASCII is set in the first case and clear in the second,
    and the rows are the oracle's."""
    from exon_duckdb_amd import device

    n = k * SUPER + d
    last = (b"@\xc3\xa9\nA\n+\nI\n" if high else b"@ab\nA\n+\nI\n")  # 10 bytes: inside the last chunk whenever n % 16 is 0 or >= 10
    front = complete_records(ragged, max(n - len(last) - 10, 0))
    gap = n - len(last) - len(front)  # a filler record of exactly that many bytes: "@f[f]\n" A..A "\n+\n" I..I "\n"
    name = b"@f" if gap % 2 == 1 else b"@ff"
    m = (gap - len(name) - 5) // 2
    assert m >= 1
    data = front + name + b"\n" + b"A" * m + b"\n+\n" + b"I" * m + b"\n" + last
    assert len(data) == n and (n % 16 == 0 or n % 16 >= 10)
    buf = np.zeros((n + 15) // 16 * 16 + 64, np.uint8)
    buf[:n] = np.frombuffer(data, np.uint8)
    buf[n:(n + 15) // 16 * 16] = ord("A")          # the rest of the last chunk: the API lets the kernel read it
    buf[(n + 15) // 16 * 16:] = 0xFF               # ... and nothing behind it
    exp, results = run_fastq(oracle, data, n, False, d_in=device.upload(buf.tobytes(), pad=0))
    assert exp.error_code == 0 and exp.n_rows >= 2
    for res in results:
        assert bool(res.flags & abi.EXG_RF_NON_ASCII) == high


@pytest.mark.parametrize("cut", ["last_line_without_newline", "after_the_plus_line"])
@pytest.mark.parametrize("d", [17, 16385])
@pytest.mark.parametrize("k", KS)
def test_fastq_cut_last_record(gpu, oracle, ragged, k, d, cut):
    """EOF rules at the end of the input inside a super-tile: an unterminated quality line is a line; a record cut behind its '+'
    line gets an empty quality line (noodles: read_line returns 0 bytes at EOF without error)."""
    n = k * SUPER + d
    front = complete_records(ragged, max(n - 9, 0))
    rest = n - len(front)
    if cut == "after_the_plus_line":
        tail = b"@t\n" + b"A" * (rest - 6) + b"\n+\n"
    else:
        name = b"@t" if rest % 2 == 0 else b"@tt"
        m = (rest - len(name) - 4) // 2
        assert m >= 1
        tail = name + b"\n" + b"A" * m + b"\n+\n" + b"I" * m
    data = front + tail
    assert len(data) == n
    exp, _ = run_fastq(oracle, data + ragged[:BEHIND], n, scribbled(k, d), flag_sets=(abi.EXG_F_BOF | abi.EXG_F_EOF,))
    assert exp.error_code == 0 and exp.n_rows == (len(front) and front.count(b"\n") // 4) + 1


def header_bytes(data):
    pos = 0
    while pos < len(data) and data[pos:pos + 1] == b"#":
        nl = data.find(b"\n", pos)
        pos = len(data) if nl < 0 else nl + 1
    return pos


def bits(words, n):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n]


@pytest.mark.parametrize("k,d", GRID)
def test_vcf_input_ends_anywhere_in_a_super_tile(gpu, oracle, vcf, k, d):
    """tests/test_vcf_gpu.py::check on a buffer that goes on behind n_bytes"""
    from exon_duckdb_amd import device

    n = k * SUPER + d
    head = vcf[:n]
    exp = oracle.vcf_parse(head, payload_base=BASE)
    d_in = upload_longer(vcf, n, scribbled(k, d))
    scan = device.VcfScan(n)
    for algo in FUSED:
        scan.launch(d_in, n_bytes=n, lead=header_bytes(head), payload_base=BASE, algo=algo)
        res = scan.fetch()
        got = scan.host(int(res.n_records))
        assert not (res.flags & abi.EXG_RF_FALLBACK), "a fused launch asked for the general path"
        if exp.error_code == abi.EXG_PE_VCF_NO_HEADER:
            # n_bytes ends inside the header (k = 0, d <= 17): "missing header" is the oracle's alone — the reader's host side
            # reports it before any launch (tests/test_vcf_gpu.py::test_no_header_is_reported_by_the_oracle_only).  The scan
            # sees a cut line and no row in front of it; what it calls that line is not pinned here.
            assert res.n_records == 0 == exp.n_rows
            continue
        assert res.error_code == exp.error_code, (res.error_code, exp.error_code, exp.error_message)
        assert res.n_records == exp.n_rows
        rows = exp.n_rows
        if exp.error_code:
            assert res.error_record == exp.error_record and res.error_offset == exp.error_offset
        for c, name in enumerate(oracle.VCF_FIELDS):
            assert np.array_equal(got["cols"][c], exp.string_t[name][0]), name
        assert np.array_equal(got["pos"], exp.extra["pos"])
        qv = bits(got["qual_valid"], rows)
        assert np.array_equal(qv, exp.extra["qual_valid"])
        assert np.array_equal(got["qual"].view(np.uint32)[qv == 1], exp.extra["qual"].view(np.uint32)[qv == 1])  # bit exact
        assert np.array_equal(bits(got["formats_valid"], rows), exp.columns["formats"].valid)
        if not exp.error_code:
            assert res.consumed_bytes == n and res.n_lines == rows
