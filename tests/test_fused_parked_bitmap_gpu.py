"""Half 0's newline masks of the lean FASTQ scan have no LDS of their own (exg_fused_core.hpp, FusedLdsT PARK): until half 0 is
staged they wait in the byte buffer, each thread's four masks where that thread's last chunk goes.  So inputs here are built for
half 0's masks to matter: newlines in the first and the last byte of a thread's 64-byte span (threads 0, 63, 64, 255 — the seams
between lanes, waves and halves), a half 0 without any newline, an input that ends inside half 0 (the cold block that takes the
bits past the end out of the parked entries), a buffer that begins in the middle of a file (no EXG_F_BOF; byte 0 is a newline)
and a record whose head lies in the window in front of its super-tile.

Every case runs the lean scan (EXG_ALGO_FUSED, with the redo run behind it) and the any-shape scan (EXG_ALGO_FUSED_FULL) and holds
both bit-exact against oracle.fastq_parse, compared as tests/test_scan_input_end_gpu.py::run_fastq does.  1 - 3 super-tiles each.
"""
import numpy as np
import pytest

from exon_duckdb_amd import abi

pytestmark = pytest.mark.gpu

BASE = 0x7F0000000000
HALF = 16384
SUPER = 3 * HALF
FUSED = (abi.EXG_ALGO_FUSED, abi.EXG_ALGO_FUSED_FULL)
NAMES = ["name", "description", "sequence", "quality_scores"]
HEADS = [b"@r", b"@rr", b"@read x", b"@read xy", b"@n \r", b"@nn d"]  # (even and odd lengths; with and without a description)
EMPTY = b"@e\n\n+\n\n"  # name line, empty sequence, '+', empty quality: newlines at +2 and +3


class File:
    """a FASTQ file put together so that chosen offsets hold a newline"""

    def __init__(self):
        self.buf = bytearray()
        self.starts = []
        self.k = 0

    def rec(self, total, fill=(b"A", b"I")):
        """a record of exactly `total` bytes (>= 10)"""
        self.k += 1
        for i in range(len(HEADS)):
            head = HEADS[(self.k + i) % len(HEADS)]
            two_m = total - len(head) - 5
            if two_m >= 2 and two_m % 2 == 0:
                break
        else:
            raise AssertionError(total)
        m = two_m // 2
        self.starts.append(len(self.buf))
        self.buf += head + b"\n" + fill[0] * m + b"\n+\n" + fill[1] * m + b"\n"

    def fill_to(self, x, piece=150):
        """whole records up to offset x exactly: the byte at x - 1 is a newline"""
        assert x - len(self.buf) >= 10, (x, len(self.buf))
        while x - len(self.buf) >= piece + 24:
            self.rec(piece + len(self.buf) % 7)
        self.rec(x - len(self.buf))
        assert len(self.buf) == x

    def newline_at(self, t):
        self.fill_to(t + 1)

    def newlines_at_pair(self, t):
        """newlines at t and t + 1: a name line that ends at t, an empty sequence line"""
        self.fill_to(t - 2)
        self.starts.append(len(self.buf))
        self.buf += EMPTY
        assert self.buf[t] == 10 and self.buf[t + 1] == 10


def compare(exp, first, res, cols, words, consumed, algo):
    """rows [first, ...) of the oracle's, as tests/test_scan_input_end_gpu.py::compare_fastq holds a launch against it"""
    assert not (res.flags & abi.EXG_RF_FALLBACK), "a fused launch asked for the general path"
    assert exp.error_code == 0 and res.error_code == 0, (res.error_code, exp.error_code, exp.error_message)
    n = exp.n_rows - first
    assert res.n_records == n
    for k, name in enumerate(NAMES):
        want, _ = exp.string_t[name]
        assert np.array_equal(cols[k], want[first:]), f"column {name} differs (algo {algo})"
    got = np.unpackbits(words.view(np.uint8), bitorder="little")[:n]
    assert np.array_equal(got, np.asarray(exp.columns["description"].valid, np.uint8)[first:]), f"description validity differs (algo {algo})"
    assert res.consumed_bytes == consumed


def run(oracle, data, origin=0, own_from=0):
    """data[origin:] as one buffer; the rows of the records that begin at `own_from` or behind it (origin > 0: no EXG_F_BOF, the
    bytes in front of own_from are the halo).  Returns the launches' results."""
    from exon_duckdb_amd import device

    data = bytes(data)
    exp = oracle.fastq_parse(data, payload_base=BASE)
    nl = np.flatnonzero(np.frombuffer(data, np.uint8) == 10)
    starts = np.concatenate([[0], nl[3::4] + 1])[: exp.n_rows]
    first = int(np.searchsorted(starts, own_from))
    buf = data[origin:]
    assert SUPER // 3 < len(buf) <= 3 * SUPER
    d_in = device.upload(buf)
    scan = device.FastqScan(len(buf))
    flags = abi.EXG_F_EOF | (abi.EXG_F_BOF if origin == 0 else 0)
    results = []
    for algo in FUSED:
        scan.launch(d_in, lead=own_from - origin, first_line_index=int(np.searchsorted(nl, own_from)), payload_base=BASE + origin,
                    flags=flags, algo=algo)
        res = scan.fetch()
        assert not (res.flags & abi.EXG_RF_HEAD_UNRESOLVED)
        cols, words = scan.columns_host(int(res.n_records))
        compare(exp, first, res, cols, words, len(buf), algo)
        results.append(res)
    return results


def span_seams(origin, base):
    """newlines in the first and the last byte of the 64-byte spans of threads 0, 63, 64 and 255 of the half that begins at `base`
    bytes into the buffer — and so in the last byte of that half and the first byte of the next"""
    f = File()
    if origin:
        f.newline_at(origin)  # byte 0 of the buffer: the first byte of thread 0's span
    b = origin + base
    if base:
        f.newline_at(b)
    f.newlines_at_pair(b + 63)        # thread 0's last byte, thread 1's first
    f.newline_at(b + 63 * 64)         # thread 63's first byte (4032)
    f.newlines_at_pair(b + 4095)      # thread 63's last byte, thread 64's first: the seam between waves 0 and 1
    f.newline_at(b + 64 * 64 + 63)    # thread 64's last byte (4159)
    f.newline_at(b + 255 * 64)        # thread 255's first byte (16320)
    f.newlines_at_pair(b + HALF - 1)  # thread 255's last byte = the half's last byte, and the next half's first byte
    return f


@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("bof", [True, False])
def test_newlines_on_the_seams_of_half_0(gpu, oracle, bof, tile):
    origin = 0 if bof else 331
    f = span_seams(origin, tile * SUPER)
    f.fill_to(origin + (tile + 1) * SUPER + 777)
    data = bytes(f.buf)
    for t in (63, 64, 4032, 4095, 4096, 4159, 16320, 16383, 16384) + (() if bof and tile == 0 else (0,)):
        assert data[origin + tile * SUPER + t] == 10, t
    own_from = 0 if bof else next(s for s in f.starts if s >= origin + 200)
    run(oracle, data, origin, own_from)


@pytest.mark.parametrize("bof", [True, False])
def test_half_0_without_a_newline(gpu, oracle, bof):
    """the sequence line of a long read covers all of half 0 of super-tile 1: the lean scan marks the super-tile (the record begins
    far in front of the window), the redo run behind it produces the rows"""
    origin = 0 if bof else 97
    f = File()
    if origin:
        f.newline_at(origin)
    f.fill_to(origin + SUPER - 500)
    f.rec(2 * 18000 + 6)
    f.fill_to(origin + 3 * SUPER - 100)
    data = bytes(f.buf)
    assert 10 not in data[origin + SUPER:origin + SUPER + HALF]
    own_from = 0 if bof else next(s for s in f.starts if s >= origin + 200)
    lean, full = run(oracle, data, origin, own_from)
    assert lean.flags & abi.EXG_RF_REDO and lean.redo_tiles >= 1, "the lean scan did not hand the long read to the redo run"


@pytest.mark.parametrize("d", range(-7, 7))
@pytest.mark.parametrize("k", [0, 1])
def test_input_ends_inside_half_0(gpu, oracle, k, d):
    """the fourteen offsets around the seam of two of a thread's chunk rows (4 096 bytes into half 0): the workgroup that holds
    the end of the input masks its parked entries"""
    b = k * SUPER
    n = b + 4096 + d
    f = File()
    if b:
        f.fill_to(b)
    f.newlines_at_pair(b + 63)   # (the seams of half 0 that lie in front of the end)
    f.newline_at(b + 63 * 64)
    f.fill_to(n)                 # the last record ends with the input
    run_behind(oracle, bytes(f.buf), n)


def run_behind(oracle, data, n):
    """data[:n] in a buffer that goes on behind n with newlines, tabs, '@' and 0xFF: never to be looked at"""
    from exon_duckdb_amd import device

    exp = oracle.fastq_parse(data, payload_base=BASE)
    buf = np.frombuffer(data + b"\n\t@\xff" * 64, np.uint8)
    d_in = device.upload(buf.tobytes())
    scan = device.FastqScan(n)
    for algo in FUSED:
        scan.launch(d_in, n_bytes=n, payload_base=BASE, flags=abi.EXG_F_BOF | abi.EXG_F_EOF, algo=algo)
        res = scan.fetch()
        cols, words = scan.columns_host(int(res.n_records))
        compare(exp, 0, res, cols, words, n, algo)


@pytest.mark.parametrize("head", [800, 1000, 64])
def test_window_holds_the_head_of_the_straddling_record(gpu, oracle, head):
    """a record that begins `head` bytes in front of super-tile 1 and ends in its half 0: its head is read from the 1 KiB window"""
    f = File()
    f.fill_to(SUPER - head)
    f.rec(head + 100)
    f.fill_to(2 * SUPER + 50)
    lean, full = run(oracle, bytes(f.buf))
    assert not (lean.flags & abi.EXG_RF_REDO), "a record that begins inside the window is the lean scan's own"
