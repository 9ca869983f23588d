"""The fuzz inputs of tests/fuzz_records.py, held to what makes them worth running on a device (no GPU here): every input goes
through its format's Python reference, which must never raise; every record error of the format occurs; at least a tenth of a
format's inputs are clean; at least half of the failing ones have rows in front of the error.  These are conditions on the
inputs — when one fails, tune the generators, not the condition.  Prints, per format, how many inputs had which outcome."""
import collections
import struct

import pytest

import bcf_files as BCF
import fuzz_records as FZ


@pytest.fixture(scope="module")
def outcomes():
    out = {}
    for fmt in FZ.FORMATS:
        rows = []
        for seed in FZ.SEEDS:
            for m, data in enumerate(FZ.case(fmt, seed)):
                try:
                    rows.append((seed, m, FZ.reference(fmt, data)))
                except Exception as e:                                   # the reference is total: an error code, never an exception
                    raise AssertionError(f"the {fmt} reference raised on ({fmt}, {seed}, {m}): {e!r}") from e
        out[fmt] = rows
    return out


@pytest.mark.parametrize("fmt", FZ.FORMATS)
def test_inputs_are_worth_running(outcomes, fmt):
    rows = outcomes[fmt]
    by_code = collections.Counter(o.code for _, _, o in rows)
    print(f"\n{fmt}: {len(rows)} inputs; " + ", ".join(f"{'clean' if c == 0 else 'error %d' % c}: {n}" for c, n in sorted(by_code.items())))
    failing = [o for _, _, o in rows if o.error]
    in_front = sum(1 for o in failing if o.rows)
    print(f"{fmt}: {in_front} of {len(failing)} failing inputs have rows in front of the error")
    assert not [c for c in FZ.error_codes(fmt) if not by_code[c]], "record errors that no input produces"
    assert by_code[0] * 10 >= len(rows), "fewer than 10 % of the inputs are clean"
    assert in_front * 2 >= len(failing), "fewer than half of the failing inputs have rows in front of the error"


def test_cases_are_reproducible():
    for fmt in FZ.FORMATS:
        assert FZ.case(fmt, 5) == FZ.case(fmt, 5) and FZ.case(fmt, 5) != FZ.case(fmt, 6)


def test_bases_cross_tiles_mid_record():
    bam, bcf = FZ.bam_base(), FZ.bcf_base()
    assert 5 * FZ.TILE <= sum(map(len, bam)) < 200_000 and FZ.TILE not in FZ.offsets_of(bam)     # the second tile begins mid-record
    assert 2 * FZ.TILE <= sum(map(len, bcf)) < 200_000 and FZ.TILE not in FZ.offsets_of(bcf)     # at least 3 tiles
    for fmt in ("bed", "sam"):
        for k in range(4):
            assert all(len(d) > FZ.TILE for d in FZ.super_tile_case(fmt, k))


def test_two_fault_records_occur_in_both_orders(outcomes):
    """among the BCF inputs are records with an INFO fault in front of a FORMAT fault and records with two INFO faults: the
    reference reports the left one, and both a reserved value in front of a bad key and the reverse occur"""
    seen = collections.Counter()
    for seed in FZ.SEEDS:
        data = FZ.case("bcf", seed)[3]
        o = FZ.reference("bcf", data)
        if o.error:
            seen[o.error[1]] += 1
    assert len(seen) >= 4, seen


def test_type_0_with_a_count_renders_as_a_dot():
    """a value of type 0 has no data whatever its count says: ID, an allele and a sample's value render as `.`,
    an INFO value as the flag"""
    import test_bcf_gpu as T
    text = T.header(samples=T.SAMPLES3)
    strings, contigs, n_samples = BCF.dictionaries(text)
    k = lambda name: T.K(text, name)
    rec = bytearray(BCF.record(chrom=1, pos=9, id_=b"abc", alleles=(b"A", b"C"), info=[(k("DP"), BCF.raw_value(0, 3, b""))], n_sample=3,
                               fmt=[(k("GQ"), [BCF.raw_value(0, 2, b"") for _ in range(3)])]))
    r = BCF.Rendered(bytes(rec), strings, contigs, n_samples)
    assert r.error is None and r.lines == [b"chr2\t10\tabc\tA\tC\t.\t.\tDP\tGQ\t.\t.\t."]
    assert rec[32] == 0x37
    rec[32] = 0x30                                                        # the ID: type 0, count 3 — its three bytes are the next values now
    r = BCF.Rendered(bytes(rec), strings, contigs, n_samples)
    assert r.error is not None or r.lines[0].split(b"\t")[2] == b"."
    one = bytearray(BCF.record(chrom=0, pos=0, id_=b"", alleles=(b"A",)))
    assert one[32] == 0x07 and one[33] == 0x17
    one[33] = 0x10                                                        # REF: type 0, count 1, and no byte of data
    l_shared = struct.unpack_from("<I", one, 0)[0]
    struct.pack_into("<I", one, 0, l_shared - 1)
    del one[34]
    r = BCF.Rendered(bytes(one), *BCF.dictionaries(T.header()))
    assert r.error is None and r.lines == [b"c1\t1\t.\t.\t.\t.\t.\t."]
