"""exg_gff_attributes on the device against the oracle tests/gff_attr_ref.py (the reference's gff_parse_attributes restated on
bytes): the list entries, and keys and values BIT-EXACT as string_t — up to 12 bytes inlined and zero padded, longer ones {length,
prefix, the input row's pointer + start} —, for a failing column the lowest failing row with the leftmost failing segment's offset
and length.  Shapes around the 64-byte word seam, row counts around a wave and a chunk, the row map, the two-call capacity
protocol, the reference's two files, the refusals, determinism and a fuzz."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import gff_attr_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gff")
EXPECTED = json.load(open(os.path.join(GOLDEN, "expected_gff_attributes.json")))
BASE = 1 << 44


def string_column(fields, base=BASE):
    """fields -> ([n, 16] uint8 string_t rows, payload bytes, each row's pointer or None): up to 12 bytes inlined, longer ones at
    base + offset"""
    rows = np.zeros((max(len(fields), 1), 16), np.uint8)
    payload = bytearray(b"front-pad")                       # (offsets that are no multiple of anything)
    ptrs = []
    for i, f in enumerate(fields):
        rows[i, :4] = np.frombuffer(len(f).to_bytes(4, "little"), np.uint8)
        if len(f) <= 12:
            rows[i, 4:4 + len(f)] = np.frombuffer(f, np.uint8)
            ptrs.append(None)
        else:
            rows[i, 4:8] = np.frombuffer(f[:4], np.uint8)
            ptrs.append(base + len(payload))
            rows[i, 8:16] = np.frombuffer(ptrs[-1].to_bytes(8, "little"), np.uint8)
            payload += f
    return rows, bytes(payload) + b"\0" * 16, ptrs


def token(field, ptr, start, length):
    """the string_t of field[start : start + length], a slice of the row at ptr (None: an inlined row)"""
    if length <= 12:
        return length.to_bytes(4, "little") + field[start:start + length].ljust(12, b"\0")
    assert ptr is not None, "a token of an inlined row is inlined"
    return length.to_bytes(4, "little") + field[start:start + 4] + (ptr + start).to_bytes(8, "little")


def run(fields, row_map=None, chunk_rows=0, capacity=None):
    import torch
    from exon_duckdb_amd import device
    rows, payload, _ = string_column(fields)
    col = torch.from_numpy(rows).cuda().view(torch.int64)
    pay = device.upload(payload)
    rm = torch.tensor(row_map, dtype=torch.int32).cuda() if row_map is not None else None
    n = len(fields) if row_map is None else len(row_map)
    ent, keys, vals, bases, r = device.gff_attributes(col, n, pay, BASE, entries_capacity=capacity, row_map=rm, chunk_rows=chunk_rows)
    raw = lambda t: t.cpu().numpy().view(np.uint8).reshape(-1, 16) if len(t) else np.zeros((0, 16), np.uint8)
    return ent.cpu().numpy().astype(np.uint64), raw(keys), raw(vals), bases, r


def check(fields, chunk_rows=0):
    """a column against the oracle: the lowest failing row with its segment, then (through a row map of the rows that parse)
    every entry bit for bit -> the oracle's spans per row (None: the row fails)"""
    from exon_duckdb_amd import ExgError, abi
    want, first_bad = [], None
    for i, f in enumerate(fields):
        try:
            want.append(R.spans(f))
        except R.AttributeError_ as e:
            want.append(None)
            if first_bad is None:
                first_bad = (i, e.offset, e.length)
    if first_bad is not None:
        with pytest.raises(ExgError) as e:
            run(fields)
        r = e.value.result
        assert (r.error_row, r.error_offset, r.error_length, r.error_code) == first_bad + (abi.EXG_PE_GFF_ATTRIBUTES,), (
            first_bad, r.error_row, r.error_offset, r.error_length, fields[first_bad[0]])
        assert e.value.code == abi.EXG_E_PARSE and f"Invalid GFF attribute in row {first_bad[0]} at byte {first_bad[1]}" in str(e.value)
    good = [i for i, w in enumerate(want) if w is not None]
    ent, keys, vals, bases, r = run(fields, row_map=good if first_bad is not None else None, chunk_rows=chunk_rows)
    _, _, ptrs = string_column(fields)
    total = sum(len(want[i]) for i in good)
    assert r.error_code == 0 and r.flags == 0 and r.total_entries == total == len(keys) == len(vals) and r.n_rows == len(good)
    want_keys = b"".join(token(fields[i], ptrs[i], k, kn) for i in good for k, kn, _, _ in want[i])
    want_vals = b"".join(token(fields[i], ptrs[i], v, vn) for i in good for _, _, v, vn in want[i])
    if keys.tobytes() != want_keys or vals.tobytes() != want_vals:
        at = 0
        for j, i in enumerate(good):
            for k, kn, v, vn in want[i]:
                assert keys[at].tobytes() == token(fields[i], ptrs[i], k, kn), ("key", j, i, fields[i], k, kn, keys[at].tobytes())
                assert vals[at].tobytes() == token(fields[i], ptrs[i], v, vn), ("value", j, i, fields[i], v, vn, vals[at].tobytes())
                at += 1
    off, chunk_start, starts = 0, 0, []
    for j, i in enumerate(good):
        if chunk_rows and j % chunk_rows == 0:
            chunk_start = off
            starts.append(off)
        assert (int(ent[j, 0]), int(ent[j, 1])) == (off - chunk_start, len(want[i])), (j, i)
        off += len(want[i])
    if chunk_rows:
        assert bases.cpu().numpy().tolist() == starts + [total]
    return want


def pairs(fields, want):
    return [[(f[k:k + kn], f[v:v + vn]) for k, kn, v, vn in w] for f, w in zip(fields, want)]


def seam_field(n):
    """a field of exactly n bytes that parses (n >= 3): `k=vvv...`"""
    return b"k=" + b"v" * (n - 2)


# ---------------------------------------------------------------- seams and shapes
def test_fields_of_0_1_12_13_63_64_65_128_and_200_bytes(gpu):
    sizes = (12, 13, 63, 64, 65, 128, 200, 4, 127, 129)
    fields = [seam_field(n) for n in sizes] + [seam_field(n - 1) + b";" for n in sizes]
    assert [len(f) for f in fields] == list(sizes) * 2
    want = check(fields)
    assert pairs(fields, want)[6] == [(b"k", b"v" * 198)]
    check([b"", seam_field(64)])            # 0 bytes: the field is its own segment, and fails
    check([seam_field(64), b"a"])           # 1 byte: no `=`
    check([seam_field(64), b";"])


def test_semicolon_and_equals_at_byte_63_and_64(gpu):
    fields = []
    for at in (62, 63, 64, 65):
        fields.append(b"k=" + b"v" * (at - 2) + b";x=y")            # `;` at byte `at`
        fields.append(b"k" * at + b"=v;x=y")                        # `=` at byte `at`
        fields.append(b"a=b;" + b"k" * (at - 4) + b"=" + b"v" * 70)     # ... in the second entry, the value two words long
        assert fields[-3][at] == 0x3B and fields[-2][at] == 0x3D and fields[-1][at] == 0x3D
    want = check(fields)
    assert all(len(w) == 2 for w in want)


def test_blanks_in_front_of_and_behind_a_semicolon_across_the_seam(gpu):
    blanks = b" \t \r \n\v\f "                                      # nine bytes: 60 .. 68
    front = b"k=" + b"v" * 58 + blanks + b";x=y"
    behind = b"k=" + b"v" * 57 + b";" + blanks + b"x=y"
    assert front[60:69] == blanks and front[69] == 0x3B and behind[59] == 0x3B and behind[60:69] == blanks
    inner = b"k=" + b"v" * 58 + blanks + b"w;x=y"                   # blanks inside a value stay
    fields = [front, behind, inner, b"k=" + b"v" * 58 + blanks, blanks * 8 + b"k=v" + blanks * 8, b"k=" + b"v" * 58 + b"=" + blanks + b";x=y"]
    want = pairs(fields, check(fields))
    assert want[0] == [(b"k", b"v" * 58), (b"x", b"y")] and want[1] == [(b"k", b"v" * 57), (b"x", b"y")] and want[2][0] == (b"k", b"v" * 58 + blanks + b"w")
    assert want[3] == [(b"k", b"v" * 58)] and want[4] == [(b"k", b"v")] and want[5] == want[0]
    # the same runs around a segment that fails: offset and length are the trimmed segment's
    check([front, b"a=b;" + b" " * 58 + b"x" + blanks + b";y=z"])
    check([front, b"a=b;" + b" " * 70 + b";y=z"])
    check([front, b"k=" + b"v" * 58 + b"=" + blanks + b"w"])        # the blanks become a third piece once a byte follows them


def test_double_equals_astride_the_seam_and_a_value_that_ends_at_byte_63(gpu):
    fields = [b"k" * 63 + b"==v", b"k" * 62 + b"==v", b"k" * 64 + b"==v", b"k" * 61 + b"===" + b"v" * 70 + b"=",
              b"k=" + b"v" * 62,                                     # the value's last byte is byte 63: the field's end is the virtual `;` of the next word
              b"k=" + b"v" * 126, b"k=" + b"v" * 61 + b";", b"a=b;k=" + b"v" * 58]
    assert fields[0][63:65] == b"==" and len(fields[4]) == 64 and len(fields[7]) == 64
    want = pairs(fields, check(fields))
    assert want[0] == [(b"k" * 63, b"v")] and want[4] == [(b"k", b"v" * 62)] and want[3] == [(b"k" * 61, b"v" * 70)]


def test_keys_of_12_and_13_bytes_and_tokens_of_an_inlined_row(gpu):
    fields = [b"k" * 12 + b"=" + b"v" * 12, b"k" * 13 + b"=" + b"v" * 13, b"abcde=fghijk", b"a=b;c=d;e=f", b" a=b ;", b"k" * 12 + b"=v"]
    assert [len(f) for f in fields[2:5]] == [12, 11, 6]
    rows, _, ptrs = string_column(fields)
    assert ptrs[2] is None and ptrs[3] is None and ptrs[4] is None and ptrs[0] is not None
    want = check(fields)                                            # (token() refuses a pointer into an inlined row)
    assert [len(w) for w in want] == [1, 1, 1, 3, 1, 1]


def test_70_entries_in_one_row_and_a_row_of_semicolons_beside_good_rows(gpu):
    many = b"a=b;" * 70
    want = check([seam_field(20), many, b";;;", seam_field(70), many[:-1], b"a=b;" * 16 + b"c"])
    assert [None if w is None else len(w) for w in want] == [1, 70, None, 1, 70, None]


# ---------------------------------------------------------------- row counts and maps
@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_row_counts_around_a_wave(gpu, n):
    rng = R.random.Random(n)
    fields = [b"ID=r%d;Parent=p%d ; note=%s" % (i, i, b"x" * rng.randrange(1, 90)) for i in range(n)]
    want = check(fields)
    assert len(want) == n
    if n == 0:
        ent, keys, vals, bases, r = run([], chunk_rows=8)
        assert r.total_entries == 0 and r.n_rows == 0 and r.error_code == 0 and bases.cpu().numpy().tolist()[0] == 0


def test_2049_rows_in_chunks_of_2048(gpu):
    rng = R.random.Random(7)
    fields = [b";".join(b"k%d=%s" % (j, b"v" * rng.randrange(1, 30)) for j in range(rng.randrange(1, 5))) for _ in range(2049)]
    check(fields, chunk_rows=2048)                                  # three chunk_base words; row 2048's offset is 0 again


def test_a_row_map_that_reverses_and_repeats_rows(gpu):
    fields = [b"ID=r%d;n=%s" % (i, b"v" * (i * 3 + 1)) for i in range(40)] + [b"broken"]
    row_map = list(range(39, -1, -1)) + [3, 3, 17, 0, 39, 3]
    ent, keys, vals, _, r = run(fields, row_map=row_map)           # (row 40 is not in the map: it is never read)
    _, _, ptrs = string_column(fields)
    want = [R.spans(fields[i]) for i in row_map]
    assert r.error_code == 0 and r.n_rows == len(row_map) and r.total_entries == 2 * len(row_map)
    assert keys.tobytes() == b"".join(token(fields[i], ptrs[i], k, kn) for i, w in zip(row_map, want) for k, kn, _, _ in w)
    assert vals.tobytes() == b"".join(token(fields[i], ptrs[i], v, vn) for i, w in zip(row_map, want) for _, _, v, vn in w)
    assert ent.tolist() == [[2 * j, 2] for j in range(len(row_map))]
    from exon_duckdb_amd import ExgError
    with pytest.raises(ExgError) as e:
        run(fields, row_map=[5, 40, 2, 40])
    assert (e.value.result.error_row, e.value.result.error_offset, e.value.result.error_length) == (1, 0, 6)      # an index of the call's rows


# ---------------------------------------------------------------- capacity
def test_the_two_call_capacity_protocol_keeps_a_canary_untouched(gpu):
    import torch
    from exon_duckdb_amd import abi, device, load_library
    lib = load_library()
    fields = R.fuzz_fields(5, 600)
    fields = [f for f in fields if R.outcome(f)[0] == "ok"]
    want = [R.spans(f) for f in fields]
    total = sum(len(w) for w in want)
    assert len(fields) > 200 and total > len(fields)
    rows, payload, ptrs = string_column(fields)
    col, pay = torch.from_numpy(rows).cuda().view(torch.int64), device.upload(payload)
    n = len(fields)
    ws_bytes = int(lib.exg_gff_attributes_workspace_bytes(n))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device="cuda")
    result = torch.empty(8, dtype=torch.int64, device="cuda")
    entries = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    keys = torch.full((total, 2), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    vals = torch.full((total, 2), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    a = abi.GffAttributesArgs()
    a.d_strings, a.d_payload, a.payload_base, a.n_rows = col.data_ptr(), pay.data_ptr(), BASE, n
    a.d_workspace, a.workspace_bytes, a.d_result, a.stream = ws.data_ptr(), ws_bytes, result.data_ptr(), device.stream_ptr().value

    def call():
        device.check(lib.exg_gff_attributes(C.byref(a)))
        r = abi.GffAttributesResult()
        device.check(lib.exg_gff_attributes_result(C.c_void_p(result.data_ptr()), device.stream_ptr(), C.byref(r)))
        return r

    r = call()                                                      # the counting call: no capacity, NULL children
    assert r.total_entries == total and r.flags & abi.EXG_RF_CAPACITY and r.error_code == 0 and r.n_rows == n
    a.d_out_entries, a.d_out_keys, a.d_out_values, a.entries_capacity = entries.data_ptr(), keys.data_ptr(), vals.data_ptr(), total - 1
    r = call()                                                      # one short: exact total, the children keep the canary
    assert r.total_entries == total and r.flags & abi.EXG_RF_CAPACITY and r.error_code == 0
    assert bool((keys == 0x5A5A5A5A5A5A5A5A).all()) and bool((vals == 0x5A5A5A5A5A5A5A5A).all())
    a.entries_capacity = total
    r = call()
    assert r.total_entries == total and r.flags == 0
    got = keys.cpu().numpy().view(np.uint8).tobytes()
    assert got == b"".join(token(f, p, k, kn) for f, p, w in zip(fields, ptrs, want) for k, kn, _, _ in w)
    assert entries.cpu().numpy()[:, 1].tolist() == [len(w) for w in want]


# ---------------------------------------------------------------- errors
R3_ERRORS = [b"a", b"a=", b"=a", b"a=b=c", b"a= =b", b"   ", b"", b";", b"x=y;" + b" " * 70 + b"k" * 70 + b"  ;z=w", b"x=y;k=" + b"v" * 80 + b"=w"]


@pytest.mark.parametrize("k", range(len(R3_ERRORS)))
def test_every_error_form_on_the_first_a_middle_and_the_last_row(gpu, k):
    good = [b"ID=r%d; Parent=p%d;note=%s" % (i, i, b"n" * (i % 77)) for i in range(130)]
    bad = R3_ERRORS[k]
    assert R.outcome(bad)[0] == "error"
    for at in (0, 70, 129):
        fields = list(good)
        fields[at] = bad
        if at != 129:
            fields[at + 30] = R3_ERRORS[(k + 1) % len(R3_ERRORS)]      # a later failing row does not win
        want = check(fields)
        assert want[at] is None
    # in a segment among good ones, and two failing segments in one row: the leftmost wins
    if bad not in (b"", b";"):
        fields = list(good)
        fields[5] = b"p=q;" + bad + b";r=s; zz ;t=u" if b";" not in bad else bad + b"; zz "
        check(fields)
        fields[5] = b"p=q; zz ;" + bad
        want = check(fields)
        assert want[5] is None and R.outcome(fields[5]) == ("error", 5, 2)


# ---------------------------------------------------------------- the reference's files
def test_gtf_scan_over_test_gff_then_the_attributes_of_its_ninth_column(gpu):
    from exon_duckdb_amd import abi, device
    data = open(os.path.join(GOLDEN, "test.gff"), "rb").read()
    rows = EXPECTED["files"]["test.gff"]
    d_in = device.upload(data)
    scan = device.GtfScan(len(data), capacity_records=len(rows))
    scan.launch(d_in, algo=abi.EXG_ALGO_FUSED_FULL)
    res = scan.fetch()
    assert res.n_records == len(rows) == 2 and res.error_code == 0
    ent, keys, vals, _, r = device.gff_attributes(scan.cols[8], len(rows), d_in, scan.PAYLOAD_BASE)
    assert r.error_code == 0 and r.total_entries == 4

    def strings(t):
        out = []
        for row in t.cpu().numpy().view(np.uint8).reshape(-1, 16):
            ln = int.from_bytes(row[:4].tobytes(), "little")
            if ln <= 12:
                out.append(row[4:4 + ln].tobytes().decode())
            else:
                o = int.from_bytes(row[8:16].tobytes(), "little") - scan.PAYLOAD_BASE
                assert 0 <= o and o + ln <= len(data) and data[o:o + 4] == row[4:8].tobytes()
                out.append(data[o:o + ln].decode())
        return out
    flat = list(zip(strings(keys), strings(vals)))
    ent = ent.cpu().numpy()
    assert [[list(kv) for kv in flat[int(o):int(o) + int(n)]] for o, n in ent] == [row["entries"] for row in rows]


def test_the_ninth_fields_of_raw_test_gff_as_a_string_column(gpu):
    rows = EXPECTED["files"]["raw-test.gff"]
    fields = [row["field"].encode() for row in rows]
    want = pairs(fields, check(fields))
    assert [[[k.decode(), v.decode()] for k, v in w] for w in want] == [row["entries"] for row in rows]
    assert len(fields) == 10 and sum(len(w) for w in want) == 20


# ---------------------------------------------------------------- refusals, determinism, fuzz
def test_bad_arguments_return_invalid_arg_without_a_launch(gpu):
    import torch
    from exon_duckdb_amd import abi, load_library
    lib = load_library()
    n = 4
    ws_bytes = int(lib.exg_gff_attributes_workspace_bytes(n))
    buf = torch.zeros(ws_bytes // 8 + 64, dtype=torch.int64, device="cuda")
    result = torch.full((8,), 0x77, dtype=torch.int64, device="cuda")

    def complete(rows=n):
        a = abi.GffAttributesArgs()
        a.d_strings, a.d_payload, a.n_rows = buf.data_ptr(), buf.data_ptr(), rows
        a.d_workspace, a.workspace_bytes, a.d_result = buf.data_ptr() + 512, ws_bytes, result.data_ptr()
        return a
    cases = []
    a = complete(); a.d_strings = None; cases.append(a)
    a = complete(); a.d_strings = buf.data_ptr() + 8; cases.append(a)
    a = complete(); a.workspace_bytes = ws_bytes - 1; cases.append(a)
    a = complete(); a.chunk_rows = 2048; cases.append(a)
    a = complete((1 << 32) - 1); a.workspace_bytes = 1 << 40; cases.append(a)
    for a in cases:
        assert lib.exg_gff_attributes(C.byref(a)) == abi.EXG_E_INVALID_ARG
    torch.cuda.synchronize()
    assert bool((result == 0x77).all())                             # nothing ran: the result block was never written


def test_the_same_input_twice_gives_byte_identical_outputs(gpu):
    fields = [f for f in R.fuzz_fields(9, 1500) if R.outcome(f)[0] == "ok"]
    outs = []
    for _ in range(2):
        ent, keys, vals, bases, r = run(fields, chunk_rows=256)
        outs.append((ent.tobytes(), keys.tobytes(), vals.tobytes(), bases.cpu().numpy().tobytes(), bytes(r)))
    assert outs[0] == outs[1] and len(outs[0][1]) > 16 * len(fields)


@pytest.mark.parametrize("seed", range(4))
def test_fuzz_against_the_oracle(gpu, seed):
    fields = R.fuzz_fields(100 + seed, 2000)
    want = check(fields)
    ok = sum(w is not None for w in want)
    print(f"seed {seed}: {ok} of {len(fields)} fields parse")
    assert ok >= len(fields) * R.VALID_SHARE and len(fields) - ok >= len(fields) // 5
