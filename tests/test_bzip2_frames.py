"""The bzip2 writer of tests/bzip2_frames.py proved against libbz2 (Python's bz2) before it judges the device: every
catalogue stream and valid generator seed decodes under libbz2 to the bytes the writer's model gives, libbz2 refuses every
invalid stream (the recorded differences of bz2.decompress aside), the catalogue holds every form its list names, the
period-5 columns enter their five RLE1 pieces in five states, the blocks begin at all eight bit phases, and the reader's
hand-built file puts a stream header, an end magic, a CRC and the padding behind it on window edges."""
import bz2
import random

import pytest

import bzip2_frames as F

SEEDS = list(range(40))
WINDOWS = (512, 1024, 4096, 65536, None)     # EXG_BZIP2_WINDOW_BYTES (None: unset)
MAX_BLOCKS = (1, None)                       # EXG_STREAM_ROUND_OUT at its floor / unset


def libbz2(data):
    try:
        return bz2.decompress(data)
    except (OSError, ValueError, EOFError):
        return None


def bzip2_program(data):
    """libbz2 stream by stream under the rule of the bzip2 program (bzip2.c, uncompressStream): behind a good stream only
    bytes that do not begin a stream header are dropped; anything that fails behind a header is an error.  -> bytes | None"""
    out, first = b"", True
    while data:
        head = data == b"BZh"[:len(data)] if len(data) < 4 else data[:3] == b"BZh" and data[3] in b"123456789"
        if not first and not head:
            break
        d = bz2.BZ2Decompressor()
        try:
            out += d.decompress(data)
        except (OSError, ValueError):
            return None
        if not d.eof:
            return None
        data, first = d.unused_data, False
    return out


def old_libbz2_refuses_surplus_selectors():
    """libbz2 before 1.0.8 refuses more than 18002 selectors: then it refuses exactly those entries, and only they may skip"""
    over = [n for n in F.catalogue() if n in ("selectors_18003_written", "selectors_32767_written")]
    assert len(over) == 2
    return all(libbz2(F.catalogue()[n][0]) is None for n in over)


@pytest.mark.parametrize("name", sorted(F.catalogue()))
def test_catalogue_stream_decodes_to_expected(name):
    s, want = F.catalogue()[name]
    if name in ("selectors_18003_written", "selectors_32767_written") and old_libbz2_refuses_surplus_selectors():
        pytest.skip("libbz2 < 1.0.8 refuses more than 18002 selectors")
    assert libbz2(s) == want, name
    assert bzip2_program(s) == want, name


def test_generator_seeds_decode_to_expected_and_nine_in_ten_are_valid():
    valid = 0
    for seed in SEEDS:
        s, want, reason = F.generate(seed)
        assert libbz2(s) == want, seed            # (None == None: a column that ends where a count is due is refused)
        assert (want is None) == (reason == F.R_RUN_AT_END), seed
        valid += want is not None
    assert 10 * valid >= 9 * len(SEEDS), (valid, len(SEEDS))
    assert F.generate(7) == F.generate(7)


def test_invalid_streams_are_refused():
    inv = F.invalid()
    whole, cut_ok, first = F.truncation_stream()
    assert 250 <= len(whole) <= 400 and sum(n.startswith("truncated_at_") for n in inv) == len(whole) - 2
    assert libbz2(whole[:cut_ok]) == first and "truncated_at_%d" % cut_ok not in inv    # the one valid cut
    for name, (s, reason, clause) in inv.items():
        assert bzip2_program(s) is None, (name, clause)
        assert (libbz2(s) is None) != (name in F.PYTHON_ACCEPTS), (name, clause)
    # the recorded differences: bz2.decompress drops what fails behind a good first stream
    for name in F.PYTHON_ACCEPTS:
        assert libbz2(inv[name][0]) == bz2.decompress(inv[name][0][:len(F.stream([F.data_block(b"block %d of four\n" % k) for k in range(2)], 5)[0])])


def test_invalid_reasons_are_the_decoders_wording():
    """every reason but the three the host words itself is a string of reason_text (exg_bzip2.hip)"""
    import os
    src = open(os.path.join(os.path.dirname(__file__), "..", "exon_duckdb_amd", "csrc", "exg_bzip2.hip")).read()
    table = src[src.index("const char *reason_text"):src.index("struct CandOut")]
    seen = set()
    for name, (s, reason, clause) in F.invalid().items():
        if reason in (F.R_TRUNCATED, F.R_NOT_BZIP2, "stream CRC mismatch"):
            continue
        assert reason in table, (name, reason)
        seen.add(reason)
    assert len(seen) >= 13, sorted(seen)       # all of reason_text but "inconsistent BWT mapping" (no stream reaches it)


def test_catalogue_holds_every_form():
    names = set(F.catalogue())
    inv = set(F.invalid())
    want = ["geometry_nblock_%d" % n for n in F.NBLOCKS] + list(F.period5_columns())
    want += ["run_at_piece_boundary_count_%d" % c for c in (0, 1, 255, 0x41)]
    want += ["run_count0_run_count2", "run_count_then_byte_equal_to_count", "run_count_then_byte_equal_to_run"]
    want += ["groups_%d_on_40_and_5000_symbols" % g for g in (2, 3, 4, 5, 6)]
    want += ["unused_tables_with_odd_lengths", "table_1_to_20_to_1", "codes_of_9_10_11_12_bits_in_one_table", "table_minlen_11", "table_minlen_15",
             "table_all_lengths_20", "incomplete_codes", "oversubscribed_table_in_use", "oversubscribed_table_unused"]
    want += ["selectors_exactly_as_needed", "selectors_one_surplus", "selectors_18002_written", "selectors_18003_written", "selectors_32767_written",
             "selector_mtf_index_last_at_every_group_of_2", "selector_mtf_index_last_at_every_group_of_6"]
    want += ["symbols_%d_with_end_of_block" % k for k in (49, 50, 51, 100)]
    want += ["run_at_block_start", "runs_of_1_2_3_4_and_powers_of_two_to_65536", "block_of_one_run", "mtf_index_255_all_256_values", "nblock_100000_at_level_1",
             "symbol_map_only_byte_0", "symbol_map_only_byte_255", "symbol_map_one_sixteen", "symbol_map_all_256", "symbol_map_sixteen_set_but_empty"]
    want += ["header_level_%d" % k for k in range(1, 10)]
    want += ["empty_stream_in_front", "empty_stream_in_the_middle", "empty_stream_at_the_end", "level_1_then_level_9_with_nblock_100001",
             "level_9_with_nblock_100001_then_level_1", "trailing_1_byte", "trailing_2_bytes", "trailing_3_bytes", "trailing_16_bytes_no_header",
             "trailing_64_zero_bytes", "false_block_magic_five_times", "false_end_of_stream_magic_five_times", "false_block_magic_in_front_of_the_end_magic"]
    assert not set(want) - names, sorted(set(want) - names)
    assert sum(n.startswith("cycle_") for n in names) == 2
    want = ["symbol_map_empty", "ngroups_0", "ngroups_1", "ngroups_7", "nselectors_0", "selector_unary_run_reaches_ngroups", "code_length_start_0",
            "code_length_start_21", "code_length_delta_reaches_0", "code_length_delta_reaches_21_and_returns", "symbol_matches_no_code_by_20_bits",
            "symbols_past_the_last_selector", "run_weight_reaches_2_21", "end_of_block_first", "origptr_equals_nblock", "origptr_2_24_minus_1",
            "block_ends_where_a_count_is_due", "block_crc_wrong_in_block_0", "block_crc_wrong_in_block_2_of_4", "stream_crc_wrong_in_stream_2_of_3",
            "randomised_block", "garbage_where_the_next_block_magic_is_due", "header_BZh0", "header_BZh_colon", "header_BZg9",
            "good_stream_then_header_and_garbage"]
    want += ["nblock_over_the_limit_by_%s_level_%d" % (how, lv) for how in ("a_run", "one_symbol") for lv in (1, 2)]
    assert not set(want) - inv, sorted(set(want) - inv)


def test_period5_columns_enter_their_pieces_in_five_states():
    for name, (L, orig) in F.period5_columns().items():
        pre = F.lf_walk(L, orig)
        assert len(set(pre)) == 1 and pre[0] == L[0]
        states = F.piece_states(pre)
        assert len(states) >= 5 and sorted(states[:5]) == [0, 1, 2, 3, 4], (name, states)


def test_cycle_entries_do_not_divide_nblock():
    r = random.Random(1)
    for name in F.catalogue():
        if name.startswith("cycle_"):
            cyc, n = int(name.split("_")[1]), int(name.split("_")[-1])
            assert 1 < cyc < n and n % cyc, name
    # the model itself: a column's walk is its cycle repeated
    L = bytes(r.choice(b"ab") for _ in range(64))
    k = F.cycle_length(L, 9)
    pre = F.lf_walk(L, 9)
    assert pre == (pre[:k] * 64)[:64]


def test_real_blocks_begin_at_all_eight_bit_phases():
    phases = {o % 8 for offs in F.block_offsets().values() for o in offs}
    assert phases == set(range(8)), phases


def test_writer_pieces():
    r = random.Random(5)
    d = r.randbytes(3000) + b"A" * 700 + b"\xff" * 5
    assert F.crc(d) == F.crc_bytewise(d)
    assert F.unrle1(F.rle1(d)) == d
    w = F.Bits()
    ref = 0
    for _ in range(2000):
        k = r.randint(0, 40)
        x = r.getrandbits(k) if k else 0
        w.put(k, x)
        ref = (ref << k) | x
    assert w.bytes() == (ref << (-w.n % 8)).to_bytes((w.n + 7) // 8, "big")
    for alpha in (3, 6, 19, 258):
        lens = F.kraft_lengths(r, alpha)
        assert len(lens) == alpha and max(lens) <= 20 and sum(1 << (20 - x) for x in lens) == 1 << 20
    pre = b"xyAAAA\x03Az"
    assert F.lf_walk(**F.block_from_pre(pre)) == pre


def reader_rounds():
    data, text, layout = F.reader_file()
    return data, layout, {(w, m): F.rounds(data, layout, w if w else 1 << 20, m) for w in WINDOWS for m in MAX_BLOCKS}


def test_reader_file_puts_its_structures_on_window_edges():
    data, text, layout = F.reader_file()
    assert libbz2(data) == text
    n_blocks = sum(k == "block" for k, _, _ in layout)
    assert 36 <= n_blocks <= 46 and sum(k == "header" for k, _, _ in layout) == 4
    data, layout, rs = reader_rounds()
    cut = set()
    for (w, m), r in rs.items():
        assert sum(x["blocks"] for x in r) == n_blocks
        cut |= F.straddled(layout, r, len(data))
        if m == 1:
            assert all(x["blocks"] <= 1 for x in r)
    assert {"header", "end", "crc", "pad", "block"} <= cut, cut
    # a 512-byte window is smaller than every block: the window doubles until it holds one
    assert min(b - a for k, a, b in layout if k == "block") > 8 * 512
    assert max(x["grow"] for x in rs[(512, 1)]) >= 8
    assert len(rs[(None, None)]) == 1
