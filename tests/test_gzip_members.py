"""The gzip / BGZF member writer of tests/gzip_members.py held to account (no GPU): every case of its catalogue through the oracle's
decoder rules (zlib), and through the host's own framing walk, exg_gzip_index."""
import ctypes as C

import numpy as np
import pytest

import gzip_members as gm
from exon_duckdb_amd import abi


def test_the_catalogue_reaches_every_required_form():
    v, i = gm.valid(), gm.invalid()
    tags = set().union(*(c.tags for c in list(v.values()) + list(i.values())))
    assert gm.REQUIRED_TAGS <= tags, sorted(gm.REQUIRED_TAGS - tags)
    assert len(v) >= 80 and len(i) >= 240
    g = gm.groups()
    assert set(g) == set(gm.GROUP_NAMES) and sum(len(x) for x in g.values()) == len(v) + len(i)
    for c in list(v.values()) + list(i.values()):
        assert c.clause and c.tags, c.name
        if c.name not in ("straddles_256k_window", "straddles_256k_window_small_segments") and "big" not in c.name:
            assert len(c.text) < 70_000, c.name            # payloads are small unless the case is about size


def test_valid_cases_decode_to_their_text_by_the_oracles_rules(oracle):
    for name, c in gm.valid().items():
        text, err = oracle.decode_by_rule(c.data, "gzip")
        assert err is None, (name, err)
        assert text == c.text, (name, len(text), len(c.text))
        assert c.text == b"".join(p.payload for p in c.parts), name


def test_invalid_cases_are_errors_behind_their_prefix_by_the_oracles_rules(oracle):
    """... but for the rule differences the catalogue names: `bsize_binds` (zlib reads the file: it never looks at BSIZE),
    `partial` (zlib has handed out a part of the member the error lies in) and `streamed` (the reader hands out a big member's
    rows before its trailer's error)"""
    seen = set()
    for name, c in gm.invalid().items():
        text, err = oracle.decode_by_rule(c.data, "gzip")
        seen.add(c.differs)
        if c.differs == "bsize_binds":
            assert err is None and text.startswith(c.text) and len(text) > len(c.text), (name, err)
            continue
        assert err is not None, name
        if c.differs == "partial":
            assert text.startswith(c.text), name
        elif c.differs == "streamed":
            assert c.text.startswith(text) and len(c.text) - len(text) > 100_000, name
        else:
            assert text == c.text, (name, text, c.text)
    assert seen == {None, "bsize_binds", "partial", "streamed"}


def walk(lib, data, start):
    """one exg_gzip_index call from `start`: -> (rc, [(comp_off, comp_size, out_cap)], open_ended)"""
    arr = np.frombuffer(data, np.uint8)
    cap = 4096
    members = (abi.InflateMember * cap)()
    n, total, open_ended = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
    rc = lib.exg_gzip_index(arr.ctypes.data, len(data), start, members, cap, C.byref(n), C.byref(total), C.byref(open_ended))
    return rc, [(members[i].comp_off, members[i].comp_size, members[i].out_cap) for i in range(n.value)], bool(open_ended.value)


@pytest.fixture(scope="module")
def lib():
    from exon_duckdb_amd import load_library
    return load_library()


def index_all(lib, c):
    """the caller's loop over exg_gzip_index (index, inflate the open-ended member, index again behind it) with the writer's own
    account of where every member ends in place of the inflate: -> error message or None.  Checks every member on the way."""
    pos, k, parts = 0, 0, c.parts
    while k < len(parts):
        rc, got, open_ended = walk(lib, c.data, pos)
        if rc:
            return lib.exg_last_error_message().decode()
        assert got, c.name
        for i, (comp_off, comp_size, out_cap) in enumerate(got):
            m = parts[k]
            assert isinstance(m, gm.Member), (c.name, k)
            assert comp_off == pos + m.hdr_len, (c.name, k, comp_off, pos + m.hdr_len)      # the first byte of the DEFLATE stream
            if m.sized:
                assert comp_size == len(m) - m.hdr_len and out_cap == m.isize, (c.name, k, comp_size, out_cap)
                assert not (open_ended and i == len(got) - 1), (c.name, k)
            else:
                assert open_ended and i == len(got) - 1, (c.name, k, "a member without BSIZE is the last of its call")
                assert comp_size == len(c.data) - comp_off and out_cap >= len(m.payload), (c.name, k)
            pos += len(m)
            k += 1
    assert pos == len(c.data), c.name
    return None


def test_index_finds_every_member_of_the_valid_cases(lib):
    for name, c in gm.valid().items():
        if name == "bc_twice_last_wins" or any(len(p) > 65536 and p.sized for p in c.parts):
            continue          # (asserted below: BSIZE is what the index goes by)
        assert index_all(lib, c) is None, name
    # two BC subfields: the last one counts
    c = gm.valid()["bc_twice_last_wins"]
    rc, got, open_ended = walk(lib, c.data, 0)
    assert rc == 0 and not open_ended and [g[1] for g in got] == [len(p) - p.hdr_len for p in c.parts]
    assert index_all(lib, gm.valid()["isize_65537_with_bc"]) is None          # a BSIZE the index takes, whatever ISIZE says


def test_index_refuses_what_zlib_refuses_in_the_header(lib):
    refused = 0
    for name, c in gm.invalid().items():
        if not c.refused_by_index:
            continue
        # members in front of the bad one are indexed as usual (index_all checks them), the call that reaches it fails
        parts = c.parts
        msg, pos, k = None, 0, 0
        while msg is None and pos < len(c.data):
            rc, got, open_ended = walk(lib, c.data, pos)
            if rc:
                msg = lib.exg_last_error_message().decode()
                break
            for comp_off, comp_size, out_cap in got:
                assert isinstance(parts[k], gm.Member) and comp_off == pos + parts[k].hdr_len, (name, k)
                pos += len(parts[k])
                k += 1
        assert msg and ("gzip" in msg), (name, msg)
        refused += 1
    assert refused >= 40
    for name in ("bad_fhcrc", "bad_flg_bit5", "bad_flg_bit6", "bad_flg_bit7", "bad_cm7", "bad_id2"):
        assert gm.invalid()[name].refused_by_index


def test_index_walks_the_cases_whose_headers_are_valid(lib):
    """a wrong trailer, slack in front of it, a member cut behind its header: nothing the framing walk can see — it finds the
    DEFLATE streams where they are (a wrong ISIZE is the out_cap it reports).  The BSIZE cases are left out: BSIZE is what the
    walk goes by, so it reports the sizes BSIZE states"""
    n = 0
    for name, c in gm.invalid().items():
        if c.refused_by_index or c.differs == "bsize_binds":
            continue
        assert index_all(lib, c) is None, name
        n += 1
    assert n >= 60


def test_index_takes_fhcrc_and_long_headers(lib):
    for name in ("hdr_combo_08", "hdr_combo_15", "hdr_longer_than_70000", "hdr_xlen_65535", "hdr_fname_latin1_300"):
        assert index_all(lib, gm.valid()[name]) is None, name
