"""vcf_query on the host (no GPU): the tabix parser, the region grammar and the chunk planner behind exg_tabix_query held against the
independent Python implementation of tests/tabix_files.py — on the reference's own index (tests/golden/vcf-index/) and on generated
ones —, the Python index writer's conservativeness, bad indexes, the catalog and the bind-time refusals that need no device, the
ABI mirrors, and the sanitized stand-alone driver (tests/region_host_driver.cpp)."""
import ctypes as C
import gzip
import os
import random
import re
import shutil
import struct
import subprocess

import pytest

import tabix_files as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vcf-index")
FIXTURE = os.path.join(GOLDEN, "index.vcf.gz")
HEADER = os.path.join(ROOT, "include", "exon_gpu.h")


@pytest.fixture(scope="module")
def fixture_index():
    """the reference's .tbi, inflated with Python's gzip"""
    return gzip.open(FIXTURE + ".tbi").read()


@pytest.fixture(scope="module")
def generated():
    """seeded indexes over ~2 000 lines, several contigs (one named `chrX:1`), 4 KiB of text a member -> [(text, members, idx, bytes)]"""
    out = []
    for seed in (11, 12):
        text = T.synth_vcf(seed)
        _, members = T.bgzip(text, 4096)
        idx = T.build_index(text, members)
        out.append((text, members, idx, T.serialize_index(idx)))
    return out


def query(index_bytes, region):
    from exon_duckdb_amd import device
    return device.tabix_query(index_bytes, region)


def query_rc(index_bytes, region):
    from exon_duckdb_amd import abi, load_library
    lib = load_library()
    n = C.c_uint64(0)
    rc = lib.exg_tabix_query(index_bytes, len(index_bytes), region, None, 0, C.byref(n), C.byref(abi.Region()))
    return rc, lib.exg_last_error_message().decode()


# ---- the reference's index ---------------------------------------------------------------------------------------------------
def test_the_fixture_is_the_indexed_file_not_the_plain_one():
    assert os.path.getsize(FIXTURE) == 8638 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "vcf", "index.vcf.gz")) == 8277
    members = T.member_offsets(open(FIXTURE, "rb").read())
    assert len(members) == 3 and members[-1][1] == 0        # two data members and the end marker


def test_reference_index_names_and_linear_index_lengths(fixture_index):
    idx = T.read_index(fixture_index)
    assert idx["names"] == [b"1", b"2", b"10"] and idx["format"] == 2 and idx["n_no_coor"] == 0
    assert [len(r["ioff"]) for r in idx["refs"]] == [611, 306, 184]
    assert all(r["meta"] is not None and T.PSEUDO_BIN not in r["bins"] for r in idx["refs"])   # every reference carries the pseudo-bin


def test_reference_index_plans_are_the_pinned_chunks(fixture_index):
    assert query(fixture_index, "1") == ([(0x13e8, 0x5d0a)], (0, b"1", 1, T.UNBOUNDED))
    assert query(fixture_index, "2") == ([(0x5d0a, 0xb387)], (1, b"2", 1, T.UNBOUNDED))
    idx = T.read_index(fixture_index)
    # the pseudo-bin never shows: with its two "chunks" overwritten (they lie behind every real offset then) the plans are the same
    tag = struct.pack("<Ii", T.PSEUDO_BIN, 2)
    garbled = bytearray(fixture_index)
    at = [m.start() for m in re.finditer(re.escape(tag), fixture_index)]
    assert len(at) == 3
    for p in at:
        garbled[p + 8:p + 40] = struct.pack("<QQQQ", 1, 1 << 62, 1 << 61, 1 << 62)
    for name in idx["names"]:
        chunks, _ = query(fixture_index, name)
        assert chunks == T.plan(idx, (name, 1, T.UNBOUNDED)) == query(bytes(garbled), name)[0]
        assert not {c for r in idx["refs"] for c in r["meta"][1:]} & set(chunks)


def test_reference_index_regions_equal_the_python_planner(fixture_index):
    idx = T.read_index(fixture_index)
    rng = random.Random(1)
    for reg in T.random_regions(rng, idx, 200, span=10_100_000):
        chunks, resolved = query(fixture_index, T.region_text(reg))
        assert chunks == T.plan(idx, reg), reg
        assert resolved[1:] == reg


# ---- generated indexes -------------------------------------------------------------------------------------------------------
def boundary_regions(idx, span=1 << 20):
    out = []
    for name in idx["names"]:
        for k in (1, 2, 17, 63):
            for s in (16384 * k, 16384 * k + 1):        # pos = 16384k and 16384k + 1: the last base of a window and the first of the next
                out += [(name, s, s), (name, s, s + 1), (name, s, T.UNBOUNDED), (name, s - 1, s)]
        out += [(name, 1, T.UNBOUNDED), (name, span + 5, span + 9), (name, span * 3, T.UNBOUNDED), (name, T.MAX_POS - 1, T.MAX_POS + 7)]
    return out


def test_generated_indexes_equal_the_python_planner(generated):
    for text, members, idx, raw in generated:
        back = T.read_index(raw)
        assert back["names"] == idx["names"] == [b"1", b"10", b"chrX:1"]
        rng = random.Random(2)
        regions = boundary_regions(idx) + T.random_regions(rng, idx, 150)
        positions = sorted(p for c, p, _, _, _ in T.rows_of(text) if c == b"1")
        gap = max(zip(positions, positions[1:]), key=lambda ab: ab[1] - ab[0])    # an empty stretch
        regions.append((b"1", gap[0] + 1, gap[1] - 1))
        for reg in regions:
            chunks, resolved = query(raw, T.region_text(reg))
            assert chunks == T.plan(back, reg), reg
            assert resolved[1:] == reg


def test_the_python_index_writer_is_conservative(generated):
    """every row a region keeps starts inside a planned chunk: the oracle's index may be trusted as an index"""
    for text, members, idx, raw in generated:
        starts = [(T.fields_of(line), T.voffset_of(members, off)) for off, line in T.data_lines(text)]
        rng = random.Random(3)
        kept = 0
        for reg in T.random_regions(rng, idx, 200) + boundary_regions(idx):
            chunks = T.plan(idx, reg)
            for f, v in starts:
                if T.keeps(*f, *reg):
                    kept += 1
                    assert any(a <= v < b for a, b in chunks), (reg, f[:2])
        assert kept > 2000      # (the regions are not all empty)


def test_a_one_window_region_needs_few_members():
    """the file of the GPU test `the index is used`: at least 64 data members, positions spread over 64 windows — the Python plan of
    a one-window region alone stays below a quarter of the members"""
    text, members, idx, window = T.spread_file()
    assert len(members) >= 64
    offsets = T.member_offsets(T.bgzip(text, T.SPREAD_MEMBER_BYTES)[0])
    ranges = T.member_ranges(T.plan(idx, window), offsets)
    planned = sum(b - a for a, b, _ in ranges) + T.header_members(text, members)
    assert 0 < planned < len(offsets) / 4


# ---- the region grammar ------------------------------------------------------------------------------------------------------
GRAMMAR_INDEX = None


def grammar_index():
    global GRAMMAR_INDEX
    if GRAMMAR_INDEX is None:
        lines = [T.vcf_line(n, 100) for n in (b"1", b"10", b"chr1:5", b"HLA-A*01:01", b"a:b:7-9")]
        text = T.HEADER + b"".join(lines)
        GRAMMAR_INDEX = T.serialize_index(T.build_index(text, T.bgzip(text, 4096)[1]))
    return GRAMMAR_INDEX


@pytest.mark.parametrize("text,want", [
    ("1", (b"1", 1, T.UNBOUNDED)),                       # the whole string is a name
    ("10", (b"10", 1, T.UNBOUNDED)),
    ("1:5", (b"1", 5, T.UNBOUNDED)),                     # name:start runs to the end of the sequence
    ("1:5-9", (b"1", 5, 9)),
    ("1:5-5", (b"1", 5, 5)),
    ("chr1:5", (b"chr1:5", 1, T.UNBOUNDED)),             # a name of the index wins over the split
    ("chr1:5:7", (b"chr1:5", 7, T.UNBOUNDED)),           # the LAST colon
    ("chr1:5:7-8", (b"chr1:5", 7, 8)),
    ("HLA-A*01:01:100-200", (b"HLA-A*01:01", 100, 200)),
    ("a:b:7-9", (b"a:b:7-9", 1, T.UNBOUNDED)),           # a name that itself ends like an interval
    ("a:b:7-9:3", (b"a:b:7-9", 3, T.UNBOUNDED)),
])
def test_region_grammar_accepts(text, want):
    idx = T.read_index(grammar_index())
    assert T.parse_region(idx["names"], text.encode()) == want
    chunks, resolved = query(grammar_index(), text)
    assert resolved[1:] == want and resolved[0] == idx["names"].index(want[0])


@pytest.mark.parametrize("text", ["", "2", "2:5", "1:0", "1:9-5", "1:5-", "1:-5", "1:", "1:1,000", "1:+5", "1:5 ", " 1", "1:1234567890123456789",
                                  ":5", "chr1", "1:5-9-11", "1:5:"])
def test_region_grammar_refuses_and_names_the_region(text):
    from exon_duckdb_amd import abi
    idx = T.read_index(grammar_index())
    with pytest.raises(T.RegionError):
        T.parse_region(idx["names"], text.encode())
    rc, msg = query_rc(grammar_index(), text.encode())
    assert rc == abi.EXG_E_INVALID_ARG and "'%s'" % text in msg, msg


def test_capacity_protocol(fixture_index):
    from exon_duckdb_amd import abi, load_library
    lib = load_library()
    n = C.c_uint64(9)
    assert lib.exg_tabix_query(fixture_index, len(fixture_index), b"1", None, 0, C.byref(n), None) == 0 and n.value == 1   # the counting call
    out = (abi.VirtualChunk * 2)()
    out[1].begin = 77
    assert lib.exg_tabix_query(fixture_index, len(fixture_index), b"1", out, 1, C.byref(n), None) == 0
    assert (out[0].begin, out[0].end, out[1].begin) == (0x13e8, 0x5d0a, 77)
    one = (abi.VirtualChunk * 1)()
    assert lib.exg_tabix_query(fixture_index, len(fixture_index), b"1", one, 0, C.byref(n), None) == abi.EXG_E_CAPACITY and n.value == 1
    assert lib.exg_tabix_query(None, 0, b"1", None, 0, C.byref(n), None) == abi.EXG_E_INVALID_ARG


# ---- bad indexes -------------------------------------------------------------------------------------------------------------
def small_index():
    text = T.HEADER + b"".join(T.vcf_line(c, p) for c in (b"1", b"10") for p in (5, 20000, 40000))
    return T.serialize_index(T.build_index(text, T.bgzip(text, 512)[1]))


def test_truncation_at_every_byte_is_an_error():
    from exon_duckdb_amd import abi
    raw = small_index()
    want = query(raw, "10")
    for n in range(len(raw)):
        rc, msg = query_rc(raw[:n], b"10")
        if n == len(raw) - 8:      # exactly the optional n_no_coor is gone: still an index, the same plan
            assert rc == 0 and query(raw[:n], "10") == want
        else:
            assert rc == abi.EXG_E_PARSE and "tabix index" in msg, (n, rc, msg)


def count_offsets(raw):
    """the byte offsets of every count and length of an index: n_ref, l_nm, per reference n_bin, per bin n_chunk, n_intv"""
    n_ref, l_nm = struct.unpack_from("<i", raw, 4)[0], struct.unpack_from("<i", raw, 32)[0]
    out, p = [4, 32], 36 + l_nm
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", raw, p)
        out.append(p)
        p += 4
        for _ in range(n_bin):
            n_chunk, = struct.unpack_from("<i", raw, p + 4)
            out.append(p + 4)
            p += 8 + 16 * n_chunk
        n_intv, = struct.unpack_from("<i", raw, p)
        out.append(p)
        p += 4 + 8 * n_intv
    assert p + 8 == len(raw)
    return out


def test_every_count_blown_up_is_an_error():
    from exon_duckdb_amd import abi
    raw = small_index()
    offsets = count_offsets(raw)
    assert len(offsets) >= 10
    for at in offsets:
        for value in (0x7FFFFFFF, -1, 1 << 24, 1 << 16):     # (more than the bytes behind it can hold, or negative)
            bad = raw[:at] + struct.pack("<i", value) + raw[at + 4:]
            rc, msg = query_rc(bad, b"10")
            assert rc == abi.EXG_E_PARSE, (at, value, rc, msg)


def test_other_formats_and_magics_are_refused():
    from exon_duckdb_amd import abi
    raw = small_index()
    for fmt in (0, 1, 0x10002):       # generic, SAM, VCF with the zero-based flag
        rc, msg = query_rc(raw[:8] + struct.pack("<i", fmt) + raw[12:], b"10")
        assert rc == abi.EXG_E_PARSE and "format" in msg
    assert query_rc(b"CSI\1" + raw[4:], b"10")[0] == abi.EXG_E_PARSE
    assert query_rc(b"", b"10")[0] == abi.EXG_E_PARSE


# ---- catalog and bind ----------------------------------------------------------------------------------------------------------
def test_catalog_has_vcf_query_and_bind_refuses_without_a_device(tmp_path):
    from exon_duckdb_amd import ExgError
    from exon_duckdb_amd.table_function import connect
    con = connect()
    assert con.has_table_function("vcf_query") and not con.has_table_function("bcf_query") and not con.has_table_function("bam_query")
    plain = os.path.join(ROOT, "tests", "golden", "vcf", "index.vcf.gz")       # BGZF, but no .tbi beside it
    with pytest.raises(ExgError, match=r"needs the tabix index '.*index\.vcf\.gz\.tbi', which does not exist"):
        con.table_function("vcf_query", plain, region="1")
    gz = tmp_path / "plain.vcf.gz"                                             # gzip, not BGZF (and an index beside it)
    gz.write_bytes(gzip.compress(T.HEADER + T.vcf_line(b"1", 5)))
    (tmp_path / "plain.vcf.gz.tbi").write_bytes(open(FIXTURE + ".tbi", "rb").read())
    with pytest.raises(ExgError, match="it is not BGZF-compressed"):
        con.table_function("vcf_query", str(gz), region="1")
    with pytest.raises(ExgError, match="it is not BGZF-compressed"):
        con.table_function("vcf_query", os.path.join(ROOT, "tests", "golden", "vcf", "index.vcf"), region="1")
    # A name the index does not hold: the .tbi is inflated by the DEVICE inflater (no zlib is linked), so the name can be checked
    # only with a device.  Without one this bind fails for that reason (EXG_E_NO_DEVICE) and the unknown name is NOT what is tested
    # here: its message is pinned on the GPU (tests/test_region_gpu.py) and, for the planner alone, by
    # test_region_grammar_refuses_and_names_the_region.  With a device the bind fails by name.
    import torch
    with pytest.raises(ExgError) as e:
        con.table_function("vcf_query", FIXTURE, region="3")
    if torch.cuda.is_available():
        assert "no reference sequence named '3'" in str(e.value)
    else:
        assert "no HIP device" in str(e.value), e.value
    with pytest.raises(ExgError, match="No function matches"):                 # vcf_query takes two arguments, read_vcf one
        con.table_function("vcf_query", FIXTURE)
    with pytest.raises(ExgError, match="No function matches"):
        con.table_function("read_vcf", FIXTURE, region="1")


def test_open_region_refuses_formats_and_shards_before_a_device():
    from exon_duckdb_amd import ExgError, abi
    from exon_duckdb_amd.reader import ShardReader
    for kwargs, code in ((dict(file_format="bcf"), abi.EXG_E_UNSUPPORTED), (dict(file_format="vcf", shard_count=0), abi.EXG_E_UNSUPPORTED),
                         (dict(file_format="vcf", shard_count=2), abi.EXG_E_UNSUPPORTED)):
        with pytest.raises(ExgError) as e:
            ShardReader(FIXTURE, region="1", **kwargs)
        assert e.value.code == code, e.value


# ---- ABI -----------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_header(tmp_path):
    from exon_duckdb_amd import abi
    structs = {"exg_vcf_region_args": abi.VcfRegionArgs, "exg_virtual_chunk": abi.VirtualChunk, "exg_region": abi.Region,
               "exg_reader_stats": abi.ReaderStats}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, "int main(void) {"]
    for cname, cls in structs.items():
        prog.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            prog.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    prog.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)
    assert C.sizeof(abi.ReaderStats) == 14 * 8      # region_members is reserved[0]: the struct did not grow


def test_exported_symbols_and_the_reference_name():
    from exon_duckdb_amd import LIB_PATH, abi, load_library
    lib = load_library()
    assert lib.exg_abi_version() == abi.EXG_ABI_VERSION == 9        # additions only
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    ours = {"exg_tabix_query", "exg_vcf_region_keep", "exg_open_region", "exg_vcf_query_reader"}
    assert ours <= exported and "vcf_query_reader" not in exported
    header = open(HEADER).read()
    for s in ours:
        assert re.search(r"\b" + s + r"\(", header) and s in abi.SIGNATURES, s
    # the reference's own name and signature (rust.hpp:60-63), over the exported entry
    assert re.search(r"VCFReaderResult vcf_query_reader\(struct ArrowArrayStream \*stream_ptr, const char \*uri, const char \*query, uintptr_t batch_size\)", header)


def test_refusals_of_the_predicate_before_any_launch():
    from exon_duckdb_amd import abi, load_library
    lib = load_library()
    a = abi.VcfRegionArgs()
    assert lib.exg_vcf_region_keep(None) == abi.EXG_E_INVALID_ARG
    a.n_rows, a.name_len, a.start, a.end = 0, 1, 1, 1
    assert lib.exg_vcf_region_keep(C.byref(a)) == 0                        # no rows: nothing to do, nothing is touched
    a.n_rows = 5
    assert lib.exg_vcf_region_keep(C.byref(a)) == abi.EXG_E_INVALID_ARG    # null columns
    a.n_rows = 0
    for name_len, start, end in ((0, 1, 1), (1, 0, 5), (1, 6, 5)):
        a.name_len, a.start, a.end = name_len, start, end
        assert lib.exg_vcf_region_keep(C.byref(a)) == abi.EXG_E_INVALID_ARG
    a.name_len, a.start, a.end, a.d_keep = 1, 1, 1, 12                     # unaligned keep words
    assert lib.exg_vcf_region_keep(C.byref(a)) == abi.EXG_E_INVALID_ARG


def test_the_shim_registers_vcf_query_and_still_compiles_against_the_stub():
    shim = open(os.path.join(ROOT, "duckdb_shim", "exon_extension.cpp")).read()
    assert "kRegionRegistrations" in shim and "input.inputs[1].GetValue<string>()" in shim
    tf = open(os.path.join(ROOT, "exon_duckdb_amd", "csrc", "exon_table_function.hpp")).read()
    assert '{"vcf_query", "vcf"}' in tf and "exg_open_region" in tf
    harness = open(os.path.join(ROOT, "exon_duckdb_amd", "csrc", "testing", "exon_tf_harness.cpp")).read()
    assert "kRegionRegistrations" in harness
    stub = os.path.join(ROOT, "tests", "duckdb_stub")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", stub, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "exon_duckdb_amd", "csrc"), os.path.join(ROOT, "duckdb_shim", "exon_extension.cpp")])


def test_host_only_units_include_no_hip():
    for name in ("exg_tabix.hpp", "exg_tabix.cpp", "exg_vcf_region.hpp"):
        src = open(os.path.join(ROOT, "exon_duckdb_amd", "csrc", name)).read()
        assert "hip_runtime" not in src and "exg_common.hpp" not in src, name


# ---- the sanitized driver ------------------------------------------------------------------------------------------------------
def test_host_functions_under_asan_ubsan(tmp_path, fixture_index, generated):
    """tests/region_host_driver.cpp: a stand-alone program over csrc/exg_tabix.cpp and csrc/exg_vcf_region.hpp (exactly-sized heap
    blocks: every truncation and every overwritten word of the reference's index and a generated one, the grammar, the INFO walk
    against a slow restatement on 20 000 texts), built with AddressSanitizer + UBSan; nothing is preloaded.  The plans it prints are
    held against the Python planner."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "region_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "exon_duckdb_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "region_host_driver.cpp")])
    files = {str(tmp_path / "fixture.tbi"): fixture_index, str(tmp_path / "generated.tbi"): generated[0][3]}
    for path, raw in files.items():
        open(path, "wb").write(raw)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)] + list(files), env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "region host functions ok: 2 indexes, 102 plans" in res.stdout and "20000 INFO texts" in res.stdout
    plans = [ln.split(" ") for ln in res.stdout.splitlines() if ln.startswith("plan ")]
    assert len(plans) == 102
    for _, path, region, *chunks in plans:
        idx = T.read_index(files[path])
        want = T.plan(idx, T.parse_region(idx["names"], region.encode()))
        assert [tuple(int(x, 16) for x in c.split("-")) for c in chunks] == want, (path, region)


def test_vectorised_index_builder_equals_the_plain_one():
    """tools/region_bench.py writes its index through build_index_snps (millions of lines): the same index as build_index"""
    import numpy as np
    rng = random.Random(5)
    text = T.HEADER + b"".join(T.vcf_line(b"1", p) for p in sorted(rng.sample(range(1, 300000), 3000)))
    _, members = T.bgzip(text, 1024)
    lines = T.data_lines(text)
    fast = T.build_index_snps(b"1", np.array([T.fields_of(l)[1] for _, l in lines], np.int64), np.array([o for o, _ in lines], np.int64),
                              len(text), members)
    assert fast == T.build_index(text, members)
