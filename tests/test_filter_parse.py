"""The `filters` grammar (exg_filter.hpp) and the row predicate (exg_filter_eval.hpp) on the CPU: tests/filter_parse_driver.cpp
prints the postfix program of each predicate and runs the predicate the device runs on rows given as text; tests/filter_oracle.py
says what DuckDB would answer.  No GPU, no library."""
import os
import random
import subprocess

import pytest

import filter_oracle as fo
from filter_oracle import and_, cmp, isnull, notnull, or_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exon_duckdb_amd", "csrc")

pytestmark = pytest.mark.skipif(not os.path.isdir("/opt/rocm/include"), reason="HIP headers not found")


def build_driver(exe, sanitize=False):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include")]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(cmd + ["-o", str(exe), os.path.join(ROOT, "tests", "filter_parse_driver.cpp")])
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("filter_parse") / "filter_parse_driver")


def run(exe, tmp_path, names, schema, rows, predicates):
    """-> [(program or None, message, kept bits or None)] per predicate"""
    rows_path, pred_path = tmp_path / "rows.txt", tmp_path / "preds.txt"
    with open(rows_path, "w") as f:
        f.write("\t".join(f"{n}:{schema[n]}" for n in names) + "\n")
        for r in rows:
            f.write(fo.encode_row(r, names, schema) + "\n")
    assert not any("\n" in p for p in predicates)
    pred_path.write_bytes("".join(p + "\n" for p in predicates).encode("latin-1"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([exe, str(rows_path), str(pred_path)], capture_output=True, env=env)
    assert res.returncode == 0, (res.returncode, res.stderr.decode("latin-1")[-3000:])   # no exception, no crash
    lines = res.stdout.decode("latin-1").split("\n")
    assert lines[-1] == ""
    lines = lines[:-1]
    per = 2 if rows else 1
    assert len(lines) == per * len(predicates), (len(lines), len(predicates))
    out = []
    for k in range(len(predicates)):
        head = lines[per * k]
        prog = fo.parse_program(head)
        bits = None
        if rows and prog is not None:
            assert lines[per * k + 1].startswith("KEEP ")
            bits = [c == "1" for c in lines[per * k + 1][5:]]
            assert len(bits) == len(rows)
        out.append((prog, head, bits))
    return out


# ---- B1 / B2: the grammar --------------------------------------------------------------------------------------------------
NAMES = ["chrom", "pos", "flag", "qual", "info", "end", "filter", "name"]
SCHEMA = {"chrom": "u", "pos": "l", "flag": "i", "qual": "f", "info": "x", "end": "l", "filter": "u", "name": "u"}
COL = {n: k for k, n in enumerate(NAMES)}


def S(col, op, s):
    return ("CMP", COL[col], op, "S", None, None, s)


def I(col, op, i, f=None):
    return ("CMP", COL[col], op, "I", i, float(i) if f is None else f, None)


def Fl(col, op, f):
    return ("CMP", COL[col], op, "F", None, f, None)


AND, OR = ("AND",), ("OR",)
LONGEST = " AND ".join(f"pos>{k}" for k in range(16))          # 16 leaves + 15 ANDs = 31 ops <= kMaxFilterOps = 32

ACCEPTED = [
    ("pos = 5", [I("pos", "=", 5)]),
    ("pos != 5", [I("pos", "!=", 5)]),
    ("pos <> 5", [I("pos", "!=", 5)]),
    ("pos < 5", [I("pos", "<", 5)]),
    ("pos <= 5", [I("pos", "<=", 5)]),
    ("pos > 5", [I("pos", ">", 5)]),
    ("pos >= 5", [I("pos", ">=", 5)]),
    ("pos<>5", [I("pos", "!=", 5)]),
    ("  pos\t=   5  ", [I("pos", "=", 5)]),
    ("chrom IS NULL", [("NULL", 0)]),
    ("chrom IS NOT NULL", [("NOTNULL", 0)]),
    ("chrom is  not\tnull", [("NOTNULL", 0)]),
    ("qual Is Null", [("NULL", 3)]),
    ('"chrom" = \'a\'', [S("chrom", "=", b"a")]),
    ('"CHROM"=\'a\'', [S("chrom", "=", b"a")]),
    ("Chrom = 'a'", [S("chrom", "=", b"a")]),
    ('"pos">1', [I("pos", ">", 1)]),
    ("pos>1 and flag<2 Or qual>=3", [I("pos", ">", 1), I("flag", "<", 2), AND, Fl("qual", ">=", 3.0), OR]),
    ("pos>1 oR flag<2 AnD qual>=3", [I("pos", ">", 1), I("flag", "<", 2), Fl("qual", ">=", 3.0), AND, OR]),
    ("chrom='it''s'", [S("chrom", "=", b"it's")]),
    ("chrom=''", [S("chrom", "=", b"")]),
    ("chrom=''''", [S("chrom", "=", b"'")]),
    ("chrom>=' a AND b '", [S("chrom", ">=", b" a AND b ")]),
    ("chrom='\xe9\x80'", [S("chrom", "=", b"\xe9\x80")]),
    ("pos=+5", [I("pos", "=", 5)]),
    ("pos=-5", [I("pos", "=", -5)]),
    ("pos= -5", [I("pos", "=", -5)]),
    ("qual=.5", [Fl("qual", "=", 0.5)]),
    ("qual=5.", [Fl("qual", "=", 5.0)]),
    ("qual=1e-3", [Fl("qual", "=", fo.f32(1e-3))]),
    ("qual=1E+3", [Fl("qual", "=", 1000.0)]),
    ("qual=-1.5e1", [Fl("qual", "=", -15.0)]),
    ("pos=1e3", [Fl("pos", "=", 1000.0)]),
    ("pos<5.", [Fl("pos", "<", 5.0)]),
    ("pos<0.1", [Fl("pos", "<", 0.1)]),                        # an integer column compares as float64: the literal stays a double
    ("flag=+.5", [Fl("flag", "=", 0.5)]),
    # a FLOAT column's literal is rounded to float32, whatever its form
    ("qual=5", [Fl("qual", "=", 5.0)]),
    ("qual=0.1", [Fl("qual", "=", fo.f32(0.1))]),
    ("qual>=16777217", [Fl("qual", ">=", 16777216.0)]),
    ("qual<99999999999999999999", [Fl("qual", "<", fo.f32(1e20))]),           # no int64, and a fine float
    ("qual<1e-45", [Fl("qual", "<", fo.f32(1e-45))]),
    ("qual<=3.4028235e38", [Fl("qual", "<=", fo.f32(3.4028235e38))]),
    ("qual=-0", [Fl("qual", "=", -0.0)]),
    ("pos=9223372036854775807", [I("pos", "=", 2 ** 63 - 1)]),
    ("pos=-9223372036854775808", [I("pos", "=", -2 ** 63)]),
    ("pos=007", [I("pos", "=", 7)]),
    # no spaces: a keyword may follow a number directly (pinned: the lexer ends a number at the first byte that cannot continue it)
    ("flag=1AND flag=2", [I("flag", "=", 1), I("flag", "=", 2), AND]),
    ("flag=1OR(flag=2)", [I("flag", "=", 1), I("flag", "=", 2), OR]),
    ("chrom='a'AND pos=1", [S("chrom", "=", b"a"), I("pos", "=", 1), AND]),
    ("((pos=1))", [I("pos", "=", 1)]),
    ("(pos=1 OR (flag=2 AND (qual<3 OR chrom='x')))", [I("pos", "=", 1), I("flag", "=", 2), Fl("qual", "<", 3.0), S("chrom", "=", b"x"), OR, AND, OR]),
    ("(pos=1 OR flag=2) AND qual<3", [I("pos", "=", 1), I("flag", "=", 2), OR, Fl("qual", "<", 3.0), AND]),
    ("( pos = 1 )AND( flag = 2 )", [I("pos", "=", 1), I("flag", "=", 2), AND]),
    ("filter = 'PASS' AND end >= 10", [S("filter", "=", b"PASS"), I("end", ">=", 10), AND]),
    ('"end"<=9 OR "filter" IS NULL', [I("end", "<=", 9), ("NULL", 6), OR]),
    ("END<1 and FILTER<>'q'", [I("end", "<", 1), S("filter", "!=", b"q"), AND]),
    (LONGEST, [x for k in range(16) for x in ([I("pos", ">", k)] + ([AND] if k else []))]),
]

REFUSED = [
    # an unterminated quoted identifier, on a name that is a column and on nothing
    '"pos', '"', '"pos" = 1 AND "flag', '""', '"" = 1',
    # numbers that are not numbers
    "pos = -", "pos=1.2.3", "flag=5e", "qual=-e", "pos=+", "pos=.", "qual=e5", "pos=5e+", "pos=1e", "qual=1..", "qual=--1", "pos=1-2",
    # integers outside int64, floats outside their type
    "pos=99999999999999999999", "pos=9223372036854775808", "pos=-9223372036854775809", "flag=123456789012345678901234567890",
    "pos=1e999", "qual=1e39", "qual=-3.5e38",
    # incomplete or foreign syntax
    '"pos"', "pos", "pos = 5 AND", "pos = 5 OR", "AND pos = 5", "flag ISNULL", "flag IS", "flag IS NOT", "flag IS NOT 5", "flag = 0x10",
    "qual = inf", "qual = nan", "qual = -inf", "qual = NULL", "", " ", "()", "(pos=5", "pos=5)", "pos==5", "pos=<5", "pos=5 flag=2",
    "chrom='abc", "chrom='a''", "pos=5;", "pos=5 -- x", "NOT pos=5", "pos BETWEEN 1 AND 2", "pos IN (1)", "5=pos", "pos=flag",
    # types
    "chrom = 5", "chrom < 1.5", "pos = 'x'", "flag='1'", "qual='x'", "qual > ''",
    # unknown and nested columns
    "nope=1", "nope IS NULL", "info = 'x'", "info IS NULL", "info IS NOT NULL", "pos=1 AND info=1",
    # one op more than kMaxFilterOps holds: 17 leaves + 16 ANDs = 33
    LONGEST + " AND pos>16",
    " OR ".join(f"(flag={k} AND pos<{k})" for k in range(40)),
]


def test_accepted_forms(driver, tmp_path):
    got = run(driver, tmp_path, NAMES, SCHEMA, [], [t for t, _ in ACCEPTED])
    for (text, want), (prog, head, _) in zip(ACCEPTED, got):
        assert prog is not None, (text, head)
        assert len(prog) == len(want), (text, head)
        for g, w in zip(prog, want):
            if w[0] != "CMP":
                assert g == w, (text, head)
                continue
            assert g[:4] == w[:4], (text, head)
            if w[3] == "S":
                assert g[6] == w[6], (text, head)
            if w[3] == "I":
                assert g[4] == w[4], (text, head)
            if w[3] != "S":
                assert g[5] == w[5] and str(g[5]) == str(w[5]), (text, head, g[5], w[5])   # (str: the sign of zero)


def test_refused_forms(driver, tmp_path):
    got = run(driver, tmp_path, NAMES, SCHEMA, [], REFUSED)
    wrong = [(text, head) for text, (prog, head, _) in zip(REFUSED, got) if prog is not None or not head.startswith("ERR ") or len(head) < 6]
    assert not wrong, wrong


# ---- B3 / C: random trees, the parsed program and the real evaluator against keep() ---------------------------------------------
RT_NAMES = ["s", "n", "k", "q", "x"]
RT_SCHEMA = {"s": "u", "n": "l", "k": "i", "q": "f", "x": "x"}       # x: a nested column, never used
STRINGS = [b"", b"a", b"ab", b"abc", b"b", b"B", b"\x80", b"a\xff", b"a\x7f", b"it's", b"0123456789ab", b"0123456789abc", b"0123456789abd",
           b"0123456789abcd", b"0123x56789abc", b" a ", b"(", b"AND"]
BIGINTS = [0, 1, -1, 5, 2 ** 31, -2 ** 31 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 - 1, -2 ** 63, 2 ** 63 - 1, 1000]
INTS = [0, 1, -1, 5, 99, 2 ** 31 - 1, -2 ** 31, 1000]
NAN = float("nan")
FLOATS = [0.0, -0.0, fo.f32(0.1), 0.5, fo.f32(1e-45), fo.f32(3.4028235e38), float("inf"), float("-inf"), NAN, 16777216.0, 50.5, -1.5, fo.f32(0.3),
          fo.f32(-0.1), fo.f32(-1e-45), fo.f32(-3.4028235e38)]
LITERALS = {
    "s": STRINGS,
    "n": [str(v) for v in BIGINTS] + ["0.5", "1e3", "9007199254740992.0", "9007199254740993.0", "5.", "-0.5", "2147483648.5"],
    "k": [str(v) for v in INTS] + ["0.5", "1e3", "98.9", "2147483648", "-2147483649", "5.0"],
    "q": ["0", "-0", "0.0", "0.1", "0.5", "1e-45", "3.4028235e38", "-3.4028235e38", "16777216", "16777217", "50.5", "-1.5", "0.3", "0.30000001", "1e-3", "7e-46"],
}


def leaves(t):
    return sum(leaves(k) for k in t[1]) if t[0] in ("and", "or") else 1


def random_rows(rnd, n):
    return [{"s": rnd.choice(STRINGS + [None] * 3), "n": rnd.choice(BIGINTS + [None] * 2), "k": rnd.choice(INTS + [None] * 2),
             "q": rnd.choice(FLOATS + [None] * 2), "x": None} for _ in range(n)]


def random_trees(rnd, n, depth):
    out = []
    while len(out) < n:
        t = fo.random_tree(rnd, LITERALS, {"s", "n", "k", "q"}, depth)
        if leaves(t) <= 16:                                   # 2 * leaves - 1 ops have to fit kMaxFilterOps = 32
            out.append(t)
    return out


@pytest.mark.parametrize("parens", ["full", "minimal"])
def test_random_trees_round_trip(driver, tmp_path, parens):
    """2000 trees of depth <= 4, as fully parenthesised text and with only the parentheses SQL's precedence needs: the program
    the parser makes of the text (interpreted in Python) and the evaluator the device runs (compiled for the host) both keep
    exactly the rows keep() keeps, on 50 random rows with NULLs."""
    rnd = random.Random(20261018)
    trees = random_trees(rnd, 2000, 4)
    assert max(leaves(t) for t in trees) > 8 and any(t[0] not in ("and", "or") for t in trees)
    rows = random_rows(rnd, 50)
    texts = [fo.render_sql(t, parens) for t in trees]
    if parens == "minimal":
        assert sum("(" in x for x in texts) < sum("(" in fo.render_sql(t, "full") for t in trees)
    got = run(driver, tmp_path, RT_NAMES, RT_SCHEMA, rows, texts)
    bad = []
    for t, text, (prog, head, bits) in zip(trees, texts, got):
        assert prog is not None, (text, head)
        want = [fo.keep(t, r, RT_SCHEMA) for r in rows]
        interp = [fo.run_program(prog, r, RT_NAMES, RT_SCHEMA) for r in rows]
        if interp != want or bits != want:
            bad.append((text, [k for k in range(50) if interp[k] != want[k]], [k for k in range(50) if bits[k] != want[k]]))
    assert not bad, (len(bad), bad[:3])


def test_minimal_renderer_on_the_shapes_that_matter():
    a, b, c = cmp("n", "<", "5"), cmp("n", ">=", "9"), cmp("k", "=", "99")
    assert fo.render_sql(and_(or_(a, b), c), "minimal") == "(n < 5 OR n >= 9) AND k = 99"
    assert fo.render_sql(or_(a, and_(b, c)), "minimal") == "n < 5 OR n >= 9 AND k = 99"
    assert fo.render_sql(and_(or_(a, b), c), "full") == "((n < 5 OR n >= 9) AND k = 99)"
    assert fo.render_sql(or_(or_(a, b), and_(b, and_(a, c))), "minimal") == "n < 5 OR n >= 9 OR n >= 9 AND n < 5 AND k = 99"


def edge_rows():
    rows = [{"s": s, "n": 0, "k": 0, "q": 0.0, "x": None} for s in STRINGS + [b"x" * 300, b"x" * 299 + b"y"]]
    rows += [{"s": b"", "n": 0, "k": 0, "q": q, "x": None} for q in FLOATS + [fo.f32(16777217.0), -fo.f32(1e-45), fo.f32(0.30000001)]]
    rows += [{"s": b"", "n": n, "k": 0, "q": 0.0, "x": None} for n in BIGINTS]
    rows += [{"s": b"", "n": 0, "k": k, "q": 0.0, "x": None} for k in INTS]
    rows += [{"s": None, "n": None, "k": None, "q": None, "x": None}]
    return rows


def test_every_leaf_on_the_edge_rows(driver, tmp_path):
    """the evaluator the device runs, one comparison at a time: each operator against each literal of each column's edge set
    (float32 rounding of the literal, NaN and signed zero, 2^53 + 1 as a double, bytes >= 0x80, strings that differ at byte 5,
    at byte 13, in length only)"""
    rows = edge_rows()
    lits = dict(LITERALS, s=STRINGS + [b"x" * 300, b"x" * 299, b"x" * 301])
    trees = [cmp(c, op, lit) for c in "snkq" for lit in lits[c] for op in fo.OPS] + [f(c) for c in "snkq" for f in (isnull, notnull)]
    got = run(driver, tmp_path, RT_NAMES, RT_SCHEMA, rows, [fo.render_sql(t) for t in trees])
    bad = []
    for t, (prog, head, bits) in zip(trees, got):
        assert prog is not None, (t, head)
        want = [fo.keep(t, r, RT_SCHEMA) for r in rows]
        if bits != want:
            bad.append((t[:3] + (t[3][:20],) if t[0] == "cmp" else t, [(rows[k][t[1]], bits[k], want[k]) for k in range(len(rows)) if bits[k] != want[k]][:4]))
    assert not bad, (len(bad), bad[:6])


def test_float_rows_named(driver, tmp_path):
    """what the widened comparison got wrong: `q = 0.1` on a QUAL of 0.1, NaN above every literal, 16777217 rounding to 16777216"""
    rows = [{"s": b"", "n": 0, "k": 0, "q": q, "x": None} for q in (fo.f32(0.1), NAN, 16777216.0, float("inf"), -0.0, None)]
    cases = [("q = 0.1", [1, 0, 0, 0, 0, 0]), ("q <= 0.1", [1, 0, 0, 0, 1, 0]), ("q > 5", [0, 1, 1, 1, 0, 0]), ("q >= 16777217", [0, 1, 1, 1, 0, 0]),
             ("q = 0", [0, 0, 0, 0, 1, 0]), ("q != 0.1", [0, 1, 1, 1, 1, 0]), ("q < 3.4028235e38", [1, 0, 1, 0, 1, 0]), ("q >= 3.4028235e38", [0, 1, 0, 1, 0, 0])]
    got = run(driver, tmp_path, RT_NAMES, RT_SCHEMA, rows, [t for t, _ in cases])
    for (text, want), (prog, head, bits) in zip(cases, got):
        assert bits == [bool(w) for w in want], (text, bits)


# ---- B4: the same driver under AddressSanitizer + UBSan, as its own program ---------------------------------------------------
def test_driver_under_asan_ubsan(tmp_path):
    exe = build_driver(tmp_path / "filter_parse_asan", sanitize=True)
    rnd = random.Random(7)
    rows = random_rows(rnd, 20) + edge_rows()
    trees = random_trees(rnd, 300, 4)
    texts = [t for t, _ in ACCEPTED if "\xe9" not in t] + REFUSED + [fo.render_sql(t, p) for t in trees for p in ("full", "minimal")]
    # every prefix of a predicate that uses each part of the grammar: the parser meets its input's end everywhere
    whole = '"s" <> \'a\'\'b\' AND (n >= -12 OR q <= 1.5e-3) OR k IS NOT NULL'
    texts += [whole[:k] for k in range(len(whole) + 1)]
    got = run(exe, tmp_path, RT_NAMES + ["chrom", "pos", "flag", "qual", "end"], dict(RT_SCHEMA, chrom="u", pos="l", flag="i", qual="f", end="l"),
              [dict(r, chrom=b"1", pos=1, flag=1, qual=1.0, end=2) for r in rows], texts)
    assert sum(prog is not None for prog, _, _ in got) > 600
    assert sum(prog is None for prog, _, _ in got) > 60


# ---- FilterToString (csrc/exon_table_function.hpp) -> the parser -> the evaluator: the text has to mean the TableFilterSet ----------
TYPE_ID = {"u": 1, "l": 2, "f": 3, "i": 4}                       # EXG_TYPE_VARCHAR / BIGINT / FLOAT / INTEGER
EXPR = {"=": 25, "!=": 26, "<": 27, ">": 28, "<=": 29, ">=": 30}  # duckdb::ExpressionType


def filter_set_line(tree, schema):
    """the TableFilterSet of a tree that fits one, as filter_to_string_driver reads it"""
    def tokens(t):
        if t[0] == "cmp":
            lit = t[3] if isinstance(t[3], bytes) else t[3].encode()
            return ["c%d=%s" % (EXPR[t[2]], lit.hex())]
        if t[0] in ("isnull", "notnull"):
            return ["n" if t[0] == "isnull" else "m"]
        return ["%s%d" % ("A" if t[0] == "and" else "O", len(t[1]))] + [x for k in t[1] for x in tokens(k)]
    cols = fo.columns_of(tree)
    per = {cols[0]: [tree]} if len(cols) == 1 else {}
    if len(cols) > 1:
        for k in tree[1]:
            per.setdefault(fo.columns_of(k)[0], []).append(k)
    return "\t".join("%s:%d:%s" % (c, TYPE_ID[schema[c]], " ".join(tokens(v[0] if len(v) == 1 else and_(*v)))) for c, v in per.items())


def test_filter_to_string_keeps_the_tree(driver, tmp_path):
    """TableFilterSets as DuckDB hands them over (one filter per column, ANDed), rendered by FilterToString, parsed and evaluated:
    the rows kept are keep()'s.  Joined bare, `n<5 OR n>=9` beside `k=99` read as `n<5 OR (n>=9 AND k=99)`."""
    exe = str(tmp_path / "filter_to_string_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "filter_to_string_driver.cpp")])
    rnd = random.Random(5)
    named = [and_(or_(cmp("n", "<", "5"), cmp("n", ">=", "9")), cmp("k", "=", "99")),
             and_(or_(cmp("n", "<", "5"), cmp("n", ">=", "9")), cmp("n", "!=", "1")),
             and_(or_(cmp("s", "=", b"a"), isnull("s")), or_(cmp("q", ">", "0.1"), cmp("q", "<=", "-1.5")), notnull("k"))]
    trees = list(named)
    while len(trees) < 400:
        t = fo.random_tree(rnd, LITERALS, {"s", "n", "k", "q"}, 3) if rnd.random() < 0.5 else \
            and_(*[fo.random_tree(rnd, {c: LITERALS[c]}, {c}, 2) for c in rnd.sample("snkq", rnd.choice((2, 3)))])
        if fo.fits_filter_set(t, RT_SCHEMA) and leaves(t) <= 16:
            trees.append(t)
    assert sum(len(fo.columns_of(t)) > 1 and "or" in fo.render_sql(t).lower() for t in trees) > 100
    sets = tmp_path / "sets.txt"
    sets.write_bytes("".join(filter_set_line(t, RT_SCHEMA) + "\n" for t in trees).encode("latin-1"))
    texts = subprocess.check_output([exe, str(sets)]).decode("latin-1").split("\n")[:-1]
    assert len(texts) == len(trees)
    assert texts[0] == "((n<5 OR n>=9)) AND (k=99)", texts[0]
    rows = random_rows(rnd, 50) + [{"s": b"", "n": n, "k": k, "q": 0.0, "x": None} for n in (1, 5, 9) for k in (99, 5)]
    got = run(driver, tmp_path, RT_NAMES, RT_SCHEMA, rows, texts)
    bad = []
    for t, text, (prog, head, bits) in zip(trees, texts, got):
        assert prog is not None, (text, head)
        if bits != [fo.keep(t, r, RT_SCHEMA) for r in rows]:
            bad.append(text)
    assert not bad, (len(bad), bad[:3])
