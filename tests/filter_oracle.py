"""An evaluator of `filters` predicates that shares no code with the library: what DuckDB would answer for the filter it
pushed down (DuckDB does not evaluate a pushed filter again, so the scan's answer is the query's).  A helper of
test_filter_parse.py and test_filters_gpu.py, not a test module.

A predicate is a tree of tuples:

    cmp(col, op, literal)    op in = != < <= > >=; literal: bytes for a VARCHAR column, the literal's TEXT (str) for a number
    isnull(col) / notnull(col)
    and_(a, b, ...) / or_(a, b, ...)

`schema` maps a column name to its kind: 'u' VARCHAR, 'l' BIGINT, 'i' INTEGER, 'f' FLOAT (anything else: nested, not
filterable).  A row is a dict name -> bytes / int / float / None (None = NULL; a FLOAT value is a Python float that holds
a float32).

keep(tree, row, schema) is SQL's three-valued logic: NULL propagates through comparisons, AND / OR are Kleene's, a row is
kept only on TRUE.  The leaves:
  * VARCHAR: unsigned bytewise order, then length — Python's bytes comparison;
  * INTEGER / BIGINT against an integer literal: exact;
  * INTEGER / BIGINT against a literal with '.' or an exponent: both sides as float64 (float(x): Python's own int < float
    is exact and would disagree at 2^53 + 1);
  * FLOAT: the literal rounded to float32, then DuckDB's order: -0 = +0, NaN = NaN, NaN above everything, +inf included.
"""
import math
import re
import struct

OPS = ("=", "!=", "<", "<=", ">", ">=")
_INT = re.compile(r"^[+-]?\d+$")


def cmp(col, op, literal):
    assert op in OPS
    return ("cmp", col, op, literal)


def isnull(col):
    return ("isnull", col)


def notnull(col):
    return ("notnull", col)


def and_(*kids):
    assert len(kids) >= 2
    return ("and", tuple(kids))


def or_(*kids):
    assert len(kids) >= 2
    return ("or", tuple(kids))


def f32(x):
    """x rounded to float32, as a Python float"""
    return struct.unpack("<f", struct.pack("<f", x))[0]


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def columns_of(tree):
    if tree[0] in ("and", "or"):
        out = []
        for k in tree[1]:
            for c in columns_of(k):
                if c not in out:
                    out.append(c)
        return out
    return [tree[1]]


# ---- the two renderers -------------------------------------------------------------------------------------------------
def _literal_sql(lit):
    if isinstance(lit, bytes):
        return "'" + lit.decode("latin-1").replace("'", "''") + "'"
    return lit


def _leaf_sql(t):
    if t[0] == "cmp":
        return f"{t[1]} {t[2]} {_literal_sql(t[3])}"
    return f"{t[1]} IS NULL" if t[0] == "isnull" else f"{t[1]} IS NOT NULL"


def render_sql(tree, parens="full"):
    """SQL text for `filters=` (a str whose code points are the bytes: encode it with latin-1).  parens="full": every inner
    node in parentheses.  parens="minimal": only where SQL's precedence needs them — AND binds tighter than OR, so an OR
    under an AND keeps its parentheses and nothing else does."""
    if tree[0] not in ("and", "or"):
        return _leaf_sql(tree)
    word = " AND " if tree[0] == "and" else " OR "
    if parens == "full":
        return "(" + word.join(render_sql(k, parens) for k in tree[1]) + ")"
    parts = []
    for k in tree[1]:
        s = render_sql(k, parens)
        parts.append("(" + s + ")" if tree[0] == "and" and k[0] == "or" else s)
    return word.join(parts)


def fits_filter_set(tree, schema):
    """A TableFilterSet holds one filter per column, ANDed: the tree must be single-column, or an AND of single-column
    subtrees.  An integer column's literals must be integers (DuckDB never pushes a filter with another constant type)."""
    def literals_ok(t):
        if t[0] in ("and", "or"):
            return all(literals_ok(k) for k in t[1])
        return t[0] != "cmp" or schema[t[1]] not in "li" or bool(_INT.match(t[3]))
    if not literals_ok(tree):
        return False
    if len(columns_of(tree)) == 1:
        return True
    return tree[0] == "and" and all(len(columns_of(k)) == 1 for k in tree[1])


def render_filter_set(tree, schema, F):
    """{column: F...} for table_function.Relation (F = exon_duckdb_amd.table_function.F), or None when the tree does not fit"""
    if not fits_filter_set(tree, schema):
        return None

    def node(t):
        if t[0] == "cmp":
            lit = t[3]
            return F.cmp(t[2], lit if isinstance(lit, bytes) else int(lit) if schema[t[1]] in "li" else lit)
        if t[0] == "isnull":
            return F.isnull()
        if t[0] == "notnull":
            return F.notnull()
        return (F.and_ if t[0] == "and" else F.or_)(*[node(k) for k in t[1]])
    if len(columns_of(tree)) == 1:
        return {columns_of(tree)[0]: node(tree)}
    per = {}
    for k in tree[1]:
        per.setdefault(columns_of(k)[0], []).append(node(k))
    return {c: v[0] if len(v) == 1 else F.and_(*v) for c, v in per.items()}


# ---- keep() --------------------------------------------------------------------------------------------------------------
def _decide(op, d):
    return {"=": d == 0, "!=": d != 0, "<": d < 0, "<=": d <= 0, ">": d > 0, ">=": d >= 0}[op]


def _sign(a, b):
    return -1 if a < b else 1 if a > b else 0


def _float_key(x):
    return (1, 0.0) if math.isnan(x) else (0, x)          # NaN = NaN, above everything; -0.0 == 0.0 in Python too


def compare(kind, x, lit):
    """sign of column value x against the literal, by the column's kind"""
    if kind == "u":
        assert isinstance(lit, bytes) and isinstance(x, bytes)
        return _sign(x, lit)
    assert isinstance(lit, str)
    if kind in "li":
        if _INT.match(lit):
            return _sign(x, int(lit))
        return _sign(_float_key(float(x)), _float_key(float(lit)))
    assert kind == "f"
    return _sign(_float_key(x), _float_key(f32(float(lit))))


def value(tree, row, schema):
    """True / False / None (NULL)"""
    t = tree[0]
    if t == "isnull":
        return row[tree[1]] is None
    if t == "notnull":
        return row[tree[1]] is not None
    if t == "cmp":
        x = row[tree[1]]
        return None if x is None else _decide(tree[2], compare(schema[tree[1]], x, tree[3]))
    vals = [value(k, row, schema) for k in tree[1]]
    if t == "and":
        return False if any(v is False for v in vals) else None if any(v is None for v in vals) else True
    return True if any(v is True for v in vals) else None if any(v is None for v in vals) else False


def keep(tree, row, schema):
    return value(tree, row, schema) is True


# ---- the postfix program the host driver prints (tests/filter_parse_driver.cpp), interpreted here ---------------------------
CMPS = ("=", "!=", "<", "<=", ">", ">=")   # exg::arrow::kEq .. kGe


def parse_program(line):
    """`OK op;op;...` -> list of ops, or None for `ERR ...`"""
    if not line.startswith("OK "):
        assert line.startswith("ERR"), line
        return None
    ops = []
    for tok in line[3:].split(";"):
        f = tok.split(" ")
        if f[0] in ("AND", "OR"):
            ops.append((f[0],))
        elif f[0] in ("NULL", "NOTNULL"):
            ops.append((f[0], int(f[1])))
        else:
            assert f[0] == "CMP", tok
            ops.append(("CMP", int(f[1]), CMPS[int(f[2])], f[3], int(f[4]), float.fromhex(f[5]), bytes.fromhex(f[6]) if len(f) > 6 else b""))
    return ops


def run_program(ops, row, names, schema):
    """the postfix program on one row, three-valued; True when the row is kept"""
    st = []
    for op in ops:
        if op[0] in ("AND", "OR"):
            b, a = st.pop(), st.pop()
            if op[0] == "AND":
                st.append(False if (a is False or b is False) else None if (a is None or b is None) else True)
            else:
                st.append(True if (a is True or b is True) else None if (a is None or b is None) else False)
            continue
        x = row[names[op[1]]]
        if op[0] == "NULL":
            st.append(x is None)
        elif op[0] == "NOTNULL":
            st.append(x is not None)
        elif x is None:
            st.append(None)
        else:
            _, _, c, lit, i, f, s = op
            kind = schema[names[op[1]]]
            if kind == "u":
                assert lit == "S"
                d = _sign(x, s)
            elif kind in "li" and lit == "I":
                d = _sign(x, i)
            elif kind in "li":
                d = _sign(_float_key(float(x)), _float_key(f))
            else:
                d = _sign(_float_key(x), _float_key(f))      # f is what the program compares with, as it stands
            st.append(_decide(c, d))
    assert len(st) == 1
    return st[0] is True


# ---- random trees ----------------------------------------------------------------------------------------------------------
def random_tree(rnd, literals, nullable, depth, p_leaf=0.3):
    """literals: {column: [literal, ...]}; nullable: the columns IS [NOT] NULL is worth asking of"""
    if depth == 0 or rnd.random() < p_leaf:
        col = rnd.choice(sorted(literals))
        if col in nullable and rnd.random() < 0.12:
            return (isnull if rnd.random() < 0.5 else notnull)(col)
        return cmp(col, rnd.choice(OPS), rnd.choice(literals[col]))
    kids = [random_tree(rnd, literals, nullable, depth - 1, p_leaf) for _ in range(rnd.choice((2, 2, 3)))]
    return (and_ if rnd.random() < 0.5 else or_)(*kids)


def encode_row(row, names, schema):
    """a row as filter_parse_driver reads it"""
    out = []
    for n in names:
        x = row[n]
        if x is None:
            out.append("N")
        elif schema[n] == "u":
            out.append("S" + x.hex())
        elif schema[n] in "li":
            out.append("I%d" % x)
        elif schema[n] == "f":
            out.append("F%08x" % f32_bits(x))
        else:
            out.append("N")
    return "\t".join(out)
