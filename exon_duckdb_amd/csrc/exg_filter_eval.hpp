// exg_filter_eval.hpp — the row predicate of `filters`, without the fetching: the comparison by column kind given a fetched
// operand, the six-way decision, and SQL's three-valued AND / OR over the postfix program of exg_filter.hpp.  Compiles for
// the device (exg_arrow.hip binds it to the columns in HBM) and for the host (tests/filter_parse_driver.cpp runs it on rows
// given as text, against an independent evaluator).
//
// The order is DuckDB's, because DuckDB does not evaluate a pushed filter again: VARCHAR by unsigned bytes, then length;
// FLOAT in float32 against the literal rounded to float32 (FilterParser stores that float in FilterOp::f), -0 = +0,
// NaN = NaN and NaN above every other value, +inf included.  An integer column against a literal with a fraction or an
// exponent compares as two doubles (DuckDB never pushes such a filter; DataFusion coerces this way).
#pragma once
#include <stdint.h>

#include "exg_arrow.hpp"

#ifndef EXG_HD
#if defined(__HIPCC__)
#define EXG_HD __host__ __device__
#else
#define EXG_HD
#endif
#endif

namespace exg {
namespace arrow {

// sign of a - b
EXG_HD inline int filter_cmp_bytes(const uint8_t *p, uint32_t len, const uint8_t *q, uint32_t qlen) {
    const uint32_t m = len < qlen ? len : qlen;
    for (uint32_t i = 0; i < m; i++) {
        int d = (int)p[i] - (int)q[i];
        if (d) return d < 0 ? -1 : 1;
    }
    return len < qlen ? -1 : len > qlen ? 1 : 0;
}
// sign of x - y where NaN = NaN and NaN is the largest value
template <class T>
EXG_HD inline int filter_cmp_float(T x, T y) {
    if (x < y) return -1;
    if (x > y) return 1;
    if (x == y) return 0;
    const bool xn = x != x, yn = y != y;  // unordered: at least one is NaN
    return xn ? (yn ? 0 : 1) : -1;
}
EXG_HD inline int filter_cmp_int(int64_t x, const FilterOp &op) {
    if (op.lit == kLitInt) return x < op.i ? -1 : x > op.i ? 1 : 0;
    return filter_cmp_float<double>((double)x, op.f);
}
EXG_HD inline int filter_cmp_f32(float x, const FilterOp &op) { return filter_cmp_float<float>(x, (float)op.f); }

EXG_HD inline bool filter_decide(uint8_t cmp, int d) {
    switch (cmp) {
        case kEq: return d == 0;
        case kNe: return d != 0;
        case kLt: return d < 0;
        case kLe: return d <= 0;
        case kGt: return d > 0;
        default: return d >= 0;
    }
}

// the operand stack: two bit fields (value, is-null), at most kMaxFilterOps deep
struct FilterStack {
    uint32_t vals = 0, nulls = 0;
    int sp = 0;
    EXG_HD void push(bool v, bool nul) {
        vals = (vals & ~(1u << sp)) | ((uint32_t)v << sp);
        nulls = (nulls & ~(1u << sp)) | ((uint32_t)nul << sp);
        sp++;
    }
    EXG_HD void combine(bool is_and) {  // Kleene AND / OR of the two on top
        sp -= 2;
        const bool av = (vals >> sp) & 1, an = (nulls >> sp) & 1;
        const bool bv = (vals >> (sp + 1)) & 1, bn = (nulls >> (sp + 1)) & 1;
        bool rv, rn;
        if (is_and) {
            const bool any_false = (!an && !av) || (!bn && !bv);
            rn = !any_false && (an || bn);
            rv = !any_false && !rn;
        } else {
            const bool any_true = (!an && av) || (!bn && bv);
            rn = !any_true && (an || bn);
            rv = any_true;
        }
        vals = (vals & ~(3u << sp)) | ((uint32_t)rv << sp);
        nulls = (nulls & ~(3u << sp)) | ((uint32_t)rn << sp);
        sp++;
    }
    EXG_HD bool kept() const { return sp == 1 && (vals & 1) && !(nulls & 1); }  // a row is kept only on TRUE
};

// One row.  `row` fetches: kind(c), is_null(c), str(c, &len), i64(c) (an Int32 column widened), f32(c).
template <class Row>
EXG_HD inline bool filter_eval_row(const FilterProgram &prog, const uint8_t *consts, const Row &row) {
    FilterStack st;
    for (uint32_t k = 0; k < prog.n_ops; k++) {
        const FilterOp &op = prog.ops[k];
        if (op.op == kOpAnd || op.op == kOpOr) {
            st.combine(op.op == kOpAnd);
            continue;
        }
        const uint32_t c = op.col;
        bool v = false, nul = false;
        if (op.op == kOpIsNull)
            v = row.is_null(c);
        else if (op.op == kOpIsNotNull)
            v = !row.is_null(c);
        else if (row.is_null(c))
            nul = true;
        else {
            int d;  // sign of column - literal
            const uint32_t kind = row.kind(c);
            if (kind == kColStr) {
                uint32_t len;
                const uint8_t *p = row.str(c, &len);
                d = filter_cmp_bytes(p, len, consts + op.str_off, op.str_len);
            } else if (kind == kColF32) {
                d = filter_cmp_f32(row.f32(c), op);
            } else {
                d = filter_cmp_int(row.i64(c), op);
            }
            v = filter_decide(op.cmp, d);
        }
        st.push(v, nul);
    }
    return st.kept();
}

}  // namespace arrow
}  // namespace exg
