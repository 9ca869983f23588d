// filter_parse_driver.cpp — the `filters` grammar (exg_filter.hpp) and the row predicate (exg_filter_eval.hpp) on the host,
// for tests/test_filter_parse.py.  No GPU, no library: the two headers are all it links.
//
//   filter_parse_driver ROWS PREDICATES
//
// ROWS: first line the schema, `name:kind` separated by tabs (kind u / l / i / f as FilterColumn has them, anything else a
// nested column); then one row per line, one field per column separated by tabs: `N` NULL, `S<hex bytes>`, `I<decimal>`,
// `F<8 hex digits: the float's bits>`.  PREDICATES: one per line (bytes as they are).
//
// Per predicate one line, `ERR <message>` or `OK <op>;<op>;...` with the postfix program:
//   AND | OR | NULL <col> | NOTNULL <col> | CMP <col> <cmp 0..5> <S|I|F> <int64> <double as %a> <string as hex>
// and, when ROWS has rows, a second line `KEEP <one 0/1 per row>` from filter_eval_row.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <string>
#include <vector>

#include "exg_filter.hpp"
#include "exg_filter_eval.hpp"

namespace ea = exg::arrow;

struct Field {
    bool null = true;
    std::string s;
    int64_t i = 0;
    float f = 0;
};
struct HostRow {
    const std::vector<exg_rd::FilterColumn> &cols;
    const std::vector<Field> &v;
    uint32_t kind(uint32_t c) const {
        return cols[c].kind == 'u' ? ea::kColStr : cols[c].kind == 'l' ? ea::kColI64 : cols[c].kind == 'i' ? ea::kColI32 : ea::kColF32;
    }
    bool is_null(uint32_t c) const { return v[c].null; }
    const uint8_t *str(uint32_t c, uint32_t *len) const {
        *len = (uint32_t)v[c].s.size();
        return (const uint8_t *)v[c].s.data();
    }
    int64_t i64(uint32_t c) const { return v[c].i; }
    float f32(uint32_t c) const { return v[c].f; }
};

static std::vector<std::string> split(const std::string &line, char sep) {
    std::vector<std::string> out(1);
    for (char ch : line) {
        if (ch == sep) out.emplace_back();
        else out.back().push_back(ch);
    }
    return out;
}
static std::string unhex(const std::string &h) {
    std::string out;
    for (size_t k = 0; k + 1 < h.size(); k += 2) out.push_back((char)strtoul(h.substr(k, 2).c_str(), nullptr, 16));
    return out;
}

int main(int argc, char **argv) {
    if (argc != 3) return fprintf(stderr, "usage: %s ROWS PREDICATES\n", argv[0]), 2;
    std::ifstream rf(argv[1], std::ios::binary), pf(argv[2], std::ios::binary);
    if (!rf || !pf) return fprintf(stderr, "cannot open the inputs\n"), 2;
    std::string line;
    if (!std::getline(rf, line)) return fprintf(stderr, "no schema line\n"), 2;
    std::vector<exg_rd::FilterColumn> cols;
    for (auto &f : split(line, '\t')) {
        const size_t colon = f.rfind(':');
        if (colon == std::string::npos || colon + 2 != f.size()) return fprintf(stderr, "bad schema field %s\n", f.c_str()), 2;
        cols.push_back({f.substr(0, colon), f[colon + 1]});
    }
    if (cols.size() > (size_t)ea::kMaxFilterCols) return fprintf(stderr, "too many columns\n"), 2;
    std::vector<std::vector<Field>> rows;
    while (std::getline(rf, line)) {
        auto fs = split(line, '\t');
        if (fs.size() != cols.size()) return fprintf(stderr, "row %zu has %zu fields\n", rows.size(), fs.size()), 2;
        std::vector<Field> row(cols.size());
        for (size_t c = 0; c < cols.size(); c++) {
            const std::string &t = fs[c];
            if (t.empty()) return fprintf(stderr, "empty field\n"), 2;
            Field &fd = row[c];
            fd.null = t[0] == 'N';
            if (t[0] == 'S') fd.s = unhex(t.substr(1));
            else if (t[0] == 'I') fd.i = strtoll(t.c_str() + 1, nullptr, 10);
            else if (t[0] == 'F') {
                const uint32_t bits = (uint32_t)strtoul(t.c_str() + 1, nullptr, 16);
                memcpy(&fd.f, &bits, 4);
            } else if (t[0] != 'N') return fprintf(stderr, "bad field %s\n", t.c_str()), 2;
        }
        rows.push_back(std::move(row));
    }
    while (std::getline(pf, line)) {
        exg_rd::FilterParser fp(line, cols);
        if (!fp.parse()) {
            printf("ERR %s\n", fp.err.c_str());
            if (!rows.empty()) printf("KEEP\n");
            continue;
        }
        printf("OK ");
        for (uint32_t k = 0; k < fp.prog.n_ops; k++) {
            const ea::FilterOp &op = fp.prog.ops[k];
            if (k) printf(";");
            if (op.op == ea::kOpAnd) printf("AND");
            else if (op.op == ea::kOpOr) printf("OR");
            else if (op.op == ea::kOpIsNull) printf("NULL %u", op.col);
            else if (op.op == ea::kOpIsNotNull) printf("NOTNULL %u", op.col);
            else {
                printf("CMP %u %u %c %lld %a ", op.col, op.cmp, op.lit == ea::kLitStr ? 'S' : op.lit == ea::kLitInt ? 'I' : 'F', (long long)op.i, op.f);
                if (op.lit == ea::kLitStr)
                    for (uint32_t b = 0; b < op.str_len; b++) printf("%02x", (unsigned char)fp.consts[op.str_off + b]);
            }
        }
        printf("\n");
        if (!rows.empty()) {
            std::string bits;
            for (auto &row : rows)
                bits.push_back(ea::filter_eval_row(fp.prog, (const uint8_t *)fp.consts.data(), HostRow{cols, row}) ? '1' : '0');
            printf("KEEP %s\n", bits.c_str());
        }
    }
    return 0;
}
