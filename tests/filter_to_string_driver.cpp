// filter_to_string_driver.cpp — FilterToString of csrc/exon_table_function.hpp on the host, over the DuckDB API slice of
// csrc/testing/duck_mini.hpp, for tests/test_filter_parse.py: the text it renders of a TableFilterSet goes back through the
// `filters` parser and has to mean the set.  No GPU, no library: only FilterToString is instantiated.
//
//   filter_to_string_driver SETS
//
// SETS: one TableFilterSet per line; entries separated by tabs, each `<column name>:<type id>:<pre-order tokens separated by
// spaces>`, a token being `c<ExpressionType>=<hex constant>` (a comparison), `n` (IS NULL), `m` (IS NOT NULL), `A<k>` / `O<k>`
// (AND / OR of the k nodes that follow).  One line of text per set.
#include <stdio.h>

#include <fstream>
#include <sstream>

#include "testing/duck_mini.hpp"
#include "exon_table_function.hpp"

using namespace exon_amd;

struct HostDuck {
    using idx_t = exon_amd::idx_t;
    using LogicalType = exon_amd::LogicalType;
    using DataChunk = exon_amd::DataChunk;
    using FunctionData = exon_amd::FunctionData;
    using GlobalTableFunctionState = exon_amd::GlobalTableFunctionState;
    using LocalTableFunctionState = exon_amd::LocalTableFunctionState;
    using TableFilter = exon_amd::TableFilter;
    using ConstantFilter = exon_amd::ConstantFilter;
    using ConjunctionFilter = exon_amd::ConjunctionFilter;
    using TableFilterSet = exon_amd::TableFilterSet;
    using TableFilterType = exon_amd::TableFilterType;
    static constexpr idx_t RowId = COLUMN_IDENTIFIER_ROW_ID;
    static constexpr idx_t VectorSize = STANDARD_VECTOR_SIZE;
    static std::string ComparisonOperator(const ConstantFilter &f) {
        switch (f.comparison_type) {
            case ExpressionType::COMPARE_EQUAL: return "=";
            case ExpressionType::COMPARE_NOTEQUAL: return "!=";
            case ExpressionType::COMPARE_LESSTHAN: return "<";
            case ExpressionType::COMPARE_GREATERTHAN: return ">";
            case ExpressionType::COMPARE_LESSTHANOREQUALTO: return "<=";
            default: return ">=";
        }
    }
    static std::string ConstantSQL(const ConstantFilter &f) { return f.constant.ToSQLString(); }
};
using TF = exon_scan::ExonTableFunction<HostDuck>;

static std::unique_ptr<TableFilter> build(std::istringstream &in, int type) {
    std::string tok;
    if (!(in >> tok)) throw std::runtime_error("malformed set");
    if (tok == "n") return std::make_unique<IsNullFilter>();
    if (tok == "m") return std::make_unique<IsNotNullFilter>();
    if (tok[0] == 'c') {
        const size_t eq = tok.find('=');
        Value v;
        v.type = (LogicalTypeId)type;
        for (size_t k = eq + 1; k + 1 < tok.size(); k += 2) v.str.push_back((char)strtoul(tok.substr(k, 2).c_str(), nullptr, 16));
        if (v.type == LogicalTypeId::BIGINT || v.type == LogicalTypeId::INTEGER) v.i = strtoll(v.str.c_str(), nullptr, 10);
        if (v.type == LogicalTypeId::FLOAT) v.f = strtod(v.str.c_str(), nullptr);
        return std::make_unique<ConstantFilter>((ExpressionType)atoi(tok.c_str() + 1), v);
    }
    auto cj = std::make_unique<ConjunctionFilter>(tok[0] == 'A' ? TableFilterType::CONJUNCTION_AND : TableFilterType::CONJUNCTION_OR);
    for (int k = atoi(tok.c_str() + 1); k > 0; k--) cj->child_filters.push_back(build(in, type));
    return cj;
}

int main(int argc, char **argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s SETS\n", argv[0]), 2;
    std::ifstream f(argv[1], std::ios::binary);
    std::string line;
    while (std::getline(f, line)) {
        TableFilterSet set;
        std::vector<HostDuck::idx_t> column_ids;
        std::vector<std::string> names;
        std::istringstream entries(line);
        std::string entry;
        while (std::getline(entries, entry, '\t')) {
            const size_t a = entry.find(':'), b = entry.find(':', a + 1);
            std::istringstream toks(entry.substr(b + 1));
            set.filters[(HostDuck::idx_t)names.size()] = build(toks, atoi(entry.substr(a + 1, b - a - 1).c_str()));
            column_ids.push_back((HostDuck::idx_t)names.size());
            names.push_back(entry.substr(0, a));
        }
        printf("%s\n", TF::FilterToString(set, column_ids, names).c_str());
    }
    return 0;
}
