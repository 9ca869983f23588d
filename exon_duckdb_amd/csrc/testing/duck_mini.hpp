// duck_mini.hpp — the slice of DuckDB v0.8.1's table-function API that the record-scan path
// touches, restated so the host side can be built and tested without DuckDB (its submodule is
// empty in the reference tree and no DuckDB headers exist on the build box).
//
// Layout-bearing types are bit-compatible with DuckDB v0.8.1:
//   string_t            == exg_string_t (16 bytes, duckdb/common/types/string_type.hpp)
//   ValidityMask words  == uint64_t[STANDARD_VECTOR_SIZE / 64], bit set = valid, nullptr = all valid
//   STANDARD_VECTOR_SIZE == 2048
// The classes below keep DuckDB's names and member meaning (duckdb/function/table_function.hpp) so
// that csrc/exon_table_function.hpp — the glue, written once against a traits struct — compiles against
// them exactly as it compiles against DuckDB's own classes in duckdb_shim/exon_extension.cpp.
// TEST SCAFFOLDING: linked into libexon_tf_test.so, never into the product library.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "exon_gpu.h"

namespace exon_amd {

using idx_t = uint64_t;
static constexpr idx_t STANDARD_VECTOR_SIZE = EXG_VECTOR_SIZE;
static constexpr idx_t COLUMN_IDENTIFIER_ROW_ID = (idx_t)-1;

enum class LogicalTypeId {
    VARCHAR = EXG_TYPE_VARCHAR,
    BIGINT = EXG_TYPE_BIGINT,
    FLOAT = EXG_TYPE_FLOAT,
    INTEGER = EXG_TYPE_INTEGER,
    BOOLEAN = EXG_TYPE_BOOLEAN,
    LIST = EXG_TYPE_LIST,
    STRUCT = EXG_TYPE_STRUCT,
    MAP = EXG_TYPE_MAP
};

// duckdb::LogicalType: LIST carries its child type (ListType::GetChildType), STRUCT its named fields
// (StructType::GetChildTypes) — here one vector of (name, type) for both
struct LogicalType {
    LogicalTypeId id = LogicalTypeId::VARCHAR;
    std::vector<std::pair<std::string, LogicalType>> children;
    LogicalType() = default;
    LogicalType(LogicalTypeId i) : id(i) {}
    static LogicalType LIST(LogicalType child) {
        LogicalType t(LogicalTypeId::LIST);
        t.children.emplace_back("", std::move(child));
        return t;
    }
    static LogicalType STRUCT(std::vector<std::pair<std::string, LogicalType>> fields) {
        LogicalType t(LogicalTypeId::STRUCT);
        t.children = std::move(fields);
        return t;
    }
    // duckdb::LogicalType::MAP(key, value): a LIST of STRUCT(key, value) (MapType::KeyType / ValueType)
    static LogicalType MAP(LogicalType key, LogicalType value) {
        LogicalType t(LogicalTypeId::MAP);
        t.children.emplace_back("", STRUCT({{"key", std::move(key)}, {"value", std::move(value)}}));
        return t;
    }
    bool operator==(const LogicalType &o) const { return id == o.id && children == o.children; }
};

using string_t = exg_string_t;

// A flat vector that references memory owned by `buffer` (DuckDB: Vector + VectorBuffer).  LIST and MAP: data = list_entry_t[]
// and children[0] = the child vector (ListVector::GetEntry / SetListSize = its length); STRUCT: children = the entries
// (StructVector::GetEntries).
struct Vector {
    LogicalType type{LogicalTypeId::VARCHAR};
    void *data = nullptr;
    uint64_t *validity = nullptr;  // nullptr = all rows valid
    idx_t length = 0;              // rows (top level) / list size (children)
    std::vector<Vector> children;
    std::shared_ptr<void> buffer;  // keeps data + string payload alive
};

struct DataChunk {
    std::vector<Vector> data;
    idx_t count = 0;
    idx_t size() const { return count; }
    void SetCardinality(idx_t n) { count = n; }
    void Reset() {
        data.clear();
        count = 0;
    }
};

struct TableFunctionInfo {
    virtual ~TableFunctionInfo() = default;
};
struct FunctionData {
    virtual ~FunctionData() = default;
};
struct GlobalTableFunctionState {
    virtual ~GlobalTableFunctionState() = default;
    virtual idx_t MaxThreads() const { return 1; }
};
struct LocalTableFunctionState {
    virtual ~LocalTableFunctionState() = default;
};

struct TableFunctionBindInput {
    std::vector<std::string> inputs;                        // positional VARCHAR arguments
    std::map<std::string, std::string> named_parameters;    // e.g. compression
    const TableFunctionInfo *info = nullptr;
};
// duckdb/planner/table_filter.hpp + filter/{constant,conjunction,null}_filter.hpp, the part FilterToString reads
enum class TableFilterType : uint8_t { CONSTANT_COMPARISON = 0, IS_NULL = 1, IS_NOT_NULL = 2, CONJUNCTION_OR = 3, CONJUNCTION_AND = 4 };
enum class ExpressionType : uint8_t {
    COMPARE_EQUAL = 25,
    COMPARE_NOTEQUAL = 26,
    COMPARE_LESSTHAN = 27,
    COMPARE_GREATERTHAN = 28,
    COMPARE_LESSTHANOREQUALTO = 29,
    COMPARE_GREATERTHANOREQUALTO = 30
};
// duckdb::Value, reduced to what a pushed-down constant of these columns can be
struct Value {
    LogicalTypeId type = LogicalTypeId::VARCHAR;
    std::string str;
    int64_t i = 0;
    double f = 0;
    // Value::ToSQLString: strings quoted with '' escaping, numbers bare
    std::string ToSQLString() const {
        if (type == LogicalTypeId::VARCHAR) {
            std::string out = "'";
            for (char c : str) {
                if (c == '\'') out += "'";
                out += c;
            }
            return out + "'";
        }
        if (type == LogicalTypeId::BIGINT || type == LogicalTypeId::INTEGER) return std::to_string(i);
        char buf[64];
        snprintf(buf, sizeof buf, "%.9g", f);
        std::string t = buf;
        if (t.find_first_of(".eEn") == std::string::npos) t += ".0";
        return t;
    }
};
struct TableFilter {
    TableFilterType filter_type;
    explicit TableFilter(TableFilterType t) : filter_type(t) {}
    virtual ~TableFilter() = default;
};
struct ConstantFilter : TableFilter {
    ExpressionType comparison_type;
    Value constant;
    ConstantFilter(ExpressionType c, Value v) : TableFilter(TableFilterType::CONSTANT_COMPARISON), comparison_type(c), constant(std::move(v)) {}
};
struct IsNullFilter : TableFilter {
    IsNullFilter() : TableFilter(TableFilterType::IS_NULL) {}
};
struct IsNotNullFilter : TableFilter {
    IsNotNullFilter() : TableFilter(TableFilterType::IS_NOT_NULL) {}
};
struct ConjunctionFilter : TableFilter {
    std::vector<std::unique_ptr<TableFilter>> child_filters;
    explicit ConjunctionFilter(TableFilterType t) : TableFilter(t) {}
};
struct TableFilterSet {
    std::map<idx_t, std::unique_ptr<TableFilter>> filters;  // key: index into column_ids
};

struct TableFunctionInitInput {
    const FunctionData *bind_data = nullptr;
    std::vector<idx_t> column_ids;  // projection pushdown
    const TableFilterSet *filters = nullptr;  // filter pushdown
};
struct TableFunctionInput {
    const FunctionData *bind_data = nullptr;
    LocalTableFunctionState *local_state = nullptr;
    GlobalTableFunctionState *global_state = nullptr;
};

struct TableFunction {
    using bind_t = std::function<std::unique_ptr<FunctionData>(TableFunctionBindInput &, std::vector<LogicalType> &,
                                                               std::vector<std::string> &)>;
    using init_global_t = std::function<std::unique_ptr<GlobalTableFunctionState>(TableFunctionInitInput &)>;
    using init_local_t =
        std::function<std::unique_ptr<LocalTableFunctionState>(TableFunctionInitInput &, GlobalTableFunctionState *)>;
    using function_t = std::function<void(TableFunctionInput &, DataChunk &)>;
    using batch_index_t = std::function<idx_t(const FunctionData *, LocalTableFunctionState *, GlobalTableFunctionState *)>;

    std::string name;
    std::vector<LogicalType> arguments;
    function_t function;
    bind_t bind;
    init_global_t init_global;
    init_local_t init_local;
    batch_index_t get_batch_index;
    std::map<std::string, LogicalType> named_parameters;
    std::shared_ptr<TableFunctionInfo> function_info;
    bool projection_pushdown = false;
    bool filter_pushdown = false;
};

class Catalog {
public:
    void CreateTableFunction(const TableFunction &f) { functions_[f.name] = f; }
    const TableFunction *GetTableFunction(const std::string &name) const {
        auto it = functions_.find(name);
        return it == functions_.end() ? nullptr : &it->second;
    }
    std::vector<std::string> Names() const {
        std::vector<std::string> n;
        for (auto &kv : functions_) n.push_back(kv.first);
        return n;
    }

private:
    std::map<std::string, TableFunction> functions_;
};

}  // namespace exon_amd
