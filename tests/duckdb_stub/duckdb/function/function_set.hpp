// test infrastructure: see tests/duckdb_stub/duckdb.hpp.  The part of DuckDB v0.8.1's duckdb/function/function_set.hpp that the
// shim's overloaded scalars (alignment_score in its two-, six- and seven-argument forms) touch.
#pragma once
#include "duckdb.hpp"

namespace duckdb {
class ScalarFunctionSet {
public:
	explicit ScalarFunctionSet(string name);
	void AddFunction(ScalarFunction function);
};
} // namespace duckdb
