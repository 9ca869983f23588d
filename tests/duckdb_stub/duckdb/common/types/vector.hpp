// test infrastructure: see tests/duckdb_stub/duckdb.hpp.  The part of DuckDB v0.8.1's duckdb/common/types/vector.hpp that the
// VARCHAR-producing scalars of the shim touch, beside what duckdb.hpp already declares of that header.
#pragma once
#include "duckdb.hpp"

namespace duckdb {
struct StringVector {
	//! Add a string to the string heap of the vector (auxiliary data)
	static string_t AddString(Vector &vector, const char *data, idx_t len);
	static string_t AddString(Vector &vector, const string &data);
};
} // namespace duckdb
