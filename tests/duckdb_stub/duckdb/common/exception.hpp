// test infrastructure: see tests/duckdb_stub/duckdb.hpp.  The exceptions of DuckDB v0.8.1's duckdb/common/exception.hpp that
// the shim's scalars throw.
#pragma once
#include <stdexcept>

#include "duckdb.hpp"

namespace duckdb {
class Exception : public std::exception {
public:
	explicit Exception(const string &msg);
	const char *what() const noexcept override;
};
class InvalidInputException : public Exception {
public:
	explicit InvalidInputException(const string &msg);
};
} // namespace duckdb
