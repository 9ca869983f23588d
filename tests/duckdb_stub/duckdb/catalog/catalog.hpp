// test infrastructure: see tests/duckdb_stub/duckdb.hpp.  The part of DuckDB v0.8.1's duckdb/catalog/catalog.hpp,
// catalog_transaction.hpp and parser/parsed_data/create_scalar_function_info.hpp that registering a ScalarFunctionSet takes
// (what ExtensionUtil::RegisterFunction does for a single function).
#pragma once
#include "duckdb.hpp"
#include "duckdb/function/function_set.hpp"

namespace duckdb {
struct CreateFunctionInfo {
	virtual ~CreateFunctionInfo();
};
struct CreateScalarFunctionInfo : public CreateFunctionInfo {
	explicit CreateScalarFunctionInfo(ScalarFunctionSet set);
};
struct CatalogTransaction {
	static CatalogTransaction GetSystemTransaction(DatabaseInstance &db);
};
class CatalogEntry;
class Catalog {
public:
	static Catalog &GetSystemCatalog(DatabaseInstance &db);
	optional_ptr<CatalogEntry> CreateFunction(CatalogTransaction transaction, CreateFunctionInfo &info);
};
} // namespace duckdb
