// duckdb_shim/exon_extension.cpp — the REAL DuckDB v0.8.1 binding of libexon_gpu.so: `LOAD exon`.
//
// All of the glue's logic — bind / init_global (shard plan, FilterToString) / init_local (one reader per shard and device) /
// scan / batch index / replacement scan — is exon_duckdb_amd/csrc/exon_table_function.hpp, written once against a traits
// struct.  This file is that header instantiated over DuckDB's own classes: the traits (how a LogicalType and a Vector are
// made in DuckDB), thin wrappers with DuckDB's callback signatures, and the registrations.  The same header instantiated
// over csrc/testing/duck_mini.hpp is what the GPU test-suite drives (csrc/testing/exon_tf_harness.cpp), so the logic is
// compiled and tested on the build box; THIS file needs DuckDB's headers, which do not exist there (the reference's
// `duckdb/` submodule is empty), and is therefore not part of build().  It replaces, in the reference tree,
//   exon/src/exon/arrow_table_function/module.cpp   (Register / FileTypeBind / InitGlobal / Scan / ReplacementScan)
//   exon/src/exon_extension.cpp:47-58,79            (registrations of the three formats + replacement scan)
// Build (out-of-tree extension, like the reference's CMakeLists.txt:131-146, minus Rust/Corrosion):
//   c++ -std=c++17 -fPIC -shared -DDUCKDB_BUILD_LOADABLE_EXTENSION -I<duckdb>/src/include -I../include
//       -I../exon_duckdb_amd/csrc exon_extension.cpp -L../exon_duckdb_amd/lib -lexon_gpu -o exon.duckdb_extension
// tests/test_host_logic.py puts this file through `c++ -fsyntax-only` against declaration-only stand-ins of the DuckDB
// headers it includes (tests/duckdb_stub/: signatures as in v0.8.1): every template instantiation of the glue over DuckDB's
// types is compiled on the build box.
#define DUCKDB_EXTENSION_MAIN
#include "duckdb.hpp"
#include "duckdb/catalog/catalog.hpp"
#include "duckdb/common/exception.hpp"
#include "duckdb/common/types/vector.hpp"
#include "duckdb/common/types/vector_buffer.hpp"
#include "duckdb/function/function_set.hpp"
#include "duckdb/function/scalar_function.hpp"
#include "duckdb/function/table_function.hpp"
#include "duckdb/main/extension_util.hpp"
#include "duckdb/parser/expression/constant_expression.hpp"
#include "duckdb/parser/expression/function_expression.hpp"
#include "duckdb/parser/tableref/table_function_ref.hpp"
#include "duckdb/planner/filter/conjunction_filter.hpp"
#include "duckdb/planner/filter/constant_filter.hpp"
#include "duckdb/planner/table_filter.hpp"
#include "duckdb/storage/statistics/node_statistics.hpp"

#include "exon_table_function.hpp"

namespace exon {
using namespace duckdb;

static_assert(sizeof(string_t) == sizeof(exg_string_t), "exg_string_t must be duckdb::string_t");
static_assert(sizeof(list_entry_t) == sizeof(exg_list_entry_t), "exg_list_entry_t must be duckdb::list_entry_t");
static_assert(STANDARD_VECTOR_SIZE == EXG_VECTOR_SIZE, "chunks are STANDARD_VECTOR_SIZE rows");

// keeps the engine chunk (vectors + pinned payload) alive as long as a Vector references it
struct ExonChunkBuffer : public VectorBuffer {
	explicit ExonChunkBuffer(std::shared_ptr<exon_scan::ExonChunk> keep_p)
	    : VectorBuffer(VectorBufferType::OPAQUE_BUFFER), keep(std::move(keep_p)) {
	}
	std::shared_ptr<exon_scan::ExonChunk> keep;
};

struct RealDuck {
	using idx_t = duckdb::idx_t;
	using LogicalType = duckdb::LogicalType;
	using DataChunk = duckdb::DataChunk;
	using FunctionData = duckdb::TableFunctionData;
	using GlobalTableFunctionState = duckdb::GlobalTableFunctionState;
	using LocalTableFunctionState = duckdb::LocalTableFunctionState;
	using TableFilter = duckdb::TableFilter;
	using ConstantFilter = duckdb::ConstantFilter;
	using ConjunctionFilter = duckdb::ConjunctionFilter; // base of ConjunctionAndFilter / ConjunctionOrFilter
	using TableFilterSet = duckdb::TableFilterSet;
	using TableFilterType = duckdb::TableFilterType;
	static constexpr idx_t RowId = COLUMN_IDENTIFIER_ROW_ID;
	static constexpr idx_t VectorSize = STANDARD_VECTOR_SIZE;

	// MAP(key, value) where the DuckDB at hand has it (v0.8.1 does: LogicalType::MAP(LogicalType, LogicalType), LogicalTypeId::MAP —
	// a LIST(STRUCT(key, value)) physically), found by overload resolution so that a header without it still compiles: there the
	// column is the LIST(STRUCT(key, value)) it is laid out as
	template <class T>
	static auto MakeMap(const T &key, const T &value, int) -> decltype(T::MAP(key, value)) {
		return T::MAP(key, value);
	}
	template <class T>
	static T MakeMap(const T &key, const T &value, long) {
		child_list_t<T> fields;
		fields.emplace_back("key", key);
		fields.emplace_back("value", value);
		return T::LIST(T::STRUCT(std::move(fields)));
	}
	template <class E>
	static auto MapTypeId(int) -> decltype(E::MAP) {
		return E::MAP;
	}
	template <class E>
	static E MapTypeId(long) {
		return E::LIST;
	}

	// module.cpp:126-147 (there: ArrowTableFunction::GetArrowLogicalType over the Arrow schema)
	static LogicalType ToLogical(const exg_type &t) {
		switch (t.type) {
		case EXG_TYPE_MAP: // children[0]: the STRUCT of key and value (read_gtf's attributes)
			return MakeMap<LogicalType>(ToLogical(t.children[0].children[0]), ToLogical(t.children[0].children[1]), 0);
		case EXG_TYPE_BIGINT:
			return LogicalType::BIGINT;
		case EXG_TYPE_FLOAT:
			return LogicalType::FLOAT;
		case EXG_TYPE_INTEGER:
			return LogicalType::INTEGER;
		case EXG_TYPE_BOOLEAN:
			return LogicalType::BOOLEAN;
		case EXG_TYPE_LIST:
			return LogicalType::LIST(ToLogical(t.children[0]));
		case EXG_TYPE_STRUCT: {
			child_list_t<LogicalType> fields;
			for (int i = 0; i < t.n_children; i++) {
				fields.emplace_back(t.children[i].name, ToLogical(t.children[i]));
			}
			return LogicalType::STRUCT(std::move(fields));
		}
		default:
			return LogicalType::VARCHAR;
		}
	}

	// an engine vector as a DuckDB Vector that references the engine's host buffers (zero-copy)
	static void Wrap(Vector &vec, const LogicalType &type, const exg_vector &src, const buffer_ptr<VectorBuffer> &keep) {
		if (src.validity) {
			FlatVector::Validity(vec).Initialize(reinterpret_cast<validity_t *>(src.validity));
		}
		if (type.id() == MapTypeId<LogicalTypeId>(0)) { // (a MAP is a LIST of STRUCT(key, value): LIST's layout and accessors)
			FlatVector::SetData(vec, data_ptr_cast(src.data));
			auto &child = ListVector::GetEntry(vec);
			Wrap(child, ListType::GetChildType(type), src.children[0], keep);
			ListVector::SetListSize(vec, src.children[0].length);
			return;
		}
		switch (type.id()) {
		case LogicalTypeId::LIST: {
			FlatVector::SetData(vec, data_ptr_cast(src.data)); // list_entry_t[], offsets relative to this chunk's child
			auto &child = ListVector::GetEntry(vec);
			Wrap(child, ListType::GetChildType(type), src.children[0], keep);
			ListVector::SetListSize(vec, src.children[0].length);
			break;
		}
		case LogicalTypeId::STRUCT: {
			auto &entries = StructVector::GetEntries(vec);
			auto &fields = StructType::GetChildTypes(type);
			for (idx_t i = 0; i < entries.size(); i++) {
				Wrap(*entries[i], fields[i].second, src.children[i], keep);
			}
			break;
		}
		case LogicalTypeId::VARCHAR:
			FlatVector::SetData(vec, data_ptr_cast(src.data)); // string_t[]; payload kept alive through the aux buffer
			vec.SetAuxiliary(keep);
			break;
		default:
			FlatVector::SetData(vec, data_ptr_cast(src.data));
			vec.SetAuxiliary(keep);
			break;
		}
	}
	static void Reference(DataChunk &out, idx_t col, const LogicalType &type, const exg_vector &src,
	                      std::shared_ptr<exon_scan::ExonChunk> keep) {
		Wrap(out.data[col], type, src, make_buffer<ExonChunkBuffer>(std::move(keep)));
	}
	static void SetCardinality(DataChunk &out, idx_t n) {
		out.SetCardinality(n);
	}
	static std::string ComparisonOperator(const ConstantFilter &f) {
		return ExpressionTypeToOperator(f.comparison_type);
	}
	static std::string ConstantSQL(const ConstantFilter &f) {
		return f.constant.ToSQLString();
	}
};

using TF = exon_scan::ExonTableFunction<RealDuck>;

// exon/include/exon/arrow_table_function/module.hpp:29-35
struct WTArrowTableScanInfo : public TableFunctionInfo {
	explicit WTArrowTableScanInfo(string file_type_p) : file_type(std::move(file_type_p)) {
	}
	string file_type;
};

static unique_ptr<FunctionData> FileTypeBind(ClientContext &, TableFunctionBindInput &input,
                                             vector<LogicalType> &return_types, vector<string> &names) {
	auto &info = input.info->Cast<WTArrowTableScanInfo>();
	string compression;
	for (auto &kv : input.named_parameters) {
		if (kv.first == "compression") {
			compression = kv.second.GetValue<string>();
		}
	}
	std::vector<LogicalType> types;
	std::vector<std::string> col_names;
	// vcf_query(path, region): the second positional argument
	const string region = input.inputs.size() > 1 ? input.inputs[1].GetValue<string>() : string();
	auto result = TF::Bind(input.inputs[0].GetValue<string>(), compression, info.file_type, types, col_names, region);
	for (auto &t : types) {
		return_types.push_back(t);
	}
	for (auto &n : col_names) {
		names.push_back(n);
	}
	return unique_ptr<FunctionData>(result.release());
}

static unique_ptr<GlobalTableFunctionState> InitGlobal(ClientContext &, TableFunctionInitInput &input) {
	auto &data = input.bind_data->Cast<TF::BindData>();
	std::vector<idx_t> column_ids(input.column_ids.begin(), input.column_ids.end());
	return unique_ptr<GlobalTableFunctionState>(TF::InitGlobal(data, column_ids, input.filters.get()).release());
}

static unique_ptr<LocalTableFunctionState> InitLocal(ExecutionContext &, TableFunctionInitInput &input,
                                                     GlobalTableFunctionState *gs) {
	return unique_ptr<LocalTableFunctionState>(
	    TF::InitLocal(input.bind_data->Cast<TF::BindData>(), gs->Cast<TF::GlobalState>()).release());
}

static void Scan(ClientContext &, TableFunctionInput &input, DataChunk &output) {
	if (!input.local_state) { // module.cpp:259-261
		return;
	}
	TF::Scan(input.bind_data->Cast<TF::BindData>(), input.global_state->Cast<TF::GlobalState>(),
	         &input.local_state->Cast<TF::LocalState>(), output);
}

static idx_t GetBatchIndex(ClientContext &, const FunctionData *, LocalTableFunctionState *ls, GlobalTableFunctionState *) {
	return TF::BatchIndex(ls->Cast<TF::LocalState>());
}

// module.cpp:307 (there: ArrowTableFunction::ArrowScanCardinality = a NodeStatistics without an estimate)
static unique_ptr<NodeStatistics> Cardinality(ClientContext &, const FunctionData *bind_data) {
	const idx_t rows = TF::EstimatedCardinality(bind_data->Cast<TF::BindData>());
	return rows ? make_uniq<NodeStatistics>(rows) : make_uniq<NodeStatistics>();
}

// module.cpp:296-318
// region: the function takes (VARCHAR path, VARCHAR region) — exon_extension.cpp:75-77
static void Register(const string &name, const string &file_type, DatabaseInstance &db, bool region = false) {
	vector<LogicalType> arguments = {LogicalType::VARCHAR};
	if (region) {
		arguments.push_back(LogicalType::VARCHAR);
	}
	TableFunction scan(name, arguments, Scan, FileTypeBind, InitGlobal, InitLocal);
	if (!region) {
		scan.named_parameters["compression"] = LogicalType::VARCHAR;
	}
	scan.function_info = make_shared<WTArrowTableScanInfo>(file_type);
	scan.cardinality = Cardinality;
	scan.get_batch_index = GetBatchIndex;
	scan.projection_pushdown = true;
	scan.filter_pushdown = true; // like the reference (module.cpp:311); the predicate runs on the device
	ExtensionUtil::RegisterFunction(db, scan);
}

// module.cpp:320-382
static unique_ptr<TableRef> ReplacementScan(ClientContext &, const string &table_name, ReplacementScanData *) {
	const string fn = TF::ReplacementFunction(table_name);
	if (fn.empty()) {
		return nullptr;
	}
	auto ref = make_uniq<TableFunctionRef>();
	vector<unique_ptr<ParsedExpression>> children;
	children.push_back(make_uniq<ConstantExpression>(Value(table_name)));
	ref->function = make_uniq<FunctionExpression>(fn, std::move(children));
	return std::move(ref);
}

// fastq_functions/module.cpp:28-54: quality_score_string_to_list(VARCHAR) -> LIST(INTEGER), one value per byte, c - 33.
// The reference goes through Value / SetValue per row; this writes the list entries and the child vector directly.  A NULL
// string gives a NULL list (the reference's GetValue path has no defined answer for it: StringValue::Get of a NULL).
static void QualityScoreStringToList(DataChunk &args, ExpressionState &, Vector &result) {
	const idx_t count = args.size();
	UnifiedVectorFormat in;
	args.data[0].ToUnifiedFormat(count, in);
	auto strings = reinterpret_cast<const string_t *>(in.data);
	result.SetVectorType(VectorType::FLAT_VECTOR);
	auto entries = FlatVector::GetData<list_entry_t>(result);
	idx_t total = 0;
	for (idx_t i = 0; i < count; i++) {
		const idx_t k = in.sel->get_index(i);
		total += in.validity.RowIsValid(k) ? strings[k].GetSize() : 0;
	}
	ListVector::Reserve(result, total);
	auto values = FlatVector::GetData<int32_t>(ListVector::GetEntry(result));
	idx_t at = 0;
	for (idx_t i = 0; i < count; i++) {
		const idx_t k = in.sel->get_index(i);
		if (!in.validity.RowIsValid(k)) {
			FlatVector::SetNull(result, i, true);
			entries[i].offset = at;
			entries[i].length = 0;
			continue;
		}
		const idx_t n = strings[k].GetSize();
		exon_scan::QualityScores(strings[k].GetData(), n, values + at);
		entries[i].offset = at;
		entries[i].length = n;
		at += n;
	}
	ListVector::SetListSize(result, total);
}

// sequence_functions/module.cpp:30-121, :168-362: complement, reverse_complement (what the reference computes: A->C, T->G,
// C->A, G->T, order kept), transcribe, reverse_transcribe, translate_dna_to_aa.  The rules are csrc/exg_seqfn.hpp's; an
// invalid row throws the reference's InvalidInputException text.  NULL in, NULL out (the reference's
// GetValue(...).ToString() would read a NULL of a flat vector as the text "NULL").
static void SequenceMapFunction(uint32_t op, DataChunk &args, Vector &result) {
	const idx_t count = args.size();
	UnifiedVectorFormat in;
	args.data[0].ToUnifiedFormat(count, in);
	auto strings = reinterpret_cast<const string_t *>(in.data);
	result.SetVectorType(VectorType::FLAT_VECTOR);
	auto out = FlatVector::GetData<string_t>(result);
	std::string buf;
	for (idx_t i = 0; i < count; i++) {
		const idx_t k = in.sel->get_index(i);
		if (!in.validity.RowIsValid(k)) {
			FlatVector::SetNull(result, i, true);
			continue;
		}
		const idx_t n = strings[k].GetSize();
		buf.resize(exon_scan::SequenceOutputLength(op, n));
		const exon_scan::SequenceStatus st = exon_scan::SequenceMap(op, strings[k].GetData(), n, &buf[0]);
		if (st.code) {
			throw InvalidInputException(exon_scan::SequenceErrorText(st));
		}
		out[i] = StringVector::AddString(result, buf.data(), buf.size());
	}
}

// module.cpp:131-158: gc_content(VARCHAR) -> FLOAT.  A flat vector with every row on its own: the reference's early return
// on an empty string (:145) leaves the rest of its chunk unset, which is not reproduced.
static void GcContentFunction(DataChunk &args, ExpressionState &, Vector &result) {
	const idx_t count = args.size();
	UnifiedVectorFormat in;
	args.data[0].ToUnifiedFormat(count, in);
	auto strings = reinterpret_cast<const string_t *>(in.data);
	result.SetVectorType(VectorType::FLAT_VECTOR);
	auto out = FlatVector::GetData<float>(result);
	for (idx_t i = 0; i < count; i++) {
		const idx_t k = in.sel->get_index(i);
		if (!in.validity.RowIsValid(k)) {
			FlatVector::SetNull(result, i, true);
			out[i] = 0;
			continue;
		}
		out[i] = exon_scan::GcContent(strings[k].GetData(), strings[k].GetSize());
	}
}

// sam_functions/module.cpp:143-154: is_segmented .. is_supplementary (INTEGER) -> BOOLEAN, bit `which` of (uint16_t)flag
static void SamFlagFunction(uint32_t which, DataChunk &args, Vector &result) {
	const idx_t count = args.size();
	UnifiedVectorFormat in;
	args.data[0].ToUnifiedFormat(count, in);
	auto flags = reinterpret_cast<const int32_t *>(in.data);
	result.SetVectorType(VectorType::FLAT_VECTOR);
	auto out = FlatVector::GetData<bool>(result);
	for (idx_t i = 0; i < count; i++) {
		const idx_t k = in.sel->get_index(i);
		if (!in.validity.RowIsValid(k)) {
			FlatVector::SetNull(result, i, true);
			out[i] = false;
			continue;
		}
		out[i] = exon_scan::SamFlag(which, flags[k]);
	}
}

// alignment_functions/module.cpp:264-329: alignment_score / alignment_score_wfa_gap_affine -> FLOAT in the two-, six- and
// seven-argument forms (n_args), on the host scalar exon_scan::AlignmentScore over the rules of csrc/exg_alignfn.hpp.  The
// arguments are taken by position as the signatures name them: (text, pattern[, match], mismatch, gap_opening, gap_extension,
// memory_model); module.cpp:68-72 reads argument 4 for both gap values, which is not reproduced.  The parameter checks
// (AlignmentBindError: the reference's texts) run here, on every row's own values, before the row is scored: the reference makes
// them in a bind callback on constant arguments, which the declaration-only stand-in of ScalarFunction does not carry — so a
// call over zero rows raises nothing, and the parameters may differ from row to row.  NULL in any argument, NULL out.
static void AlignmentScoreFunction(idx_t n_args, DataChunk &args, Vector &result) {
	const idx_t count = args.size();
	UnifiedVectorFormat in[7];
	for (idx_t c = 0; c < n_args; c++) {
		args.data[c].ToUnifiedFormat(count, in[c]);
	}
	result.SetVectorType(VectorType::FLAT_VECTOR);
	auto out = FlatVector::GetData<float>(result);
	const idx_t first = n_args == 7 ? 3 : 2; // the column of `mismatch`
	for (idx_t i = 0; i < count; i++) {
		bool valid = true;
		idx_t k[7];
		for (idx_t c = 0; c < n_args; c++) {
			k[c] = in[c].sel->get_index(i);
			valid = valid && in[c].validity.RowIsValid(k[c]);
		}
		out[i] = 0;
		if (!valid) {
			FlatVector::SetNull(result, i, true);
			continue;
		}
		exon_scan::AlignmentParams prm;
		if (n_args > 2) {
			auto integer = [&](idx_t c) { return (int64_t) reinterpret_cast<const int32_t *>(in[c].data)[k[c]]; };
			const string_t &model = reinterpret_cast<const string_t *>(in[n_args - 1].data)[k[n_args - 1]];
			const std::string msg = exon_scan::AlignmentBindError(n_args == 7, n_args == 7 ? integer(2) : 0, integer(first), integer(first + 1),
			                                                      integer(first + 2), model.GetData(), model.GetSize());
			if (!msg.empty()) {
				throw InvalidInputException(msg);
			}
			prm.mismatch = (int32_t)integer(first), prm.gap_opening = (int32_t)integer(first + 1), prm.gap_extension = (int32_t)integer(first + 2);
		}
		const string_t &text = reinterpret_cast<const string_t *>(in[0].data)[k[0]];
		const string_t &pattern = reinterpret_cast<const string_t *>(in[1].data)[k[1]];
		if (exon_scan::AlignmentScore(text.GetData(), text.GetSize(), pattern.GetData(), pattern.GetSize(), prm, &out[i]) != EXG_OK) {
			throw InvalidInputException("alignment_score: the pair is longer than 2^21 bytes");
		}
	}
}

// exon_extension.cpp:81-93: both names, each a set of three signatures (module.cpp:308-329).  A set goes into the system
// catalog the way ExtensionUtil::RegisterFunction puts a single function there.
static void RegisterAlignmentScore(DatabaseInstance &db, const char *name) {
	ScalarFunctionSet set(name);
	const LogicalType V = LogicalType::VARCHAR, I = LogicalType::INTEGER;
	const vector<LogicalType> forms[] = {{V, V}, {V, V, I, I, I, V}, {V, V, I, I, I, I, V}};
	for (const auto &arguments : forms) {
		const idx_t n_args = arguments.size();
		set.AddFunction(ScalarFunction(name, arguments, LogicalType::FLOAT,
		                               [n_args](DataChunk &args, ExpressionState &, Vector &result) { AlignmentScoreFunction(n_args, args, result); }));
	}
	CreateScalarFunctionInfo info(std::move(set));
	Catalog::GetSystemCatalog(db).CreateFunction(CatalogTransaction::GetSystemTransaction(db), info);
}

// alignment_functions/module.cpp:150-247: alignment_string / alignment_string_wfa_gap_affine -> VARCHAR in the same three
// forms, on the host scalar exon_scan::AlignmentString: the run-length CIGAR of the optimum that the backtrace rule of
// csrc/exg_alignfn.hpp picks.  The checks (AlignmentStringBindError: the reference's texts; a match score below 0 is folded into
// the penalties) run per row, exactly as AlignmentScoreFunction makes them.  NULL in any argument, NULL out.
static void AlignmentStringFunction(idx_t n_args, DataChunk &args, Vector &result) {
	const idx_t count = args.size();
	UnifiedVectorFormat in[7];
	for (idx_t c = 0; c < n_args; c++) {
		args.data[c].ToUnifiedFormat(count, in[c]);
	}
	result.SetVectorType(VectorType::FLAT_VECTOR);
	auto out = FlatVector::GetData<string_t>(result);
	const idx_t first = n_args == 7 ? 3 : 2; // the column of `mismatch`
	std::string cigar;
	for (idx_t i = 0; i < count; i++) {
		bool valid = true;
		idx_t k[7];
		for (idx_t c = 0; c < n_args; c++) {
			k[c] = in[c].sel->get_index(i);
			valid = valid && in[c].validity.RowIsValid(k[c]);
		}
		if (!valid) {
			FlatVector::SetNull(result, i, true);
			continue;
		}
		exon_scan::AlignmentParams prm;
		if (n_args > 2) {
			auto integer = [&](idx_t c) { return (int64_t) reinterpret_cast<const int32_t *>(in[c].data)[k[c]]; };
			const string_t &model = reinterpret_cast<const string_t *>(in[n_args - 1].data)[k[n_args - 1]];
			const std::string msg = exon_scan::AlignmentStringBindError(n_args == 7, n_args == 7 ? integer(2) : 0, integer(first), integer(first + 1),
			                                                            integer(first + 2), model.GetData(), model.GetSize(), &prm);
			if (!msg.empty()) {
				throw InvalidInputException(msg);
			}
		}
		const string_t &text = reinterpret_cast<const string_t *>(in[0].data)[k[0]];
		const string_t &pattern = reinterpret_cast<const string_t *>(in[1].data)[k[1]];
		const int rc = exon_scan::AlignmentString(text.GetData(), text.GetSize(), pattern.GetData(), pattern.GetSize(), prm, &cigar);
		if (rc == EXG_E_NOMEM) {
			throw InvalidInputException(exg::alignfn::kHistoryLimitText);
		}
		if (rc != EXG_OK) {
			throw InvalidInputException("alignment_string: the pair is longer than 2^21 bytes");
		}
		out[i] = StringVector::AddString(result, cigar.data(), cigar.size());
	}
}

// exon_extension.cpp:82-91: both names, each a set of the three signatures of the score, returning VARCHAR
static void RegisterAlignmentString(DatabaseInstance &db, const char *name) {
	ScalarFunctionSet set(name);
	const LogicalType V = LogicalType::VARCHAR, I = LogicalType::INTEGER;
	const vector<LogicalType> forms[] = {{V, V}, {V, V, I, I, I, V}, {V, V, I, I, I, I, V}};
	for (const auto &arguments : forms) {
		const idx_t n_args = arguments.size();
		set.AddFunction(ScalarFunction(name, arguments, LogicalType::VARCHAR,
		                               [n_args](DataChunk &args, ExpressionState &, Vector &result) { AlignmentStringFunction(n_args, args, result); }));
	}
	CreateScalarFunctionInfo info(std::move(set));
	Catalog::GetSystemCatalog(db).CreateFunction(CatalogTransaction::GetSystemTransaction(db), info);
}

// sam_functions/module.cpp:32-77: parse_cigar(VARCHAR) -> LIST(STRUCT(op VARCHAR, len INTEGER)) on the host scalar
// exon_scan::ParseCigar over the rules of csrc/exg_cigarfn.hpp.  The list entries, the two STRUCT children and the one-letter
// strings are written directly, as QualityScoreStringToList writes its list.  The empty string and `*` give an empty list
// (the reference rejects the empty string; the scans hand `*` over as one).  NULL in, NULL out.
static void ParseCigarFunction(DataChunk &args, ExpressionState &, Vector &result) {
	const idx_t count = args.size();
	UnifiedVectorFormat in;
	args.data[0].ToUnifiedFormat(count, in);
	auto strings = reinterpret_cast<const string_t *>(in.data);
	result.SetVectorType(VectorType::FLAT_VECTOR);
	auto entries = FlatVector::GetData<list_entry_t>(result);
	std::vector<exon_scan::CigarOp> all, row;
	for (idx_t i = 0; i < count; i++) {
		const idx_t k = in.sel->get_index(i);
		entries[i].offset = all.size();
		entries[i].length = 0;
		if (!in.validity.RowIsValid(k)) {
			FlatVector::SetNull(result, i, true);
			continue;
		}
		if (exon_scan::ParseCigar(strings[k].GetData(), strings[k].GetSize(), &row).code) {
			throw InvalidInputException(exon_scan::ParseCigarErrorText(strings[k].GetData(), strings[k].GetSize()));
		}
		entries[i].length = row.size();
		all.insert(all.end(), row.begin(), row.end());
	}
	ListVector::Reserve(result, all.size());
	auto &fields = StructVector::GetEntries(ListVector::GetEntry(result));
	auto ops = FlatVector::GetData<string_t>(*fields[0]);
	auto lens = FlatVector::GetData<int32_t>(*fields[1]);
	for (idx_t j = 0; j < all.size(); j++) {
		ops[j] = StringVector::AddString(*fields[0], &all[j].op, 1);
		lens[j] = all[j].len;
	}
	ListVector::SetListSize(result, all.size());
}

// sam_functions/module.cpp:79-131: extract_from_cigar(VARCHAR, VARCHAR) -> STRUCT(sequence_start INTEGER, sequence_end
// INTEGER, sequence VARCHAR) on exon_scan::ExtractFromCigar: the sequence without a leading and a trailing insertion.  An
// absent CIGAR gives the whole sequence (the reference panics on it), insertions that exceed the sequence are an error (the
// reference panics in the slice).  NULL in either argument, NULL out.
static void ExtractFromCigarFunction(DataChunk &args, ExpressionState &, Vector &result) {
	const idx_t count = args.size();
	UnifiedVectorFormat in[2];
	args.data[0].ToUnifiedFormat(count, in[0]);
	args.data[1].ToUnifiedFormat(count, in[1]);
	result.SetVectorType(VectorType::FLAT_VECTOR);
	auto &fields = StructVector::GetEntries(result);
	auto starts = FlatVector::GetData<int32_t>(*fields[0]);
	auto ends = FlatVector::GetData<int32_t>(*fields[1]);
	auto slices = FlatVector::GetData<string_t>(*fields[2]);
	for (idx_t i = 0; i < count; i++) {
		const idx_t ks = in[0].sel->get_index(i), kc = in[1].sel->get_index(i);
		if (!in[0].validity.RowIsValid(ks) || !in[1].validity.RowIsValid(kc)) {
			FlatVector::SetNull(result, i, true);
			for (auto &field : fields) {
				FlatVector::SetNull(*field, i, true);
			}
			starts[i] = ends[i] = 0;
			continue;
		}
		const string_t &sequence = reinterpret_cast<const string_t *>(in[0].data)[ks];
		const string_t &cigar = reinterpret_cast<const string_t *>(in[1].data)[kc];
		const exon_scan::CigarStatus st = exon_scan::ExtractFromCigar(sequence.GetSize(), cigar.GetData(), cigar.GetSize(), &starts[i], &ends[i]);
		if (st.code) {
			throw InvalidInputException(exon_scan::ExtractFromCigarErrorText(st));
		}
		slices[i] = StringVector::AddString(*fields[2], sequence.GetData() + starts[i], (idx_t)(ends[i] - starts[i]));
	}
}

// gff_functions/module.cpp:29-84: gff_parse_attributes(VARCHAR) -> MAP(VARCHAR, VARCHAR) on the host scalar
// exon_scan::GffParseAttributes over the rules of csrc/exg_gffattr.hpp.  A MAP is a LIST(STRUCT(key, value)) physically: the list
// entries and the two children are written directly, as ParseCigarFunction writes its list.  Entries stay in field order and a
// repeated key stays a second entry.  NULL in, NULL out; a segment that is not key=value throws with the reference's text.
static void GffParseAttributesFunction(DataChunk &args, ExpressionState &, Vector &result) {
	const idx_t count = args.size();
	UnifiedVectorFormat in;
	args.data[0].ToUnifiedFormat(count, in);
	auto strings = reinterpret_cast<const string_t *>(in.data);
	result.SetVectorType(VectorType::FLAT_VECTOR);
	auto entries = FlatVector::GetData<list_entry_t>(result);
	struct Slice {
		idx_t row; // of `strings`
		exon_scan::GffAttribute at;
	};
	std::vector<Slice> all;
	std::vector<exon_scan::GffAttribute> row;
	for (idx_t i = 0; i < count; i++) {
		const idx_t k = in.sel->get_index(i);
		entries[i].offset = all.size();
		entries[i].length = 0;
		if (!in.validity.RowIsValid(k)) {
			FlatVector::SetNull(result, i, true);
			continue;
		}
		const exon_scan::GffAttributeStatus st = exon_scan::GffParseAttributes(strings[k].GetData(), strings[k].GetSize(), &row);
		if (st.code) {
			throw InvalidInputException(exon_scan::GffAttributeErrorText(strings[k].GetData(), st));
		}
		entries[i].length = row.size();
		for (const auto &at : row) {
			all.push_back(Slice {k, at});
		}
	}
	ListVector::Reserve(result, all.size());
	auto &fields = StructVector::GetEntries(ListVector::GetEntry(result));
	auto keys = FlatVector::GetData<string_t>(*fields[0]);
	auto values = FlatVector::GetData<string_t>(*fields[1]);
	for (idx_t j = 0; j < all.size(); j++) {
		const char *field = strings[all[j].row].GetData();
		keys[j] = StringVector::AddString(*fields[0], field + all[j].at.key_start, (idx_t)all[j].at.key_len);
		values[j] = StringVector::AddString(*fields[1], field + all[j].at.value_start, (idx_t)all[j].at.value_len);
	}
	ListVector::SetListSize(result, all.size());
}

// exon_extension.cpp:62-73, :81-93: the sequence scalars, the flag predicates, the alignment scores and strings, the two
// CIGAR scalars and gff_parse_attributes
static void RegisterScalars(DatabaseInstance &db) {
	RegisterAlignmentScore(db, "alignment_score");
	RegisterAlignmentScore(db, "alignment_score_wfa_gap_affine");
	RegisterAlignmentString(db, "alignment_string");
	RegisterAlignmentString(db, "alignment_string_wfa_gap_affine");
	static const struct {
		const char *name;
		uint32_t op;
	} kSequenceMaps[] = {{"complement", EXG_SEQ_COMPLEMENT},
	                     {"reverse_complement", EXG_SEQ_REVERSE_COMPLEMENT},
	                     {"transcribe", EXG_SEQ_TRANSCRIBE},
	                     {"reverse_transcribe", EXG_SEQ_REVERSE_TRANSCRIBE},
	                     {"translate_dna_to_aa", EXG_SEQ_TRANSLATE}};
	for (const auto &f : kSequenceMaps) {
		const uint32_t op = f.op;
		ExtensionUtil::RegisterFunction(
		    db, ScalarFunction(f.name, {LogicalType::VARCHAR}, LogicalType::VARCHAR,
		                       [op](DataChunk &args, ExpressionState &, Vector &result) { SequenceMapFunction(op, args, result); }));
	}
	ExtensionUtil::RegisterFunction(db, ScalarFunction("gc_content", {LogicalType::VARCHAR}, LogicalType::FLOAT, GcContentFunction));
	ExtensionUtil::RegisterFunction(
	    db, ScalarFunction("parse_cigar", {LogicalType::VARCHAR},
	                       LogicalType::LIST(LogicalType::STRUCT({{"op", LogicalType::VARCHAR}, {"len", LogicalType::INTEGER}})), ParseCigarFunction));
	ExtensionUtil::RegisterFunction(
	    db, ScalarFunction("extract_from_cigar", {LogicalType::VARCHAR, LogicalType::VARCHAR},
	                       LogicalType::STRUCT({{"sequence_start", LogicalType::INTEGER}, {"sequence_end", LogicalType::INTEGER}, {"sequence", LogicalType::VARCHAR}}),
	                       ExtractFromCigarFunction));
	// exon_extension.cpp:63-64; the return type through RealDuck::MakeMap, as read_gtf's attributes column gets it
	ExtensionUtil::RegisterFunction(db, ScalarFunction("gff_parse_attributes", {LogicalType::VARCHAR},
	                                                   RealDuck::MakeMap<LogicalType>(LogicalType::VARCHAR, LogicalType::VARCHAR, 0),
	                                                   GffParseAttributesFunction));
	for (uint32_t which = 0; which < (uint32_t)exg::seqfn::kSamFlagCount; which++) {
		ExtensionUtil::RegisterFunction(
		    db, ScalarFunction(exg::seqfn::kSamFlagNames[which], {LogicalType::INTEGER}, LogicalType::BOOLEAN,
		                       [which](DataChunk &args, ExpressionState &, Vector &result) { SamFlagFunction(which, args, result); }));
	}
}

// exon/src/exon_extension.cpp:25-96, restricted to the path
static void LoadInternal(DatabaseInstance &db) {
	for (const auto &reg : exon_scan::kRegistrations) {
		Register(reg.name, reg.file_type, db);
	}
	for (const auto &reg : exon_scan::kRegionRegistrations) { // vcf_query(path, region)
		Register(reg.name, reg.file_type, db, true);
	}
	RegisterScalars(db);
	// exon_extension.cpp:60 (FastqFunctions::GetQualityScoreStringToList)
	ExtensionUtil::RegisterFunction(db, ScalarFunction("quality_score_string_to_list", {LogicalType::VARCHAR},
	                                                   LogicalType::LIST(LogicalType::INTEGER), QualityScoreStringToList));
	DBConfig::GetConfig(db).replacement_scans.emplace_back(ReplacementScan);
}
} // namespace exon

extern "C" {
DUCKDB_EXTENSION_API void exon_init(duckdb::DatabaseInstance &db) { // exon_extension.cpp:110-116
	exon::LoadInternal(db);
}
DUCKDB_EXTENSION_API const char *exon_version() { // exon_extension.cpp:118-122
	return duckdb::DuckDB::LibraryVersion();
}
}
