// exon_table_function.hpp — the host glue of the drop-in: the reference's WTArrowTableFunction
// (exon/src/exon/arrow_table_function/module.cpp:75-318, exon/include/exon/arrow_table_function/module.hpp) re-designed on
// top of the reader-level C-ABI (include/exon_gpu.h), written ONCE against a traits struct `D` that names DuckDB's types:
//
//   * duckdb_shim/exon_extension.cpp instantiates it with DuckDB v0.8.1's own classes (the real `LOAD exon` binding; it
//     needs DuckDB's headers, which do not exist on the build box);
//   * csrc/testing/exon_tf_harness.cpp instantiates it with csrc/testing/duck_mini.hpp, the slice of that API restated for
//     the tests — so every line of logic below is compiled and exercised by the GPU test-suite, and the shim adds only the
//     adapters (how a LogicalType / a Vector is made in real DuckDB) and the registration calls.
//
// Same lifecycle as the reference — bind (schema from a reader that is closed again), init_global (FilterToString ->
// `filters`), init_local, scan (<= STANDARD_VECTOR_SIZE rows per call, zero rows = end) — with these deliberate differences
// (SURVEY.md Appendix B):
//   * no Arrow hop: the DataChunk's vectors reference the engine's host buffers (kept alive by the vector buffer);
//   * SEVERAL scan threads: the reference pins MaxThreads() to 1 (module.cpp:36 has an unused `max_threads = 6`).  Here
//     init_global plans byte-range shards (exg_plan_shards: as many as there are devices, when the input can be sharded and
//     is large enough) and MaxThreads() returns that number — an UPPER bound: DuckDB runs fewer scan threads when
//     `threads` is smaller or the pipeline is not parallel.  A scan thread therefore does not own a shard for life: whenever
//     its reader is exhausted (or it has none yet) it claims the next unclaimed shard and opens that shard's reader on that
//     shard's device, until no shard is left — one thread scans every shard in file order, N threads scan N shards at a
//     time on N GPUs, nothing exchanged between them.  COUNT(*) (only the row id projected) is counted per
//     shard and summed by DuckDB's aggregate;
//   * get_batch_index orders the chunks (shard-major, then the shard's device batches), so an order-preserving plan sees
//     the file order; a device batch (~256 MiB of input) is one DuckDB batch, and the index stays far below DuckDB's
//     per-pipeline increment (10^13) for any shard count the planner allows;
//   * FilterToString keeps the tree: every conjunction it renders, and every per-column entry of the TableFilterSet, goes
//     into parentheses.  The reference joins them bare (module.cpp:158-214), so `start<5 OR start>=9` on one column beside
//     `flag=99` on another is read back as `start<5 OR (start>=9 AND flag=99)` — rows DuckDB never sees again to reject.
//
// What D provides: the types FunctionData, GlobalTableFunctionState, LocalTableFunctionState, LogicalType, DataChunk,
// TableFilter, ConstantFilter, ConjunctionFilter, TableFilterSet, TableFilterType, idx_t, the constants
// RowId / VectorSize, and the adapters
//   static LogicalType ToLogical(const exg_type &);                                       (module.cpp:126-147)
//   static void Reference(DataChunk &, idx_t out_col, const LogicalType &, const exg_vector &, std::shared_ptr<ExonChunk>);
//   static void SetCardinality(DataChunk &, idx_t);
//   static std::string ComparisonOperator(const ConstantFilter &);   static std::string ConstantSQL(const ConstantFilter &);
#pragma once
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "exon_gpu.h"
#include "exg_alignfn.hpp"
#include "exg_cigarfn.hpp"
#include "exg_gffattr.hpp"
#include "exg_seqfn.hpp"

namespace exon_scan {

// one engine chunk: released when the last vector that references it is dropped
struct ExonChunk {
    exg_reader *reader = nullptr;
    exg_chunk chunk;
    ExonChunk() { memset(&chunk, 0, sizeof chunk); }
    ~ExonChunk() {
        if (chunk.keepalive) exg_release_chunk(reader, &chunk);
    }
    ExonChunk(const ExonChunk &) = delete;
    ExonChunk &operator=(const ExonChunk &) = delete;
};

template <class D>
struct ExonTableFunction {
    using idx_t = typename D::idx_t;
    using LogicalType = typename D::LogicalType;

    // module.cpp:29-41
    struct BindData : public D::FunctionData {
        std::string file_type;
        std::string compression;  // "auto_detect" when the named parameter is absent (module.cpp:85)
        std::string file_name;
        std::string region;  // vcf_query(path, region): the region text ("": not a region query); the reader is exg_open_region's
        std::vector<std::string> all_names;
        std::vector<LogicalType> all_types;
        uint64_t input_bytes = 0;        // size of the input files on disk (exg_reader_stats.input_bytes at bind)
        uint64_t input_compression = 0;  // 0 text, 1 gzip, 2 zstd, 3 bzip2
    };

    struct GlobalState : public D::GlobalTableFunctionState {
        std::vector<idx_t> column_ids;
        std::string filter_clause;
        uint64_t columns = 0;  // exg_open_args.columns: the projection as a mask (0 = all)
        uint64_t open_flags = 0;  // exg_open_args.flags
        bool count_only = false;
        uint32_t n_shards = 1;
        int devices[64];
        std::atomic<uint32_t> next_shard{0};
        idx_t MaxThreads() const override { return n_shards; }
    };

    struct LocalState : public D::LocalTableFunctionState {
        exg_reader *reader = nullptr;
        uint32_t shard = 0;
        uint64_t batch_no = 0;  // the device batch (of the current shard's reader) the last chunk came from
        bool counted = false;
        uint64_t count_remaining = 0;
        ~LocalState() override {
            if (reader) exg_close(reader);
        }
    };
    static constexpr unsigned kBatchBits = 24;  // device batches per shard: 2^24 x 256 MiB = 4 PiB

    static exg_reader *OpenReader(const BindData &d, const std::string &filter_clause, uint64_t columns, uint64_t flags, uint32_t shard, uint32_t n_shards, int device) {
        exg_open_args a;
        memset(&a, 0, sizeof a);
        a.filters = filter_clause.empty() ? nullptr : filter_clause.c_str();                // module.cpp:239-243
        a.path = d.file_name.c_str();
        a.file_format = d.file_type.c_str();
        a.compression = d.compression == "auto_detect" ? nullptr : d.compression.c_str();  // module.cpp:95-103
        a.batch_rows = D::VectorSize;                                                      // module.cpp:83
        a.shard_index = shard;
        a.shard_count = n_shards;
        a.device = device;
        a.columns = columns;  // projection_pushdown (module.cpp:310): only these columns' vectors cross PCIe
        a.flags = flags;
        exg_reader *r = nullptr;
        const int rc = d.region.empty() ? exg_open(&a, &r) : exg_open_region(&a, d.region.c_str(), &r);
        if (rc != EXG_OK) throw std::runtime_error(exg_last_error_message());  // module.cpp:105-108
        return r;
    }

    // module.cpp:75-156.  The reference learns the schema by opening a reader; so does this (and closes it again).
    // region (vcf_query's second argument): the bind opens with exg_open_region, so a missing index, a file that is not BGZF and a
    // region the index does not hold all fail here
    static std::unique_ptr<BindData> Bind(const std::string &file_name, const std::string &compression, const std::string &file_type,
                                          std::vector<LogicalType> &return_types, std::vector<std::string> &names, const std::string &region = "") {
        auto result = std::make_unique<BindData>();
        result->file_name = file_name;
        result->region = region;
        result->compression = compression.empty() ? "auto_detect" : compression;
        result->file_type = file_type;
        exg_reader *r = OpenReader(*result, "", 0, 0, 0, 1, 0);
        exg_schema sch;
        const int rc = exg_schema_of(r, &sch);
        if (rc == EXG_OK)
            for (int i = 0; i < sch.n_columns; i++) {
                return_types.push_back(D::ToLogical(*sch.tree[i]));  // (the trees are the reader's: convert before it closes)
                names.emplace_back(sch.names[i]);
            }
        const std::string why = rc == EXG_OK ? "" : exg_reader_error(r);
        exg_reader_stats st;
        if (exg_reader_stats_of(r, &st) == EXG_OK) result->input_bytes = st.input_bytes, result->input_compression = st.input_compression;
        exg_close(r);
        if (rc != EXG_OK) throw std::runtime_error("Failed to get schema: " + why);  // module.cpp:112-119
        result->all_names = names;
        result->all_types = return_types;
        return result;
    }

    static std::string Join(const std::vector<std::string> &v, const std::string &sep) {
        std::string out;
        for (size_t i = 0; i < v.size(); i++) out += (i ? sep : "") + v[i];
        return out;
    }

    // module.cpp:158-199: the predicate text the engine parses again (`filters` of exg_open / new_reader); parenthesised, unlike
    // the reference's, so that the text means the tree
    static std::string FilterToString(const typename D::TableFilter &filter, const std::string &column_name) {
        using T = typename D::TableFilterType;
        switch (filter.filter_type) {
            case T::CONSTANT_COMPARISON: {
                auto &cf = static_cast<const typename D::ConstantFilter &>(filter);
                return column_name + D::ComparisonOperator(cf) + D::ConstantSQL(cf);
            }
            case T::CONJUNCTION_AND:
            case T::CONJUNCTION_OR: {
                auto &cj = static_cast<const typename D::ConjunctionFilter &>(filter);
                std::vector<std::string> parts;
                for (auto &c : cj.child_filters) parts.push_back(FilterToString(*c, column_name));
                return "(" + Join(parts, filter.filter_type == T::CONJUNCTION_AND ? " AND " : " OR ") + ")";
            }
            case T::IS_NOT_NULL: return column_name + " IS NOT NULL";
            case T::IS_NULL: return column_name + " IS NULL";
            default: break;
        }
        throw std::runtime_error("FilterToString: filter type not implemented");
    }
    // module.cpp:201-214
    static std::string FilterToString(const typename D::TableFilterSet &set, const std::vector<idx_t> &column_ids,
                                      const std::vector<std::string> &column_names) {
        std::vector<std::string> parts;
        for (auto &f : set.filters) parts.push_back("(" + FilterToString(*f.second, column_names.at(column_ids.at(f.first))) + ")");
        return Join(parts, " AND ");
    }

    // module.cpp:216-255
    static std::unique_ptr<GlobalState> InitGlobal(const BindData &data, const std::vector<idx_t> &column_ids,
                                                   const typename D::TableFilterSet *filters) {
        auto gs = std::make_unique<GlobalState>();
        gs->column_ids = column_ids;
        gs->count_only = true;
        for (idx_t c : column_ids) {
            gs->count_only = gs->count_only && c == D::RowId;
            if (c != D::RowId && c < 63) gs->columns |= (uint64_t)1 << c;
        }
        // the scan is going to pull chunks (anything but COUNT(*)): a compressed input's decoded segments travel to the host from
        // the first one on, beside the decoder (include/exon_gpu.h: EXG_OPEN_CHUNKS)
        if (!gs->count_only) gs->open_flags |= EXG_OPEN_CHUNKS;
        if (filters) gs->filter_clause = FilterToString(*filters, column_ids, data.all_names);  // module.cpp:222-226
        exg_open_args a;
        memset(&a, 0, sizeof a);
        a.path = data.file_name.c_str();
        a.file_format = data.file_type.c_str();
        a.compression = data.compression == "auto_detect" ? nullptr : data.compression.c_str();
        a.filters = gs->filter_clause.empty() ? nullptr : gs->filter_clause.c_str();
        uint32_t n = 1;
        if (!data.region.empty()) gs->devices[0] = 0;  // a region reader is one shard: MaxThreads() == 1
        else if (exg_plan_shards(&a, &n, gs->devices, 64) != EXG_OK) throw std::runtime_error(exg_last_error_message());
        gs->n_shards = n;
        return gs;
    }

    // one per scan thread (<= MaxThreads(), and DuckDB may run fewer): the shards are claimed in Scan, one after the other
    static std::unique_ptr<LocalState> InitLocal(const BindData &, GlobalState &) { return std::make_unique<LocalState>(); }

    // the next unclaimed shard becomes this thread's: false when none is left
    static bool ClaimShard(const BindData &data, GlobalState &gs, LocalState &ls) {
        if (ls.reader) {
            exg_close(ls.reader);  // (chunks it handed out keep their buffers alive on their own)
            ls.reader = nullptr;
        }
        const uint32_t shard = gs.next_shard.fetch_add(1);
        if (shard >= gs.n_shards) {
            gs.next_shard.store(gs.n_shards);  // (no wrap-around, however often exhausted threads ask)
            return false;
        }
        ls.shard = shard;
        ls.batch_no = 0;
        ls.counted = false;
        ls.reader = OpenReader(data, gs.filter_clause, gs.columns, gs.open_flags, shard, gs.n_shards, gs.devices[shard]);
        return true;
    }

    // module.cpp:257-294: leaves output.size() == 0 at the end of the (thread's) stream — here: when its reader is
    // exhausted AND no shard is left to claim
    static void Scan(const BindData &data, GlobalState &gs, LocalState *ls, typename D::DataChunk &output) {
        if (!ls) return;  // (module.cpp:259-261)
        D::SetCardinality(output, 0);
        for (;;) {
            if (!ls->reader && !ClaimShard(data, gs, *ls)) return;
            if (gs.count_only) {
                if (!ls->counted) {
                    if (exg_count_only(ls->reader, &ls->count_remaining) != EXG_OK) throw std::runtime_error(exg_reader_error(ls->reader));
                    ls->counted = true;
                }
                if (ls->count_remaining == 0) {
                    if (!ClaimShard(data, gs, *ls)) return;
                    continue;
                }
                const idx_t n = ls->count_remaining < (uint64_t)D::VectorSize ? (idx_t)ls->count_remaining : (idx_t)D::VectorSize;
                ls->count_remaining -= n;
                D::SetCardinality(output, n);
                return;
            }
            auto buf = std::make_shared<ExonChunk>();
            buf->reader = ls->reader;
            if (exg_next_chunk(ls->reader, &buf->chunk) != EXG_OK) throw std::runtime_error(exg_reader_error(ls->reader));
            if (buf->chunk.n_rows == 0) {
                if (!ClaimShard(data, gs, *ls)) return;
                continue;
            }
            D::SetCardinality(output, (idx_t)buf->chunk.n_rows);
            for (size_t i = 0; i < gs.column_ids.size(); i++) {
                const idx_t col = gs.column_ids[i];
                if (col == D::RowId) continue;
                D::Reference(output, (idx_t)i, data.all_types.at(col), *buf->chunk.vectors[col], buf);
            }
            ls->batch_no = buf->chunk.batch_no;
            return;
        }
    }

    // TableFunction::cardinality (registered at module.cpp:307: ArrowTableFunction::ArrowScanCardinality, which returns a
    // NodeStatistics without an estimate — the reference cannot know: its input is an opaque Arrow stream).  The reader knows
    // the input's size on disk, so the planner gets an estimate here: bytes (x the usual deflate / zstd ratio of sequence text)
    // / the usual bytes per row of the format.  0 = unknown (no estimate is set, like the reference).  Only the join order
    // and the sink's sizing look at it; no result depends on it.
    static idx_t EstimatedCardinality(const BindData &d) {
        if (!d.input_bytes) return 0;
        const double text = (double)d.input_bytes * (d.input_compression ? 3.5 : 1.0);
        const double per_row = d.file_type == "fastq" ? 300.0 : d.file_type == "vcf" ? 120.0 : d.file_type == "bam" ? 350.0 : d.file_type == "bed" ? 40.0 : d.file_type == "sam" ? 400.0 : d.file_type == "gtf" ? 250.0 :
                               d.file_type == "bcf" ? 50.0 : 4096.0;  // (bcf: decoded BCF bytes of a single-sample record, a third of its line)
        const double rows = text / per_row;
        return rows < 1 ? (idx_t)1 : (idx_t)rows;
    }

    // TableFunction::get_batch_index: the chunks of shard s come before those of shard s + 1, a shard's device batches in
    // their order; the chunks of one device batch share an index (they are one DuckDB batch).  Non-decreasing per scan
    // thread: a thread claims shards in increasing order.  64 shards x 2^24 stays below 1.1e9 (DuckDB's pipelines are 1e13 apart).
    static idx_t BatchIndex(const LocalState &ls) {
        const uint64_t b = ls.batch_no < ((uint64_t)1 << kBatchBits) ? ls.batch_no : ((uint64_t)1 << kBatchBits) - 1;
        return ((idx_t)ls.shard << kBatchBits) + (idx_t)b;
    }

    // module.cpp:320-382 on rust/src/arrow_reader.rs:173-197 (`replacement_scan`, same symbol as exon/include/rust.hpp:48):
    // the table function that replaces a bare 'file' reference, or "" when the name is not one of ours
    static std::string ReplacementFunction(const std::string &table_name) {
        std::string lower = table_name;
        for (char &c : lower) c = (char)tolower((unsigned char)c);
        const ReplacementScanResult res = replacement_scan(lower.c_str());
        if (!res.file_type) return "";
        const std::string ft = res.file_type;
        if (ft == "FASTA") return "read_fasta";
        if (ft == "FASTQ") return "read_fastq";
        if (ft == "VCF") return "read_vcf_file_records";
        if (ft == "BAM") return "read_bam_file_records";
        if (ft == "BED") return "read_bed_file";
        if (ft == "BCF") return "read_bcf_file_records";
        if (ft == "GTF") return "read_gtf";
        return "";
    }
};

// quality_score_string_to_list (exon/src/exon/fastq_functions/module.cpp:28-54, registered at exon_extension.cpp:60): one INTEGER
// per byte of the string, `c - 33` with `char` signed as on x86-64.  The per-row arithmetic of the SQL scalar the shim registers
// (host loop: the function runs on whatever VARCHAR vector DuckDB hands it); exg_quality_score_list is the same op on a scan
// column that is still in HBM.
static inline void QualityScores(const char *s, size_t n, int32_t *out) {
    for (size_t i = 0; i < n; i++) out[i] = (int32_t)(signed char)s[i] - 33;
}

// The sequence scalars (exon/src/exon/sequence_functions/module.cpp:30-370) and the SAM flag predicates
// (sam_functions/module.cpp:143-154): the per-row arithmetic of the SQL scalars the shim registers, on the tables of
// exg_seqfn.hpp (exg_sequence_op is the same rules on a scan column that is still in HBM).  A status instead of an
// exception: the caller formats the reference's text with SequenceErrorText.
struct SequenceStatus {
    uint32_t code = EXG_PE_NONE;  // EXG_PE_SEQ_*
    uint64_t offset = 0;          // of the bad byte / codon; 0 for the length error
    uint64_t length = 0;          // of the row
    uint8_t bytes[4] = {0, 0, 0, 0};
};
static inline size_t SequenceOutputLength(uint32_t op, size_t n) { return (size_t)exg::seqfn::output_length(op, n); }
// the five VARCHAR -> VARCHAR functions (op = EXG_SEQ_COMPLEMENT .. EXG_SEQ_TRANSLATE); out holds SequenceOutputLength(op, n) bytes
static inline SequenceStatus SequenceMap(uint32_t op, const char *s, size_t n, char *out) {
    namespace sf = exg::seqfn;
    SequenceStatus st;
    st.length = n;
    const uint8_t *u = reinterpret_cast<const uint8_t *>(s);
    if (op == EXG_SEQ_TRANSLATE) {
        if (n % 3) {
            st.code = EXG_PE_SEQ_LENGTH;
            return st;
        }
        for (size_t i = 0; i < n / 3; i++) {
            const uint8_t *c = u + 3 * i;
            if (!sf::codon_ok(c[0], c[1], c[2])) {
                st.code = EXG_PE_SEQ_CODON, st.offset = 3 * i;
                memcpy(st.bytes, c, 3);
                return st;
            }
            out[i] = sf::codon_aa(sf::codon_index(c[0], c[1], c[2]));
        }
        return st;
    }
    const sf::ByteMap m = sf::byte_map(op);
    for (size_t i = 0; i < n; i++) {
        if (!sf::base_ok(m.from, u[i])) {
            st.code = EXG_PE_SEQ_INVALID_CHARACTER, st.offset = i, st.bytes[0] = u[i];
            return st;
        }
        out[i] = (char)sf::base_to(m.to, u[i]);
    }
    return st;
}
static inline float GcContent(const char *s, size_t n) {
    uint32_t count = 0;
    for (size_t i = 0; i < n; i++) count += exg::seqfn::is_gc((uint8_t)s[i]) ? 1u : 0u;
    return exg::seqfn::gc_ratio(count, (uint32_t)n);
}
static inline std::string SequenceErrorText(const SequenceStatus &st) {
    char buf[96];
    const size_t k = exg::seqfn::format_error(st.code, st.bytes, st.length, buf, sizeof buf);
    return std::string(buf, k);
}
// is_segmented .. is_supplementary: `which` indexes exg::seqfn::kSamFlagNames
static inline bool SamFlag(uint32_t which, int32_t flag) { return exg::seqfn::sam_flag(which, flag); }

// alignment_score / alignment_score_wfa_gap_affine (exon/src/exon/alignment_functions/module.cpp:264-329): the score of the
// optimal global gap-affine alignment, on the rules and the recurrences of exg_alignfn.hpp (exg_align_score is the same on two
// scan columns that are still in HBM).  The exact wavefront algorithm with whole wavefronts of the last max(x, o + e) + 1
// scores: O((n + m) * depth) memory, O(penalty * width) time.
struct AlignmentParams {
    int32_t mismatch = exg::alignfn::kDefaultMismatch;
    int32_t gap_opening = exg::alignfn::kDefaultGapOpening;
    int32_t gap_extension = exg::alignfn::kDefaultGapExtension;
};
// The bind-time checks of the SQL forms, by position as the signatures name them (module.cpp:68-72 reads argument 4 for both
// gap values; that slip is not reproduced).  has_match: the seven-argument form.  "" or the exception's text.
static inline std::string AlignmentBindError(bool has_match, int64_t match, int64_t mismatch, int64_t gap_opening, int64_t gap_extension,
                                             const char *memory_model, size_t memory_model_len) {
    namespace af = exg::alignfn;
    if (has_match && match > 0) return af::kMatchPositiveText;
    if (has_match && match < 0) return af::kMatchNegativeText;
    if (!af::params_ok(mismatch, gap_opening, gap_extension)) return af::kParamRangeText;
    if (!af::memory_model_ok(memory_model, memory_model_len)) return std::string(af::kMemoryModelPrefix) + std::string(memory_model, memory_model_len);
    return std::string();
}
// EXG_OK and *score; EXG_E_INVALID_ARG for parameters outside their limits, EXG_E_CAPACITY for a pair longer than
// exg::alignfn::kMaxPairBytes (2^21)
static inline int AlignmentScore(const char *text, size_t n_, const char *pattern, size_t m_, const AlignmentParams &prm, float *score) {
    namespace af = exg::alignfn;
    if (!af::params_ok(prm.mismatch, prm.gap_opening, prm.gap_extension)) return EXG_E_INVALID_ARG;
    if ((uint64_t)n_ + (uint64_t)m_ > af::kMaxPairBytes) return EXG_E_CAPACITY;
    const int32_t n = (int32_t)n_, m = (int32_t)m_;
    const int32_t x = prm.mismatch, o = prm.gap_opening, e = prm.gap_extension;
    const int32_t rm = (int32_t)af::m_ring_depth(x, o, e), rg = (int32_t)af::gap_ring_depth(e);
    const int32_t nd = n + m + 1;  // diagonal k = h - v lives at index d = k + m
    const int32_t bound = (int32_t)af::penalty_bound(o, e, n, m);
    std::vector<int32_t> M((size_t)rm * nd, af::kNone), I((size_t)rg * nd, af::kNone), D((size_t)rg * nd, af::kNone);
    auto extend = [&](int32_t h, int32_t k) {
        int32_t v = h - k;
        while (h < n && v < m) {
            if (n - h >= 8 && m - v >= 8) {
                uint64_t a, b;
                memcpy(&a, text + h, 8), memcpy(&b, pattern + v, 8);
                const int32_t c = (int32_t)af::equal_prefix8(a, b);
                h += c, v += c;
                if (c < 8) break;
            } else {
                if (text[h] != pattern[v]) break;
                h++, v++;
            }
        }
        return h;
    };
    int32_t lo = m, hi = m;  // the diagonals any wavefront has reached so far
    for (int32_t s = 0; s <= bound; s++) {
        const int32_t from = s ? (lo > 0 ? lo - 1 : 0) : m, to = s ? (hi < nd - 1 ? hi + 1 : nd - 1) : m;
        const int32_t *m_sub = s >= x ? &M[(size_t)((s - x) % rm) * nd] : nullptr;
        const int32_t *m_open = s >= o + e ? &M[(size_t)((s - o - e) % rm) * nd] : nullptr;
        const int32_t *i_prev = s >= e ? &I[(size_t)((s - e) % rg) * nd] : nullptr, *d_prev = s >= e ? &D[(size_t)((s - e) % rg) * nd] : nullptr;
        int32_t *m_now = &M[(size_t)(s % rm) * nd], *i_now = &I[(size_t)(s % rg) * nd], *d_now = &D[(size_t)(s % rg) * nd];
        for (int32_t d = from; d <= to; d++) {
            const int32_t k = d - m;
            af::Cell c = af::cell(m_open && d > 0 ? m_open[d - 1] : af::kNone, i_prev && d > 0 ? i_prev[d - 1] : af::kNone,
                                  m_open && d < nd - 1 ? m_open[d + 1] : af::kNone, d_prev && d < nd - 1 ? d_prev[d + 1] : af::kNone,
                                  m_sub ? m_sub[d] : af::kNone, k, n, m);
            if (!s) c.m = 0;
            if (c.m >= 0) {
                c.m = extend(c.m, k);
                lo = d < lo ? d : lo, hi = d > hi ? d : hi;
            }
            i_now[d] = c.i, d_now[d] = c.d, m_now[d] = c.m;
        }
        if (m_now[n] >= n) {
            *score = af::score_of((uint32_t)s);
            return EXG_OK;
        }
    }
    return EXG_E_INVALID_ARG;  // (unreachable: the bound is an alignment's penalty)
}

// alignment_string / alignment_string_wfa_gap_affine (exon/src/exon/alignment_functions/module.cpp:150-247): the run-length
// CIGAR of ONE optimal global gap-affine alignment, chosen by the backtrace rule of exg_alignfn.hpp (exg_align_string is the
// same on two scan columns that are still in HBM).  The bind-time checks of the SQL forms; unlike the score, a match score
// below 0 is folded into the penalties, and *prm gets the penalties the rule runs on.  "" or the exception's text.
static inline std::string AlignmentStringBindError(bool has_match, int64_t match, int64_t mismatch, int64_t gap_opening, int64_t gap_extension,
                                                   const char *memory_model, size_t memory_model_len, AlignmentParams *prm) {
    namespace af = exg::alignfn;
    if (has_match && match > 0) return af::kMatchPositiveText;
    if (!af::params_ok(mismatch, gap_opening, gap_extension)) return af::kStringParamRangeText;
    if (has_match && match < -af::kMaxParam) return af::kStringParamRangeText;  // no folded gap_extension passes; the products below stay small
    const int64_t a = has_match ? match : 0;
    const int64_t x = a ? af::fold_mismatch(a, mismatch) : mismatch, o = a ? af::fold_gap_opening(a, gap_opening) : gap_opening,
                  e = a ? af::fold_gap_extension(a, gap_extension) : gap_extension;
    if (!af::params_ok(x, o, e)) return af::kStringParamRangeText;
    if (!af::memory_model_ok(memory_model, memory_model_len)) return std::string(af::kMemoryModelPrefix) + std::string(memory_model, memory_model_len);
    prm->mismatch = (int32_t)x, prm->gap_opening = (int32_t)o, prm->gap_extension = (int32_t)e;
    return std::string();
}
// EXG_OK and *out (emptied first); EXG_E_INVALID_ARG for parameters outside their limits, EXG_E_CAPACITY for a pair longer than
// exg::alignfn::kMaxPairBytes, EXG_E_NOMEM when the kept wavefronts would pass 1 GiB (kHistoryLimitText).  The forward loop is
// AlignmentScore's with every step's visited diagonals kept: M after extend, I and D, as the reference's memory_high keeps them.
static inline int AlignmentString(const char *text, size_t n_, const char *pattern, size_t m_, const AlignmentParams &prm, std::string *out) {
    namespace af = exg::alignfn;
    out->clear();
    if (!af::params_ok(prm.mismatch, prm.gap_opening, prm.gap_extension)) return EXG_E_INVALID_ARG;
    if ((uint64_t)n_ + (uint64_t)m_ > af::kMaxPairBytes) return EXG_E_CAPACITY;
    const int32_t n = (int32_t)n_, m = (int32_t)m_;
    const int32_t x = prm.mismatch, o = prm.gap_opening, e = prm.gap_extension;
    const int32_t nd = n + m + 1;
    const int32_t bound = (int32_t)af::penalty_bound(o, e, n, m);
    struct Step {
        int32_t from, width;
        std::vector<int32_t> v;  // M | I | D, `width` entries each
    };
    struct History {
        std::vector<Step> steps;
        int32_t m;
        int32_t at(int32_t s, int32_t k, int32_t plane) const {
            if (s < 0) return af::kNone;
            const Step &st = steps[(size_t)s];
            const int32_t d = k + m - st.from;
            return d < 0 || d >= st.width ? af::kNone : st.v[(size_t)plane * st.width + d];
        }
    } hist;
    struct View {
        const History *h;
        int32_t m(int32_t s, int32_t k) const { return h->at(s, k, 0); }
        int32_t i(int32_t s, int32_t k) const { return h->at(s, k, 1); }
        int32_t d(int32_t s, int32_t k) const { return h->at(s, k, 2); }
    };
    hist.m = m;
    auto extend = [&](int32_t h, int32_t k) {
        int32_t v = h - k;
        while (h < n && v < m && text[h] == pattern[v]) h++, v++;
        return h;
    };
    const View w{&hist};
    uint64_t kept = 0;
    int32_t lo = m, hi = m, penalty = -1;
    for (int32_t s = 0; s <= bound && penalty < 0; s++) {
        const int32_t from = s ? (lo > 0 ? lo - 1 : 0) : m, to = s ? (hi < nd - 1 ? hi + 1 : nd - 1) : m;
        Step st;
        st.from = from, st.width = to - from + 1;
        kept += 12ull * st.width + sizeof(Step);
        if (kept > af::kHostHistoryBytes) return EXG_E_NOMEM;
        st.v.assign((size_t)3 * st.width, af::kNone);
        for (int32_t d = from; d <= to; d++) {
            const int32_t k = d - m;
            af::Cell c = af::cell(w.m(s - o - e, k - 1), w.i(s - e, k - 1), w.m(s - o - e, k + 1), w.d(s - e, k + 1), w.m(s - x, k), k, n, m);
            if (!s) c.m = 0;
            if (c.m >= 0) {
                c.m = extend(c.m, k);
                lo = d < lo ? d : lo, hi = d > hi ? d : hi;
            }
            st.v[(size_t)(d - from)] = c.m, st.v[(size_t)st.width + (d - from)] = c.i, st.v[(size_t)2 * st.width + (d - from)] = c.d;
        }
        hist.steps.push_back(std::move(st));
        if (w.m(s, n - m) >= n) penalty = s;
    }
    if (penalty < 0) return EXG_E_INVALID_ARG;  // (unreachable: the bound is an alignment's penalty)
    std::vector<uint8_t> buf(2 * ((size_t)n + m) + 16);
    af::RunWriter rw{buf.data() + buf.size(), buf.data(), 0, 0, false};
    if (!af::backtrace(w, penalty, x, o, e, n, m, &rw)) return EXG_E_INVALID_ARG;  // (unreachable: the history is the forward pass's)
    const uint8_t *begin = rw.finish();
    out->assign(reinterpret_cast<const char *>(begin), (size_t)(buf.data() + buf.size() - begin));
    return EXG_OK;
}

// parse_cigar / extract_from_cigar (exon/src/exon/sam_functions/module.cpp:32-131, rust/src/sam_functions.rs:114-200): the
// per-row arithmetic of the SQL scalars the shim registers, on the rules of exg_cigarfn.hpp (exg_cigar_op is the same on scan
// columns that are still in HBM).  A status instead of an exception, like SequenceMap.
struct CigarStatus {
    uint32_t code = EXG_PE_NONE;  // EXG_PE_CIGAR_*
    uint64_t offset = 0;          // EXG_PE_CIGAR_INVALID: where a left-to-right parser stops
};
struct CigarOp {
    char op;
    int32_t len;
};
// the operations of s[0, n) into *out (emptied first); the empty string and `*` have none
static inline CigarStatus ParseCigar(const char *s, size_t n, std::vector<CigarOp> *out) {
    namespace cf = exg::cigarfn;
    const uint8_t *u = reinterpret_cast<const uint8_t *>(s);
    CigarStatus st;
    out->clear();
    if (cf::is_absent(u, n)) return st;
    for (uint64_t i = 0; i < n;) {
        const cf::Step step = cf::next_op(u, n, i);
        if (!step.ok) {
            st.code = EXG_PE_CIGAR_INVALID, st.offset = step.next;
            return st;
        }
        out->push_back(CigarOp{(char)step.op, (int32_t)step.len});
        i = step.next;
    }
    return st;
}
// the slice of the sequence is its bytes [*start, *end)
static inline CigarStatus ExtractFromCigar(size_t sequence_length, const char *cigar, size_t n, int32_t *start, int32_t *end) {
    namespace cf = exg::cigarfn;
    const uint8_t *u = reinterpret_cast<const uint8_t *>(cigar);
    CigarStatus st;
    const bool absent = cf::is_absent(u, n);
    cf::Step first{0, 0, 0, true}, last{0, 0, 0, true};
    for (uint64_t i = 0; !absent && i < n;) {  // the whole CIGAR is validated
        last = cf::next_op(u, n, i);
        if (!last.ok) {
            st.code = EXG_PE_CIGAR_INVALID, st.offset = last.next;
            return st;
        }
        if (i == 0) first = last;
        i = last.next;
    }
    if (!cf::extract_range(absent, first.op, first.len, last.op, last.len, sequence_length, start, end)) st.code = EXG_PE_CIGAR_RANGE;
    return st;
}
// the exception texts of the two SQL scalars: parse_cigar names the string (test_scalar_functions.test:97), extract_from_cigar
// does not
static inline std::string ParseCigarErrorText(const char *s, size_t n) { return std::string(exg::cigarfn::kInvalidText) + ": " + std::string(s, n); }
static inline std::string ExtractFromCigarErrorText(const CigarStatus &st) {
    return st.code == EXG_PE_CIGAR_RANGE ? exg::cigarfn::kRangeText : exg::cigarfn::kInvalidText;
}

// gff_parse_attributes (exon/src/exon/gff_functions/module.cpp:29-84): the per-row work of the SQL scalar the shim registers, on
// the rules of exg_gffattr.hpp (exg_gff_attributes is the same on a column that is still in HBM).  Keys and values are slices
// of the field: offsets and lengths.  A status instead of an exception, like ParseCigar.
struct GffAttribute {
    uint64_t key_start, key_len, value_start, value_len;
};
struct GffAttributeStatus {
    uint32_t code = EXG_PE_NONE;  // EXG_PE_GFF_ATTRIBUTES (EXG_PE_FIELD_TOO_LONG: a field of 2^32 - 1 bytes and more)
    uint64_t offset = 0;          // of the failing segment behind its trim (exg_gffattr.hpp, R6)
    uint64_t length = 0;          // its length behind the trim
};
// the entries of s[0, n) into *out (emptied first), in field order
static inline GffAttributeStatus GffParseAttributes(const char *s, size_t n, std::vector<GffAttribute> *out) {
    namespace ga = exg::gffattr;
    GffAttributeStatus st;
    out->clear();
    if (n >= 0xFFFFFFFFull) {
        st.code = EXG_PE_FIELD_TOO_LONG;
        return st;
    }
    const ga::Verdict v = ga::parse_field(reinterpret_cast<const uint8_t *>(s), (uint32_t)n, [out](uint32_t k, uint32_t kn, uint32_t val, uint32_t vn) {
        out->push_back(GffAttribute{k, kn, val, vn});
    });
    if (v.kind == ga::kError) st.code = EXG_PE_GFF_ATTRIBUTES, st.offset = v.a, st.length = v.b;
    return st;
}
// the exception's text: the reference's (module.cpp:61), around the segment behind its trim
static inline std::string GffAttributeErrorText(const char *s, const GffAttributeStatus &st) {
    if (st.code != EXG_PE_GFF_ATTRIBUTES) return "gff_parse_attributes: the field is longer than 2^32 - 2 bytes";
    return std::string(exg::gffattr::kInvalidHead) + std::string(s + st.offset, (size_t)st.length) + exg::gffattr::kInvalidTail;
}

// exon/src/exon_extension.cpp:47-58: the registrations of the path (+ the read_vcf alias the north star names)
struct Registration {
    const char *name, *file_type;
};
static const Registration kRegistrations[] = {
    {"read_fasta", "fasta"}, {"read_fastq", "fastq"}, {"read_vcf_file_records", "vcf"}, {"read_vcf", "vcf"},
    {"read_bam_file_records", "bam"}, {"read_bed_file", "bed"}, {"read_sam_file_records", "sam"},
    {"read_bcf_file_records", "bcf"}, {"read_gtf", "gtf"}};
// exon/src/exon_extension.cpp:75-77: the indexed region queries, (VARCHAR path, VARCHAR region); bcf_query and bam_query are not built
static const Registration kRegionRegistrations[] = {{"vcf_query", "vcf"}};

}  // namespace exon_scan
