// exg_vcf_nested_build.cpp — the nested VCF columns of a scanned device batch (id / alt / filter LIST(VARCHAR), info STRUCT,
// formats LIST(STRUCT); kernels: exg_vcf_nested.hip).  build_nested runs them for both boundaries, in named stages over the
// state of one batch (NestedBuild); the host decisions it takes are exg_nested_layout.hpp's.  nested_prepare / nested_schema /
// nested_emit are the chunk boundary (exg_next_chunk, `read_vcf` in DuckDB): the columns' exg_type trees and their NVec nodes.
#include <time.h>

#include "exg_emit.hpp"

namespace exg_rd {

int upload_keys(exg_reader *r, const std::vector<KeyDef> &defs, StreamState::NestedKeys *nk) {
    KeyTable t;
    if (!build_key_table(defs, &t)) return fail(r, EXG_E_UNSUPPORTED, "a VCF header key of more than 65 535 bytes");
    EM_HIP(hipMalloc(&nk->d_keys, t.keys.size() * sizeof(vn::Key) + 16));
    EM_HIP(hipMalloc(&nk->d_slots, t.slots.size() * 4));
    EM_HIP(hipMalloc(&nk->d_names, t.names.size() + 16));
    if (!t.keys.empty()) EM_HIP(hipMemcpy(nk->d_keys, t.keys.data(), t.keys.size() * sizeof(vn::Key), hipMemcpyHostToDevice));
    EM_HIP(hipMemcpy(nk->d_slots, t.slots.data(), t.slots.size() * 4, hipMemcpyHostToDevice));
    if (!t.names.empty()) EM_HIP(hipMemcpy(nk->d_names, t.names.data(), t.names.size(), hipMemcpyHostToDevice));
    nk->tab.keys = (const vn::Key *)nk->d_keys;
    nk->tab.slots = (const uint32_t *)nk->d_slots;
    nk->tab.names = (const uint8_t *)nk->d_names;
    nk->tab.n_keys = (uint32_t)t.keys.size();
    nk->tab.slot_mask = (uint32_t)t.slots.size() - 1;
    nk->tab.names_bytes = (uint32_t)t.names.size();
    nk->tab.n_lists = t.n_lists;
    return EXG_OK;
}

namespace {

struct NestedBuild {  // one batch: what the stages share
    Emit &em;
    const ScanCtx &ctx;
    const uint64_t B;
    const bool *want, mirror;
    NestedOut *o;
    exg_reader *r = em.r;
    StreamState *st = em.st;
    hipStream_t s = em.s;
    const uint64_t n = em.n, nc = (n + B - 1) / B;
    const std::vector<KeyDef> &ik = st->info_keys, &fk = st->format_keys;
    const vn::KeyTab &it = st->nk_info.tab, &ft = st->nk_format.tab;
    const uint32_t nil = it.n_lists, nfl = ft.n_lists;
    const uint64_t C = (uint64_t)vn::kColInfo0 + nil;
    const bool rows_info = vn::rows_take_info(it.n_keys);
    const uint8_t *d_base = (const uint8_t *)ctx.d_input;
    const uint64_t pb = (uint64_t)(uintptr_t)ctx.h;
    // rows a wavefront looks at per turn of the wave kernels: one for cohort lines, 64 where most lines are k_rows' own
    const uint64_t avg = ctx.res.n_records ? ctx.res.consumed_bytes / ctx.res.n_records : 64;
    const uint32_t rpg = avg >= 2048 ? 1u : avg >= 256 ? 8u : 64u;
    struct timespec ts0;
    double t_stage1 = 0, t_stage2 = 0, t_stage3 = 0;
    vn::Batch b;
    vn::Samples sm;
    vn::Ctl *d_ctl = nullptr;
    uint32_t *d_cnt = nullptr, *d_seen = nullptr;
    uint64_t *d_goff = nullptr, *d_tot = nullptr, *h_tot = nullptr, *h_ftot = nullptr, S = 0;
    bool small_rows = false;
    Layout L[5];
    // of one attempt of write_children
    size_t side_cap = 0;
    uint8_t *d_side = nullptr;
    char *h_side = nullptr;
    uint64_t *h_ctl = nullptr;
    uint32_t *d_any = nullptr, *h_any = nullptr;

    double since() const {
        struct timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return (ts.tv_sec - ts0.tv_sec) * 1e3 + (ts.tv_nsec - ts0.tv_nsec) * 1e-6;
    }
    int reset_ctl() {
        EM_HIP(hipMemsetAsync(d_ctl, 0xFF, 8, s));
        EM_HIP(hipMemsetAsync((char *)d_ctl + 8, 0, 16, s));
        return EXG_OK;
    }

    // ---- stage 1: elements per row of every list column over rows
    int count_rows() {
        clock_gettime(CLOCK_MONOTONIC, &ts0);
        o->n = n;
        o->n_chunks = nc;
        memset(&b, 0, sizeof b);
        const int src_col[5] = {2, 4, 6, 7, 8};
        for (int c = 0; c < 5; c++) b.col[c] = (const exg_string_t *)r->d_cols[src_col[c]];
        b.rest_valid = (const uint64_t *)r->d_col_valid[8];  // (formats: the lines that have a FORMAT field)
        b.row_map = em.d_row_map;
        b.d_base = d_base;
        b.payload_base = pb;
        b.n = n;
        d_ctl = (vn::Ctl *)em.dalloc(sizeof(vn::Ctl));
        d_cnt = (uint32_t *)em.dalloc(C * n * 4);
        d_goff = (uint64_t *)em.dalloc(C * (n + 1) * 8);
        uint64_t *d_tmp = (uint64_t *)em.dalloc(vn::scan_tmp_entries(C, n) * 8);
        d_tot = (uint64_t *)em.dalloc((C + nfl + 1) * 8);
        h_tot = (uint64_t *)em.halloc((C + nfl + 1) * 8 + 64);
        const size_t seen_bytes = vn::info_wide_seen_bytes(it, n, rpg);
        d_seen = seen_bytes ? (uint32_t *)em.dalloc(seen_bytes) : nullptr;
        if (em.rc) return em.rc;
        b.ctl = d_ctl;
        b.cnt = d_cnt;
        b.cnt_stride = n;
        b.goff = d_goff;
        b.goff_stride = n + 1;
        if (int rc = reset_ctl()) return rc;
        if (!rows_info && nil) EM_HIP(hipMemsetAsync(d_cnt + (uint64_t)vn::kColInfo0 * n, 0, (size_t)nil * n * 4, s));  // (k_info_wide writes the keys a row has)
        b.mid_rows = (unsigned long long *)(d_tot + C + nfl);
        EM_HIP(hipMemsetAsync(b.mid_rows, 0, 8, s));
        vn::rows_count(b, it, st->small_rows, s);
        vn::info_wide_count(b, it, rpg, d_seen, st->small_rows, s);
        vn::samples_count(b, rpg, s);
        vn::scan_counts(d_cnt, n, C, n, d_goff, n + 1, d_tot, d_tmp, s);
        EM_HIP(hipMemcpyAsync(h_tot, d_tot, (C + nfl + 1) * 8, hipMemcpyDeviceToHost, s));
        EM_HIP(hipStreamSynchronize(s));
        // the writing pass's row size: small when at most one INFO field in 64 would be pushed to the wave kernel by it
        small_rows = rows_info && h_tot[C + nfl] * 64 <= n;
        st->small_rows = small_rows;
        o->S = S = h_tot[vn::kColSamples];
        o->d_goff = d_goff;
        t_stage1 = since();
        return EXG_OK;
    }

    // ---- stage 2: elements per sample of the FORMAT keys that are lists
    int count_sample_lists() {
        memset(&sm, 0, sizeof sm);
        sm.S = S;
        h_ftot = h_tot + C;
        for (uint32_t k = 0; k < nfl; k++) h_ftot[k] = 0;
        if (S && nfl) {
            uint32_t *d_fcnt = (uint32_t *)em.dalloc((size_t)nfl * S * 4);
            uint64_t *d_fgoff = (uint64_t *)em.dalloc((size_t)nfl * (S + 1) * 8);
            uint64_t *d_tmp2 = (uint64_t *)em.dalloc(vn::scan_tmp_entries(nfl, S) * 8);
            uint32_t *d_srow = (uint32_t *)em.dalloc(S * 4);
            if (em.rc) return em.rc;
            EM_HIP(hipMemsetAsync(d_fcnt, 0, (size_t)nfl * S * 4, s));
            sm.cnt = d_fcnt;
            sm.cnt_stride = S;
            vn::samples_count_lists(b, sm, ft, rpg, s);
            vn::scan_counts(d_fcnt, S, nfl, S, d_fgoff, S + 1, d_tot + C, d_tmp2, s);
            EM_HIP(hipMemcpyAsync(h_ftot, d_tot + C, (size_t)nfl * 8, hipMemcpyDeviceToHost, s));
            EM_HIP(hipStreamSynchronize(s));
            sm.goff = d_fgoff;
            sm.goff_stride = S + 1;
            sm.srow = d_srow;
            o->d_fgoff = d_fgoff;
        }
        t_stage2 = since();
        return EXG_OK;
    }

    // ---- stage 3: the children.  First where they go in the five regions (the totals are known) ...
    void lay_out() {
        for (int c = 0; c < 3; c++) {
            o->l_total[c] = h_tot[c];
            L[c].add(1, &o->l_entries[c], n * 16);
            L[c].add(1, &o->l_bases[c], (nc + 1) * 8);
            L[c].add(1, &o->l_elems[c], h_tot[c] * 16 + 16);
        }
        // (k_rows stores every row's values and validity words of a header it takes; the wave kernels store what a row / sample has)
        lay_keys(L[3], ik, &o->info, n, nc, h_tot + vn::kColInfo0, rows_info ? 1 : 0);
        L[4].add(1, &o->f_entries, n * 16);
        L[4].add(1, &o->f_bases, (nc + 1) * 8);
        lay_keys(L[4], fk, &o->format, S, nc, h_ftot, 0);
    }
    void fill_ko(vn::KeyOut *ko, const std::vector<KeyDef> &defs, const std::vector<NKeyBuf> &bufs, char *base) const {
        for (size_t q = 0; q < defs.size(); q++) {
            const NKeyBuf &kb = bufs[q];
            ko[q].vals = defs[q].is_list ? nullptr : base + kb.vals;
            ko[q].valid = (uint64_t *)(base + kb.valid);
            ko[q].child_vals = defs[q].is_list ? base + kb.child_vals : nullptr;
            ko[q].child_valid = defs[q].is_list ? (uint32_t *)(base + kb.child_valid) : nullptr;
        }
    }
    // DuckDB's list_entry_t of every list column + where every DataChunk's children begin
    int write_entries(vn::EntryJob *h_jobs, vn::EntryJob *d_jobs) {
        uint32_t nj = 0;
        for (int c = 0; c < 3; c++) h_jobs[nj++] = vn::EntryJob{d_goff + (uint64_t)c * (n + 1), o->g[c].d + o->l_entries[c], (uint64_t *)(o->g[c].d + o->l_bases[c])};
        h_jobs[nj++] = vn::EntryJob{d_goff + (uint64_t)vn::kColSamples * (n + 1), o->g[4].d + o->f_entries, (uint64_t *)(o->g[4].d + o->f_bases)};
        for (size_t q = 0, li = 0; q < ik.size(); q++)
            if (ik[q].is_list) {
                h_jobs[nj++] = vn::EntryJob{d_goff + (vn::kColInfo0 + li) * (n + 1), o->g[3].d + o->info[q].entries, (uint64_t *)(o->g[3].d + o->info[q].bases)};
                li++;
            }
        const uint32_t nj_rows = nj;
        if (sm.goff)
            for (size_t q = 0, li = 0; q < fk.size(); q++)
                if (fk[q].is_list) {
                    h_jobs[nj++] = vn::EntryJob{sm.goff + li * (S + 1), o->g[4].d + o->format[q].entries, (uint64_t *)(o->g[4].d + o->format[q].bases)};
                    li++;
                }
        EM_HIP(hipMemcpyAsync(d_jobs, h_jobs, nj * sizeof(vn::EntryJob), hipMemcpyHostToDevice, s));
        vn::entries_rows(d_jobs, nj_rows, n, B, nc, s);
        if (nj > nj_rows) vn::entries_elems(d_jobs + nj_rows, nj - nj_rows, S, sm.srow, d_goff + (uint64_t)vn::kColSamples * (n + 1), n, B, nc, s);
        return EXG_OK;
    }
    // ... then one attempt at writing them: the regions, the side buffer of st->side_cap bytes, the kernels, and what they report
    // (h_ctl: the first error, whether the side buffer overflowed, the bytes it was asked for)
    int write_children() {
        for (int c = 0; c < 5; c++) {
            NGroup &g = o->g[c];
            g.bytes = L[c].finish();
            g.d = (char *)em.dalloc(g.bytes + 64);
            g.h = mirror && want[c] ? (char *)em.halloc(g.bytes + 64) : nullptr;
            if (em.rc) return em.rc;
            if (L[c].end[0]) EM_HIP(hipMemsetAsync(g.d, 0, L[c].end[0], s));
            if (L[c].end[2] > L[c].end[1]) EM_HIP(hipMemsetAsync(g.d + L[c].end[1], 0xFF, L[c].end[2] - L[c].end[1], s));
        }
        side_cap = st->side_cap;
        d_side = (uint8_t *)em.dalloc(side_cap + 16);
        h_side = mirror ? (char *)em.halloc(side_cap + 16) : nullptr;
        vn::KeyOut *h_ko = (vn::KeyOut *)em.halloc((ik.size() + fk.size() + 1) * sizeof(vn::KeyOut));
        vn::KeyOut *d_ko = (vn::KeyOut *)em.dalloc((ik.size() + fk.size() + 1) * sizeof(vn::KeyOut));
        const size_t n_jobs_max = 4 + nil + nfl;
        vn::EntryJob *h_jobs = (vn::EntryJob *)em.halloc(n_jobs_max * sizeof(vn::EntryJob));
        vn::EntryJob *d_jobs = (vn::EntryJob *)em.dalloc(n_jobs_max * sizeof(vn::EntryJob));
        h_ctl = (uint64_t *)em.halloc(64);
        d_any = (uint32_t *)em.dalloc(ik.size() * 4 + 16);
        h_any = (uint32_t *)em.halloc(ik.size() * 4 + 16);
        if (em.rc) return em.rc;
        EM_HIP(hipMemsetAsync(d_any, 0, ik.size() * 4 + 16, s));
        b.key_any = mirror ? d_any : nullptr;
        fill_ko(h_ko, ik, o->info, o->g[3].d);
        fill_ko(h_ko + ik.size(), fk, o->format, o->g[4].d);
        EM_HIP(hipMemcpyAsync(d_ko, h_ko, (ik.size() + fk.size()) * sizeof(vn::KeyOut) + 1, hipMemcpyHostToDevice, s));
        for (int c = 0; c < 3; c++) b.elems[c] = (exg_string_t *)(o->g[c].d + o->l_elems[c]);
        b.d_side = d_side;
        b.side_cap = side_cap;
        // (Arrow: the decoded strings become Utf8 values through the text's own (device base, payload base) pair)
        b.side_payload_base = mirror ? (uint64_t)(uintptr_t)h_side : pb + (uint64_t)((const uint8_t *)d_side - d_base);
        vn::rows_write(b, it, d_ko, small_rows, s);
        vn::info_wide_write(b, it, d_ko, rpg, d_seen, small_rows, s);
        vn::samples_write(b, sm, ft, d_ko + ik.size(), rpg, s);
        vn::fix_slow_floats(d_ctl, s);
        if (int rc = write_entries(h_jobs, d_jobs)) return rc;
        EM_HIP(hipMemcpyAsync(h_ctl, d_ctl, 24, hipMemcpyDeviceToHost, s));
        if (mirror && !ik.empty()) EM_HIP(hipMemcpyAsync(h_any, d_any, ik.size() * 4, hipMemcpyDeviceToHost, s));
        EM_HIP(hipStreamSynchronize(s));
        return EXG_OK;
    }
    bool side_overflow() const { return (h_ctl[1] >> 32) != 0; }
    int grow_side() {  // (then everything is made again)
        st->side_cap = (size_t)(h_ctl[2] + h_ctl[2] / 4 + 4096);
        return reset_ctl();
    }
    void report() {
        o->err = h_ctl[0];
        t_stage3 = since();
        trace_at("N nested kernels done", n);
        r->nested_ns += (uint64_t)(t_stage3 * 1e6);
        if (!getenv("EXG_TRACE")) return;
        size_t bytes = 0;
        for (int c = 0; c < 5; c++) bytes += o->g[c].h ? o->g[c].bytes : 0;
        fprintf(stderr, "[exg]   nested: counts %.2f ms, sample lists %.2f ms, children %.2f ms (%llu rows, %llu samples, %.1f MiB to the host)\n", t_stage1,
                t_stage2 - t_stage1, t_stage3 - t_stage2, (unsigned long long)n, (unsigned long long)S, bytes / 1048576.0);
    }

    // ---- the chunk boundary: the regions it wants go to pinned memory
    int mirror_home() {
        // What is all zeros stays at home (round 6): a list column without a single element in the batch (`formats` of a file without
        // samples, `id` of a file of "."s), an INFO key that no row of the batch has — 16 bytes a row each that said nothing; their
        // NVec nodes point every chunk at one block of zeros instead (VCF-8: 32 of a line's 171 bytes)
        static const bool no_zero_skip = getenv("EXG_VCF_NO_ZERO_SKIP") != nullptr;
        std::vector<const size_t *> skip;
        if (!no_zero_skip) {
            void *hz = em.halloc(B * 16 + 64);
            if (em.rc) return em.rc;
            memset(hz, 0, B * 16 + 64);
            o->h_zero = hz;
            for (int c = 0; c < 3; c++) o->group_zero[c] = o->l_total[c] == 0;
            o->group_zero[4] = S == 0;
            skip = zero_skip(ik, &o->info, h_any);
        }
        const hipStream_t cs = em.d2h ? em.d2h : st->copy_stream;
        for (int c = 0; c < 5; c++) {
            if (!o->g[c].h || !o->g[c].bytes || o->group_zero[c]) continue;
            for (const auto &rg : L[c].ranges(skip)) {
                EM_HIP(hipMemcpyAsync(o->g[c].h + rg.first, o->g[c].d + rg.first, rg.second, hipMemcpyDeviceToHost, cs));
                r->host_vector_bytes += rg.second;
            }
        }
        const uint64_t side_used = h_ctl[2];
        if (side_used) EM_HIP(hipMemcpyAsync(h_side, d_side, (size_t)std::min<uint64_t>(side_used, side_cap), hipMemcpyDeviceToHost, cs));
        return EXG_OK;
    }
};

}  // namespace

int build_nested(Emit &em, const ScanCtx &ctx, uint64_t B, const bool *want, bool mirror, NestedOut *o) {
    NestedBuild nb{em, ctx, B, want, mirror, o};
    int rc;
    if ((rc = nb.count_rows()) || (rc = nb.count_sample_lists())) return rc;
    nb.lay_out();
    for (int turn = 0;; turn++) {
        if ((rc = nb.write_children())) return rc;
        // (a second turn: a batch with more percent-decoded bytes than the side buffer held)
        if (turn == 1 || !nb.side_overflow()) break;
        if ((rc = nb.grow_side())) return rc;
    }
    nb.report();
    return mirror ? nb.mirror_home() : EXG_OK;
}

// ---- the chunk boundary (exg_next_chunk): the columns' types, and the NVec nodes of a batch -----------------------------------
static exg_type *alloc_types(StreamState *st, size_t n) {
    st->type_nodes.emplace_back(new exg_type[n ? n : 1]());
    return st->type_nodes.back().get();
}
static exg_type leaf(int type, const char *name, int nullable) {
    exg_type t;
    memset(&t, 0, sizeof t);
    t.type = type, t.name = name, t.nullable = nullable;
    return t;
}
static exg_type list_of(StreamState *st, const char *name, const exg_type &item, int nullable) {
    exg_type t = leaf(EXG_TYPE_LIST, name, nullable);
    exg_type *c = alloc_types(st, 1);
    c[0] = item;
    t.n_children = 1;
    t.children = c;
    return t;
}
static exg_type key_type(StreamState *st, const KeyDef &k) {
    const int base = key_type_info(k.type).exg_type;
    if (!k.is_list) return leaf(base, k.id.c_str(), 1);
    return list_of(st, k.id.c_str(), leaf(base, "item", 1), 1);
}
static exg_type struct_of(StreamState *st, const char *name, const std::vector<KeyDef> &keys, int nullable) {
    exg_type t = leaf(EXG_TYPE_STRUCT, name, nullable);
    exg_type *c = alloc_types(st, keys.size());
    for (size_t k = 0; k < keys.size(); k++) c[k] = key_type(st, keys[k]);
    t.n_children = (int)keys.size();
    t.children = c;
    return t;
}

int nested_prepare(exg_reader *r) {
    if (r->nested_state || r->format != EXG_FMT_VCF) return EXG_OK;
    if (!r->file) {  // the schema is the first file's header (like register_exon_table, arrow_reader.rs:118-123)
        if (r->file_idx >= r->files.size()) return fail(r, EXG_E_IO, "no input file");
        int rc = open_next_file(r);
        if (rc) return rc;
    }
    auto st = std::make_shared<StreamState>();
    st->r = r;
    st->owns_reader = false;
    parse_vcf_header((const char *)r->file->p, (size_t)r->vcf_header_bytes, &st->info_keys, &st->format_keys);
    int rc;
    if ((rc = upload_keys(r, st->info_keys, &st->nk_info)) || (rc = upload_keys(r, st->format_keys, &st->nk_format))) return rc;
    // A wide header makes wide rows of vectors whatever the lines hold — every key is a child with a value slot per row (per sample)
    // and, on the device, a count and an offset per row for each list key: a 1 000-key header over 256 MiB of SHORT lines would ask
    // for tens of GB of both.  The device batch shrinks with the number of keys (64 keys: as before).
    {
        const uint64_t keys = st->info_keys.size() + st->format_keys.size();
        if (keys > 64) r->device_batch_bytes = std::max<uint64_t>(8ull << 20, (r->device_batch_bytes * 64 / keys) & ~0xFFFFFull);
    }
    // the flat columns as the table has them; the nested ones by hand, under the table's names
    const FormatDesc &f = format_desc(EXG_FMT_VCF);
    exg_type *t = st->type_roots;
    for (int c = 0; c < f.n_columns; c++)
        if (!f.col[c].nested) t[c] = *flat_tree(EXG_FMT_VCF, c);
    for (int c : {2, 4, 6}) t[c] = list_of(st.get(), f.col[c].name, leaf(EXG_TYPE_VARCHAR, "item", 1), 1);  // id, alt, filter
    t[7] = struct_of(st.get(), f.col[7].name, st->info_keys, 1);                                        // info
    t[8] = list_of(st.get(), f.col[8].name, struct_of(st.get(), "item", st->format_keys, 1), 1);        // formats
    r->nested_state = st;
    return EXG_OK;
}

void nested_schema(exg_reader *r, exg_schema *out) {
    StreamState *st = (StreamState *)r->nested_state.get();
    if (!st) return;
    for (int c = 0; c < 9; c++) {
        out->tree[c] = &st->type_roots[c];
        out->types[c] = st->type_roots[c].type;
        out->nullable[c] = st->type_roots[c].nullable;
    }
}

namespace {

// The NVec nodes over a batch's mirrored regions.  A node whose buffers stayed at home — NKeyBuf::zero, NestedOut::group_zero —
// points at the batch's block of zeros (hz; NULL: EXG_VCF_NO_ZERO_SKIP)
struct NVecs {
    const NestedOut &no;
    const char *hz;
    const uint64_t *zero_bases;  // all chunks' children begin at 0 when a list column has no element at all

    static NVec node(int type, uint32_t elem, uint64_t length, const void *data, const void *validity, bool zero) {
        NVec v;
        v.type = type;
        v.elem = elem;
        v.length = length;
        v.data = data;
        v.validity = (const uint64_t *)validity;
        v.zero = zero;
        return v;
    }
    // a LIST over m elements of the enclosing space: entries, chunk bases and one child
    NVec list(uint64_t m, bool z, const char *h, size_t entries, const void *valid, const uint64_t *bases, NVec child) const {
        NVec v = node(EXG_TYPE_LIST, 16, m, z ? hz : h + entries, valid, z);
        v.child_base = bases;
        v.children.push_back(std::move(child));
        return v;
    }
    NVec list_of_strings(int c) const {  // id / alt / filter (not percent-decoded)
        const char *h = no.g[c].h;
        const bool z = no.group_zero[c] && hz;
        return list(no.n, z, h, no.l_entries[c], nullptr, z ? zero_bases : (const uint64_t *)(h + no.l_bases[c]),
                    node(EXG_TYPE_VARCHAR, 16, no.l_total[c], z ? hz : h + no.l_elems[c], nullptr, z));
    }
    std::vector<NVec> key_vecs(const std::vector<KeyDef> &defs, const std::vector<NKeyBuf> &bufs, const char *h, uint64_t m, bool all_zero) const {
        std::vector<NVec> kids;
        for (size_t q = 0; q < defs.size(); q++) {
            const NKeyBuf &kb = bufs[q];
            const KeyTypeInfo &ti = key_type_info(defs[q].type);
            const bool z = (kb.zero || all_zero) && hz;
            if (!defs[q].is_list)
                kids.push_back(node(ti.exg_type, (uint32_t)ti.elem, m, z ? hz : h + kb.vals, z ? hz : h + kb.valid, z));
            else
                kids.push_back(list(m, z, h, kb.entries, z ? hz : h + kb.valid, all_zero ? zero_bases : (const uint64_t *)(h + kb.bases),
                                    node(ti.exg_type, (uint32_t)ti.elem, kb.total, z ? hz : h + kb.child_vals, z ? hz : h + kb.child_valid, z)));
        }
        return kids;
    }
};

}  // namespace

// Columns id, alt, filter, info, formats of one scanned batch -> b->nested (the flat columns are copied by next_batch).
// *n_rows: in = rows of the batch, out = rows to hand out (a typed value that does not parse ends the stream there).
int nested_emit(exg_reader *r, const ScanCtx &ctx, Batch *b, const uint32_t *d_row_map, uint64_t *n_rows) {
    StreamState *st = (StreamState *)r->nested_state.get();
    if (!st) return fail(r, EXG_E_INVALID_ARG, "nested_emit without nested_prepare");
    if (getenv("EXG_TRACE"))
        fprintf(stderr, "[exg] nested emit: the batch before used %zu KiB of a %zu KiB arena + %zu extra blocks (%zu KiB)\n", st->arena().used >> 10,
                st->arena().cap >> 10, st->arena().extra.size(), st->arena().extra_bytes >> 10);
    // (the other arena: the one of the batch before may still be read by its copies — whose end the consumer waits for before this
    // function is entered a second time after it)
    if (int rc = begin_batch(r, st, true)) return rc;
    StreamDrain drain(st->copy_stream);
    const uint64_t n = *n_rows;
    Emit em(r, st, &b->host, n, d_row_map);
    // (columns outside the projection are built like the others — a malformed value is an error whether or not its column is
    // selected, like in the reference — but their regions stay on the device)
    const int top[5] = {2, 4, 6, 7, 8};
    bool want[5];
    for (int c = 0; c < 5; c++) want[c] = r->want(top[c]);
    // Every byte that goes back to the host travels on ONE stream — behind the flat columns' copies when next_batch gave them a
    // stream of their own: a copy occupies an SDMA engine, a second stream of D2H copies takes a second engine, and that was the
    // one the next batch's upload runs on (EXG_TRACE=2: the upload landed 2 ms after the columns had left, the link never duplex)
    em.d2h = r->col_stream && !getenv("EXG_VCF_TWO_D2H") ? r->col_stream : st->copy_stream;
    StreamDrain drain2(em.d2h);  // (an error return: nothing may still be writing the batch's blocks)
    NestedOut no;
    if (int rc = build_nested(em, ctx, r->batch_rows, want, true, &no)) return rc;
    if (r->lazy_landing && em.d2h == r->col_stream)
        drain2.release();  // the caller records the batch's landing event behind these copies (Batch::landed)
    else
        EM_HIP(hipStreamSynchronize(em.d2h));
    b->nested.assign(9, NVec());
    NVecs nv{no, (const char *)no.h_zero, nullptr};
    if (nv.hz && (no.group_zero[0] || no.group_zero[1] || no.group_zero[2] || no.group_zero[4])) {
        void *zb = em.halloc((no.n_chunks + 1) * 8);
        if (em.rc) return em.rc;
        memset(zb, 0, (no.n_chunks + 1) * 8);
        nv.zero_bases = (const uint64_t *)zb;
    }
    for (int c = 0; c < 3; c++)
        if (want[c]) b->nested[(size_t)top[c]] = nv.list_of_strings(c);
    if (want[3]) {
        NVec info = NVecs::node(EXG_TYPE_STRUCT, 0, n, nullptr, nullptr, false);
        info.children = nv.key_vecs(st->info_keys, no.info, no.g[3].h, n, false);
        b->nested[7] = std::move(info);
    }
    if (want[4]) {
        const char *h = no.g[4].h;
        const bool z = no.group_zero[4] && nv.hz;  // (no line of the batch has a sample: every entry {0, 0}, every child empty)
        NVec item = NVecs::node(EXG_TYPE_STRUCT, 0, no.S, nullptr, nullptr, false);
        item.children = nv.key_vecs(st->format_keys, no.format, h, no.S, z);
        b->nested[8] = nv.list(n, z, h, no.f_entries, nullptr, z ? nv.zero_bases : (const uint64_t *)(h + no.f_bases), std::move(item));
    }
    stop_at_value_error(r, no.err, n_rows);
    return EXG_OK;
}

}  // namespace exg_rd
