// exg_emit.hpp — internal: what the two emitters of a scanned device batch share.  exg_arrow_stream.cpp turns the batch into
// Arrow buffers (new_reader), exg_vcf_nested_build.cpp builds the nested VCF columns for both boundaries and hands them out at
// the chunk boundary (nested_emit).  Here: the device arena they allocate from, the state that lives as long as the stream, the
// allocation front of one batch (Emit), the builder's result (NestedOut), and how a batch begins and ends at either boundary.
#pragma once
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "exg_arrow.hpp"
#include "exg_arrow_export.hpp"
#include "exg_nested_layout.hpp"
#include "exg_rd_fanout.hpp"
#include "exg_rd_source.hpp"
#include "exg_vcf_nested.hpp"

namespace exg_rd {
namespace ea = exg::arrow;

// ---- memory ------------------------------------------------------------------------------------------------------------------
struct DevArena {  // bump allocator, reset per batch; what does not fit comes from the device pool, and the next batch's
                   // arena is as large as this batch turned out to need (hipMalloc / hipFree per batch cost milliseconds)
    char *base = nullptr;
    size_t cap = 0, used = 0, extra_bytes = 0, need = 0, min_extra = 1u << 20;
    std::vector<std::pair<void *, size_t>> extra;
    int dev = 0;
    void *alloc(size_t n) {
        n = (n + 255) & ~(size_t)255;
        if (n == 0) n = 256;
        if (used + n <= cap) {
            void *p = base + used;
            used += n;
            return p;
        }
        const size_t sz = n < min_extra ? min_extra : n;  // (1 MiB: small blocks would come one by one; 64 KiB under a memory budget)
        void *p = dev_pool()->take(dev, sz);
        if (!p) return nullptr;
        extra.emplace_back(p, sz);
        extra_bytes += sz;
        return p;
    }
    bool owns(const void *p) const {  // (a block of this arena: what stays put until its reset)
        const char *q = (const char *)p;
        if (base && q >= base && q < base + cap) return true;
        for (const auto &e : extra)
            if (q >= (const char *)e.first && q < (const char *)e.first + e.second) return true;
        return false;
    }
    void reset() {
        need = used + extra_bytes;
        for (auto &e : extra) dev_pool()->give(dev, e.first, e.second);
        extra.clear();
        used = 0;
        extra_bytes = 0;
    }
    // before a batch: an arena of `want` bytes, or — when the batch before overflowed it — of what that one needed + 25 %
    void prepare(int device, size_t want) {
        dev = device;
        if (base && need > cap) {
            dev_pool()->give(dev, base, cap);
            base = nullptr, cap = 0;
            want = std::max(want, need + need / 4);
        }
        if (!base) {
            want = (want + 4095) & ~(size_t)4095;
            if ((base = (char *)dev_pool()->take(dev, want))) cap = want;
        }
    }
    ~DevArena() {
        reset();
        if (base) dev_pool()->give(dev, base, cap);
    }
};

struct ABatch {
    HostArena host;
    AColumn root;  // a kStruct over the rows: its children are the batch's columns
    uint64_t n_rows = 0;
    // round 6: the batch is handed on while its buffers still travel (an event behind the last copy): whoever hands out its first
    // record batch waits for it — after the batch BEHIND it has begun to be made, whose kernels then run beside these copies
    hipEvent_t landed = nullptr;
    void wait_landed() {
        if (!landed) return;
        (void)hipEventSynchronize(landed);
        (void)hipEventDestroy(landed);
        landed = nullptr;
    }
    ABatch() { root.kind = AColumn::kStruct; }
    ~ABatch() { wait_landed(); }  // (before `host` gives its pinned blocks back)
};

struct StreamState {
    exg_reader *r = nullptr;
    std::vector<Field> schema;
    std::vector<KeyDef> info_keys, format_keys;
    bool has_filter = false;
    ea::FilterProgram prog;
    std::string consts;
    void *d_consts = nullptr, *d_prog = nullptr;
    // the header's keys on the device (exg_vcf_nested.hpp): any number of them, looked up by a hash of their text
    struct NestedKeys {
        vn::KeyTab tab;
        void *d_keys = nullptr, *d_slots = nullptr, *d_names = nullptr;
        NestedKeys() { memset(&tab, 0, sizeof tab); }
    } nk_info, nk_format;
    size_t side_cap = 64u << 10;  // bytes of percent-decoded String values a batch may hold (grows when a batch needs more)
    bool small_rows = false;      // k_rows' row size: the batch before had (nearly) no INFO field of 65 - 128 bytes (exg_vcf_nested.hip)
    // two arenas, taken in turn: a batch's regions are still being copied back while the batch behind it is built (Batch::landed)
    DevArena arena_a, arena_b;
    DevArena *arena_p = &arena_a;
    DevArena &arena() { return *arena_p; }
    int arena_idx() const { return arena_p == &arena_a ? 0 : 1; }
    hipEvent_t arena_done[2] = {nullptr, nullptr};  // (Arrow mode) behind the last copy out of arena_a / arena_b; arena_busy: recorded, not yet waited for
    bool arena_busy[2] = {false, false};
    std::shared_ptr<ABatch> batch;
    uint64_t batch_row = 0;
    // the device batch AFTER the one being handed out is produced on a thread of its own (scan, Arrow buffers, their way
    // back over PCIe: ~6 ms per 256 MiB) while the consumer walks the ~400 record batches of the current one
    std::shared_ptr<ABatch> produced;  // written by arrow_emit
    std::thread producer;
    int produced_state = 0;            // 1 a batch, 2 end of stream, 3 error (last_error)
    std::string last_error;
    size_t host_hint = 0;  // pinned bytes the previous batch needed
    hipStream_t copy_stream = nullptr;
    int copy_dev = 0;
    hipEvent_t copy_ev = nullptr;
    std::unique_ptr<FanOut> fan;  // several devices: the batches come from the stripes' streams (exg_rd_fanout.hpp)
    bool owns_reader = true;  // new_reader: the stream owns its reader; chunk mode: the reader owns this state
    // chunk mode: the columns' exg_type trees (node arrays and names live here)
    std::vector<std::unique_ptr<exg_type[]>> type_nodes;
    exg_type type_roots[16];
    ~StreamState() {
        fan.reset();  // (the workers' streams end first)
        if (copy_ev) (void)hipEventDestroy(copy_ev);
        if (copy_stream) stream_pool()->give_d2h(copy_dev, copy_stream);  // (synchronises it: nothing reads the arenas any more)
        for (hipEvent_t e : arena_done)
            if (e) (void)hipEventDestroy(e);
        for (void *p : {d_consts, d_prog, nk_info.d_keys, nk_info.d_slots, nk_info.d_names, nk_format.d_keys, nk_format.d_slots, nk_format.d_names})
            if (p) (void)hipFree(p);
        arena_a.reset();
        arena_b.reset();
        if (owns_reader) delete r;
    }
};

#define EM_HIP(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess) return fail(r, EXG_E_HIP, std::string(#expr " failed: ") + hipGetErrorString(_e)); \
    } while (0)

// ---- the allocation front of one batch; the Arrow conversions over it are exg_arrow_stream.cpp's --------------------------------
struct Emit {
    exg_reader *r;
    StreamState *st;
    HostArena *host;  // pinned memory of the batch being built
    hipStream_t s;
    uint64_t n;                 // output rows
    const uint32_t *d_row_map;  // NULL: identity
    int rc = 0;
    hipStream_t d2h = nullptr;  // the stream build_nested's mirrors travel on (NULL: st->copy_stream)
    bool lazy = false;  // arrow_emit: the copies are not waited for here (ABatch::landed) — a source outside the arena is staged in it first

    Emit(exg_reader *r_, StreamState *st_, HostArena *host_, uint64_t n_, const uint32_t *d_row_map_)
        : r(r_), st(st_), host(host_), s(r_->stream), n(n_), d_row_map(d_row_map_) {}
    void *dalloc(size_t bytes) {
        void *p = st->arena().alloc(bytes);
        if (!p && !rc) rc = fail(r, EXG_E_HIP, "out of device memory in the Arrow emitter");
        return p;
    }
    void *halloc(size_t bytes) {
        void *p = host->alloc(bytes);
        if (!p && !rc) rc = fail(r, EXG_E_HIP, "out of pinned host memory in the Arrow emitter");
        return p;
    }
    // exg_arrow_stream.cpp
    uint64_t fetch_u64(const uint64_t *d);
    const uint8_t *to_host(const void *d, size_t bytes);
    const uint8_t *row_validity(const uint64_t *d_src);
    const uint8_t *off32_of(const uint64_t *d_goff, uint64_t m);
    bool too_long(uint64_t total);
    uint8_t *utf8_values(const ea::StrCol &c, const uint32_t *d_map, uint64_t m, uint64_t limit, uint64_t **d_goff, uint64_t *total);
    AColumn utf8_top(const ea::StrCol &c, const uint64_t *d_valid_src);
    AColumn utf8_abs(const exg_string_t *d_col, const uint8_t *d_base, uint64_t payload_base, uint64_t m, const uint8_t *h_validity);
    AColumn prim(const void *d_src, int es, const uint64_t *d_valid_src);
};

// ---- the nested VCF columns of one device batch (exg_vcf_nested.hpp), for both boundaries ------------------------------------
// Everything is made in DuckDB's layouts — list_entry_t + child vectors, string_t, a byte per BOOLEAN, validity bits — one
// device region per top-level column (id, alt, filter, info, formats), mirrored to pinned memory by one copy when the chunk
// boundary wants the column; the Arrow boundary converts what differs (int32 offsets, Utf8 values, Boolean bits) on the device.
struct NGroup {
    char *d = nullptr, *h = nullptr;
    size_t bytes = 0;
};
struct NestedOut {
    uint64_t n = 0, S = 0, n_chunks = 0;
    NGroup g[5];  // id, alt, filter, info, formats
    size_t l_entries[3] = {0, 0, 0}, l_bases[3] = {0, 0, 0}, l_elems[3] = {0, 0, 0};
    uint64_t l_total[3] = {0, 0, 0};
    size_t f_entries = 0, f_bases = 0;
    std::vector<NKeyBuf> info, format;
    const uint64_t *d_goff = nullptr;  // list columns over rows (vn::kCol*), n + 1 offsets each
    const uint64_t *d_fgoff = nullptr;  // FORMAT list keys over samples, S + 1 offsets each
    uint64_t err = ~0ull;  // (row << 8) | code of the first typed value that does not parse
    bool group_zero[5] = {false, false, false, false, false};  // id / alt / filter: no element at all; formats: no sample at all
    const void *h_zero = nullptr;  // the batch's block of zeros (B x 16 bytes): what NVec::zero nodes point at
};
// exg_vcf_nested_build.cpp.  want[c]: the chunk boundary hands column c out (its region is mirrored to pinned memory);
// mirror == false: the Arrow boundary (nothing is copied here).  em.n rows (through em.d_row_map), B rows per DataChunk.
int build_nested(Emit &em, const ScanCtx &ctx, uint64_t B, const bool *want, bool mirror, NestedOut *o);
int upload_keys(exg_reader *r, const std::vector<KeyDef> &defs, StreamState::NestedKeys *nk);

// ---- how a batch begins and ends at either boundary -----------------------------------------------------------------------
// Before the first allocation of a batch.  other_arena: the arena the batch before did not use — its copies may still read
// that one's (the Arrow boundary's lazy landing waits here for the last copy out of the arena it takes, arena_done; the chunk
// boundary's consumer has waited before this is entered again).  Then the arena is reset and sized, and the D2H stream and its
// event are taken on first use.
inline int begin_batch(exg_reader *r, StreamState *st, bool other_arena) {
    if (other_arena) {
        st->arena_p = st->arena_p == &st->arena_a ? &st->arena_b : &st->arena_a;
        const int idx = st->arena_idx();
        if (st->arena_busy[idx]) {
            EM_HIP(hipEventSynchronize(st->arena_done[idx]));
            st->arena_busy[idx] = false;
        }
    }
    st->arena().reset();
    // sized for the typical batch: offsets + values + views of every column; what a batch needs beyond that comes from the
    // pool and enlarges the arena of the next one
    st->arena().min_extra = r->mem_cap ? (64u << 10) : (1u << 20);
    st->arena().prepare(r->device, (size_t)std::min<uint64_t>(r->mem_cap ? r->d_in_cap * 6 + (1u << 20) : r->d_in_cap * 3 + (64u << 20), 6ull << 30));
    if (!st->copy_stream) {
        EM_HIP(stream_pool()->take_d2h(r->device, &st->copy_stream, /*calibrate=*/r->file && r->file->n >= (512ull << 20) && !r->mem_cap));
        st->copy_dev = r->device;
        EM_HIP(hipEventCreateWithFlags(&st->copy_ev, hipEventDisableTiming));
    }
    return EXG_OK;
}
struct StreamDrain {  // whatever way a function is left, no copy may still be writing into the batch's blocks
    hipStream_t cs;
    explicit StreamDrain(hipStream_t s) : cs(s) {}
    StreamDrain(const StreamDrain &) = delete;
    void release() { cs = nullptr; }  // (the batch carries a landing event behind these copies)
    ~StreamDrain() {
        if (cs) (void)hipStreamSynchronize(cs);
    }
};
// a typed value did not parse (err: NestedOut::err): the rows in front of it are handed out, then the error (like the scan's own errors)
inline void stop_at_value_error(exg_reader *r, uint64_t err, uint64_t *n_rows) {
    if (err == ~0ull) return;
    *n_rows = err >> 8;
    if (!r->pending_error) {
        r->pending_error = (uint32_t)(err & 0xFF);
        r->pending_error_offset = 0;
    }
}

}  // namespace exg_rd
