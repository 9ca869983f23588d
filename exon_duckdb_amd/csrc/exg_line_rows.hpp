// exg_line_rows.hpp — the driver of the "one row per text line, strings are slices of the input" scans (BED, SAM): all that
// such a format needs around its row function.  Two implementations behind line_rows_scan<R>, one row function (R::line<Src>):
//   * fused (exg_fused_core.hpp skeleton, the any-shape instance only): thread = line, fields cut out of LDS; a half with more
//     lines than its list holds is emitted in passes; the one line per half that begins in front of the 1 KiB window is left
//     to k_line_far behind the kernel (FarRec);
//   * general: line index (exg_lines.hip) + thread = line reading global memory — the differential partner.
// A format R supplies
//   kName, kLabel                         "exg_bed_scan", "BED": for the error messages
//   kColumns                              columns of a row (d_columns / d_validity of its scan args)
//   kValidBits, valid_col(bit)            RowInfo::valid bit b says column valid_col(b) is not NULL (ascending in b)
//   kKeepBit                              -1, or the valid bit that says "this line is a row": a line without it (and without an
//                                         error) keeps its row number, leaves its slot unwritten and raises EXG_RF_ROWS_SKIPPED
//   kGeneralBytesPerLine                  what sizes the general path's grid
//   kNlCap, kHalvesFull, kWavesFull       the fused scan's line list, halves per workgroup and waves per SIMD
//   line<Src>(src, s, e, dev, out, store) the row function: one line [s, e) (CR already stripped) to row `out`
// The small pieces — row_report, half_qend, mark_far_line, head_unresolved, global_line — are the VCF scan's too (exg_vcf.hip).
#pragma once
#include "exg_fused_core.hpp"
#include "exg_line_src.hpp"
#include "exg_lines.hpp"

namespace exg {

template <int N>
struct LineRowsDev {
    const uint8_t *d_in;
    uint64_t n_bytes;
    uint64_t lead;
    uint64_t first_line_index;  // unused (kept for the core's EOF arithmetic): 0
    uint64_t payload_base;
    uint32_t flags;
    uint32_t pad;
    void *d_col[N];        // exg_string_t[] / the format's integers; NULL: validated only
    uint64_t *d_valid[N];  // the columns R::valid_col names
    uint64_t capacity;
};

struct RowInfo {
    uint32_t code;
    uint32_t valid;  // bit b: column R::valid_col(b) is not NULL
};

__device__ __forceinline__ void put_str(void *col, unsigned long long out, uint4 v) {
    if (col) st_stream16(reinterpret_cast<uint4 *>(col) + out, v);
}
__device__ __forceinline__ void put_i32(void *col, unsigned long long out, int v) {
    if (col) __builtin_nontemporal_store(v, reinterpret_cast<int *>(col) + out);
}
__device__ __forceinline__ void put_i64(void *col, unsigned long long out, long long v) {
    if (col) __builtin_nontemporal_store(v, reinterpret_cast<long long *>(col) + out);
}

__device__ __forceinline__ void row_report(ScanWsHeader *hdr, uint32_t code, unsigned long long out, uint64_t line_off) {
    atomicMin(&hdr->err_word, (out << 8) | (code & 0x7Fu));
    atomicMin(&hdr->err_off, (unsigned long long)line_off);
}
// a line that is no row (R::kKeepBit: GTF's `#` lines)
template <class R>
__device__ __forceinline__ void note_skipped(ScanWsHeader *hdr, const RowInfo &r) {
    if constexpr (R::kKeepBit >= 0)
        if (!r.code && !((r.valid >> R::kKeepBit) & 1u)) atomicOr(&hdr->flags, EXG_RF_ROWS_SKIPPED);
}
// the validity words of 64 consecutive rows from out_base on: a ballot per bit
template <class R>
__device__ __forceinline__ void store_row_validity(const LineRowsDev<R::kColumns> &a, uint32_t valid, long long out_base, uint32_t lane) {
#pragma unroll
    for (int b = 0; b < R::kValidBits; b++) store_validity64(a.d_valid[R::valid_col(b)], __ballot((valid >> b) & 1u), out_base, lane);
}

// ---- pieces of an emit_half (any-shape scan) ---------------------------------------------------------------------------
// tile_qend[half] = the offset just past the last line that ends in this half (0: none), stored by the pass's `first` thread,
// which gets the word back (the others: 0)
template <class L>
__device__ __forceinline__ unsigned long long half_qend(const L &s, const TileCtx &c, uint64_t n_bytes, bool first,
                                                        unsigned long long *__restrict__ tile_qend, uint64_t tile_index) {
    unsigned long long qend_word = 0;
    if (first && (c.pass_base == 0 || c.n_lines)) {
        long long e = 0;
        if (c.n_lines) {
            e = (long long)c.tile_off + (int)s.nlist[4 + c.n_lines - 1] - kWin + 1;
            if ((unsigned long long)e > n_bytes) e = (long long)n_bytes;
        }
        if (c.pass_base) e |= (long long)(tile_qend[tile_index] & kFarBit);  // (a later pass keeps the first pass's mark)
        qend_word = (unsigned long long)e;
        tile_qend[tile_index] = qend_word;
    }
    return qend_word;
}
// The line that ends at e1 begins in front of the LDS window (only the first line of a half's first pass can: the thread that
// stored qend_word): its row is the far kernel's
template <class L>
__device__ __forceinline__ void mark_far_line(const L &s, const TileCtx &c, uint64_t n_bytes, int e1, long long out, unsigned long long qend_word,
                                              ScanWsHeader *hdr, unsigned long long *__restrict__ tile_qend, uint64_t tile_index) {
    FarRec f;
    f.pos[0] = s.prev32[3];
    f.pos[1] = c.half * kTile + e1 - kWin;
    f.pos[2] = f.pos[3] = f.pos[4] = 0;
    f.flags = c.is_eof_tile ? 1u : 0u;
    f.out = out;
    far_rec_of<false>(tile_qend, n_bytes)[tile_index] = f;
    hdr->any_far = 1u;
    tile_qend[tile_index] = qend_word | kFarBit;  // (this thread stored the word above: no load — a load behind the store cost a
                                                  // memory round trip per half of a cohort VCF)
}

// ---- a line in global memory (general path, far kernels) ----------------------------------------------------------------
// The head of a line is not in the buffer (it is the buffer's first and EXG_F_BOF is not set): no row, counted — the caller
// widens the halo
__device__ __forceinline__ void head_unresolved(ScanWsHeader *hdr) {
    atomicAdd(&hdr->n_unresolved, 1ull);
    atomicOr(&hdr->flags, EXG_RF_HEAD_UNRESOLVED);
}
// Line [s0, e1) of row `out`, e1 its terminator.  Longer than a row function's positions reach: reported, no row.  Otherwise
// row(src, s0, e1) parses it: s0 clamped, the CR stripped unless the terminator is the virtual one at the end of input, src
// reading from s0 on.  (row is a callable, not a bool to branch on: the kernels keep the branches they were measured with)
template <class Dev, class Row>
__device__ __forceinline__ void global_line(const Dev &a, ScanWsHeader *hdr, unsigned long long out, uint64_t s0, uint64_t e1, Row &&row) {
    if (e1 - s0 > 0x7FFFFFF0ull) {
        row_report(hdr, EXG_PE_FIELD_TOO_LONG, out, s0);
    } else {
        if (s0 > e1) s0 = e1;
        const bool virt = e1 >= a.n_bytes;
        if (!virt && e1 > s0 && a.d_in[e1 - 1] == '\r') e1--;
        row(GlobalSrc{a.d_in, s0, a.payload_base, (a.n_bytes + 15) & ~15ull}, s0, e1);
    }
}

// ---- fused: the any-shape scan ------------------------------------------------------------------------------
template <class R>
struct LineRowsFormat {
    using Dev = LineRowsDev<R::kColumns>;
    static constexpr int kNlCap = R::kNlCap;  // denser halves go in passes
    static constexpr int kHalves = R::kHalvesFull;  // (no lean instance: only kFullPrimary is instantiated)
    static constexpr int kHalvesFull = R::kHalvesFull;
    // a line's tabs come from its 64-byte words in LDS, read when the line is cut (LdsSrc::tabs64): no '\t' map
    static constexpr bool kTabMapLean = false, kTabMapFull = false;
    static constexpr bool kBarriers = false;
    static constexpr bool kParkHalf0 = false;
    static constexpr int kMinWavesPerSimd = R::kWavesFull, kMinWavesPerSimdRedo = R::kWavesFull;
    static constexpr int kMinWavesPerSimdFull = R::kWavesFull;
    __device__ static __forceinline__ uint32_t eof_extra_lines(unsigned long long) { return 0; }
    __device__ static __forceinline__ unsigned long long analytic_prefix(uint64_t) { return 0; }

    template <int kMode, class L>
    __device__ static __forceinline__ void emit_half(const L &s, const Dev &a, ScanWsHeader *hdr, const TileCtx &c, unsigned long long halo_nl,
                                                     uint32_t dev_mode, uint32_t lane, uint32_t wave, unsigned long long *__restrict__ tile_qend,
                                                     uint64_t tile_index) {
        static_assert(kMode == kFullPrimary, "a line-row scan has the any-shape instance only");
        const uint32_t tid = threadIdx.x;  // this thread's line of a pass of 256
        const unsigned long long qend_word = half_qend(s, c, a.n_bytes, tid == 0, tile_qend, tile_index);
        if (dev_mode == 3 || dev_mode == 4) return;
        const bool no_store = (a.flags & EXG_F_NO_STORE) != 0;
        const LdsSrc<L> src{s, a.payload_base + c.tile_off - kWin, s.tabmap[0]};
        for (uint32_t jb = 0; jb < c.n_lines; jb += kThreads) {
            const uint32_t j = jb + tid;
            const long long out = (long long)(c.P + j) - (long long)halo_nl;
            bool act = j < c.n_lines;
            int e1 = 0;
            if (act) {
                e1 = s.nlist[4 + j];
                act = (uint64_t)((int64_t)c.tile_off + e1 - kWin) >= a.lead && out >= 0;
                if (act && !no_store && (unsigned long long)out >= a.capacity) {
                    atomicOr(&hdr->flags, EXG_RF_CAPACITY);
                    act = false;
                }
            }
            uint32_t valid = 0;
            if (act) {
                const uint32_t q0 = s.nlist[3 + j];  // newline before the line
                if (q0 == kNoneE) {
                    mark_far_line(s, c, a.n_bytes, e1, out, qend_word, hdr, tile_qend, tile_index);
                } else {
                    const int s0 = (int)q0 + 1;
                    if (e1 > s0 && !(c.is_eof_tile && e1 == c.lim_e) && ldb(s, e1 - 1) == '\r') e1--;
                    RowInfo r = R::line(src, s0, e1, a, (unsigned long long)out, !no_store && dev_mode != 2);
                    if (!r.code && c.non_ascii && !utf8_valid_lds(s, s0, e1)) r.code = EXG_PE_INVALID_UTF8;  // noodles reads lines into a String
                    if (r.code) row_report(hdr, r.code, (unsigned long long)out, c.tile_off + s0 - kWin);
                    else valid = r.valid;
                    note_skipped<R>(hdr, r);
                }
            }
            if (!no_store) store_row_validity<R>(a, valid, (long long)(c.P + jb + wave * 64) - (long long)halo_nl, lane);
        }
    }
};

// ---- general path: thread = line, bytes from global memory -----------------------------------------------
template <class R>
__global__ __launch_bounds__(256) void k_line_rows(LineRowsDev<R::kColumns> a, const uint64_t *__restrict__ nl_pos, ScanWsHeader *hdr) {
    const uint64_t T = hdr->total_lines < hdr->lines_cap ? hdr->total_lines : hdr->lines_cap;
    const uint64_t halo = hdr->halo_nl;
    const bool no_store = (a.flags & EXG_F_NO_STORE) != 0;
    const uint64_t n_iter = (T + 63) / 64;
    const uint64_t wave_id = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t it = wave_id; it < n_iter; it += n_waves) {
        const uint64_t j = it * 64 + lane_id();
        bool act = j < T && j >= halo;
        const uint64_t out = j - halo;
        if (act && !no_store && out >= a.capacity) {
            atomicOr(&hdr->flags, EXG_RF_CAPACITY);
            act = false;
        }
        uint32_t valid = 0;
        if (act) {
            const uint64_t e1 = nl_pos[j];
            const bool resolved = j > 0 || (a.flags & EXG_F_BOF);
            const uint64_t s0 = j > 0 ? nl_pos[j - 1] + 1 : 0;
            if (!resolved) head_unresolved(hdr);
            else global_line(a, hdr, out, s0, e1, [&](const GlobalSrc &src, uint64_t s0, uint64_t e1) {
                RowInfo r = R::line(src, 0, (int)(e1 - s0), a, out, !no_store);
                if (!r.code && (hdr->flags & EXG_RF_NON_ASCII) && !utf8_valid_global(a.d_in, s0, e1)) r.code = EXG_PE_INVALID_UTF8;
                if (r.code) row_report(hdr, r.code, out, s0);
                else valid = r.valid;
                note_skipped<R>(hdr, r);
            });
        }
        if (!no_store) store_row_validity<R>(a, valid, (long long)(it * 64) - (long long)halo, lane_id());
    }
}

// The rows k_fused<LineRowsFormat<R>> left out: one line per marked half (it begins in front of the half's window — a line longer
// than a half always does), read from global memory like the general path reads its lines.  Runs behind k_fused on the stream.
template <class R, uint32_t kHalves>
__global__ __launch_bounds__(256) void k_line_far(LineRowsDev<R::kColumns> a, const unsigned int *__restrict__ tileA, const int32_t *__restrict__ tileL,
                                                  const unsigned long long *__restrict__ tile_qend, const FarRec *__restrict__ far_rec,
                                                  ScanWsHeader *hdr, uint32_t n_halves) {
    if (!hdr->any_far) return;
    constexpr uint64_t kSuper = (uint64_t)kHalves * kTile;
    const bool no_store = (a.flags & EXG_F_NO_STORE) != 0;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n_halves; x += (uint64_t)gridDim.x * blockDim.x) {
        if (!(tile_qend[x] & kFarBit)) continue;
        const FarRec f = far_rec[x];
        int64_t p[2];
        const unsigned long long out = (unsigned long long)f.out;
        if (!far_positions<2>(f, (uint32_t)(x / kHalves), kSuper, tileA, tileL, (a.flags & EXG_F_BOF) != 0, p)) {
            head_unresolved(hdr);
            continue;
        }
        global_line(a, hdr, out, (uint64_t)(p[0] + 1), (uint64_t)p[1], [&](const GlobalSrc &src, uint64_t s0, uint64_t e1) {
            RowInfo r = R::line(src, 0, (int)(e1 - s0), a, out, !no_store);
            if (!r.code && tiles_non_ascii(tileA, kSuper, (int64_t)s0, (int64_t)e1) && !utf8_valid_global(a.d_in, s0, e1)) r.code = EXG_PE_INVALID_UTF8;
            note_skipped<R>(hdr, r);
            if (r.code) {
                row_report(hdr, r.code, out, s0);
            } else if (!no_store) {
#pragma unroll
                for (int b = 0; b < R::kValidBits; b++)
                    if (((r.valid >> b) & 1u) && a.d_valid[R::valid_col(b)])
                        atomicOr((unsigned long long *)&a.d_valid[R::valid_col(b)][out >> 6], 1ull << (out & 63));
            }
        });
    }
}

// Result block (exg_lines.hip).  fused != 0: positions come from tile_qend; else from nl_pos.
__global__ void k_line_rows_finalize(uint64_t n_bytes, uint64_t lead, uint64_t capacity, uint32_t flags, ScanWsHeader *hdr,
                                     const unsigned long long *__restrict__ tile_qend, uint32_t n_tiles, const uint64_t *__restrict__ nl_pos,
                                     int fused, exg_scan_result *res);
__global__ void k_init_hdr(ScanWsHeader *hdr, uint64_t lines_cap, uint32_t mode);

template <class R>
static int run_line_rows_general(const LineRowsDev<R::kColumns> &dev, uint8_t *ws, const FastqWsLayout &l, exg_scan_result *d_result, hipStream_t stream) {
    ScanWsHeader *hdr = reinterpret_cast<ScanWsHeader *>(ws);
    const uint64_t *nl_pos = reinterpret_cast<const uint64_t *>(ws + l.off_nl_pos);
    hipLaunchKernelGGL(k_init_hdr, dim3(1), dim3(1), 0, stream, hdr, l.lines_cap, 0u);
    const int rc = launch_line_index(dev.d_in, dev.n_bytes, dev.lead, ws, l, (dev.flags & EXG_F_EOF) ? 1 : 0, 0, stream);
    if (rc) return rc;
    const uint64_t est = dev.n_bytes / R::kGeneralBytesPerLine + 256;
    const uint32_t grid = (uint32_t)((est + 255) / 256 < 2048 ? (est + 255) / 256 : 2048);
    hipLaunchKernelGGL(k_line_rows<R>, dim3(grid), dim3(256), 0, stream, dev, nl_pos, hdr);
    hipLaunchKernelGGL(k_line_rows_finalize, dim3(1), dim3(256), 0, stream, dev.n_bytes, dev.lead, dev.capacity, dev.flags, hdr,
                       (const unsigned long long *)nullptr, 0u, nl_pos, 0, d_result);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

template <class R>
static int run_line_rows_fused(const LineRowsDev<R::kColumns> &dev, uint8_t *ws, const FastqWsLayout &l, exg_scan_result *d_result, hipStream_t stream) {
    ScanWsHeader *hdr = reinterpret_cast<ScanWsHeader *>(ws);
    constexpr uint32_t kHalvesHost = R::kHalvesFull;
    const uint64_t kSuperBytes = (uint64_t)kHalvesHost * kTile;
    uint64_t n_super64 = (dev.n_bytes + kSuperBytes - 1) / kSuperBytes;
    if (n_super64 == 0) n_super64 = 1;
    if (n_super64 > 0x7FFFFFF0ull / kHalvesHost) {
        set_error("%s: buffer too large for one launch", R::kName);
        return EXG_E_INVALID_ARG;
    }
    const uint32_t n_super = (uint32_t)n_super64;
    // descriptor block (exg_fastq_ws.hpp): u64 tileA[n] (u32 counts), u64 tileP[n], u64 tile_redo[n] (unused here), u64 tile_qend[n],
    // int32 tileL[n][4], FarRec[n]
    const uint64_t n = l.n_tiles_fused;
    unsigned int *tileA = reinterpret_cast<unsigned int *>(ws + l.off_tile_desc);
    unsigned long long *tileP = reinterpret_cast<unsigned long long *>(ws + l.off_tile_desc) + n;
    unsigned long long *tile_qend = tileP + 2 * n;
    int32_t *tileL = reinterpret_cast<int32_t *>(ws + l.off_tile_last4);
    FarRec *far_rec = reinterpret_cast<FarRec *>(ws + l.off_far);
    hipLaunchKernelGGL(k_init_hdr, dim3(1), dim3(1), 0, stream, hdr, l.lines_cap, 0u);
    EXG_HIP_CHECK(hipMemsetAsync(tileA, 0, (size_t)n * 24, stream));
    if (dev.lead) {
        const int rc = exg_count_newlines(dev.d_in, 0, dev.lead, (uint64_t *)&hdr->halo_nl, stream);
        if (rc) return rc;
    }
    hipLaunchKernelGGL((k_fused<LineRowsFormat<R>, kFullPrimary>), dim3(n_super + 1), dim3(kThreads), 0, stream, dev, tileA, tileP, tile_qend, hdr, n_super);
    // the rows of lines that begin in front of their half's window (returns at once when there is none)
    const uint32_t n_halves = n_super * kHalvesHost;
    const uint32_t grid = (n_halves + 255) / 256 < 4096 ? (n_halves + 255) / 256 : 4096;
    hipLaunchKernelGGL((k_line_far<R, kHalvesHost>), dim3(grid), dim3(256), 0, stream, dev, tileA, tileL, tile_qend, far_rec, hdr, n_halves);
    hipLaunchKernelGGL(k_line_rows_finalize, dim3(1), dim3(256), 0, stream, dev.n_bytes, dev.lead, dev.capacity, dev.flags, hdr, tile_qend, n_halves,
                       (const uint64_t *)nullptr, 1, d_result);
    EXG_HIP_CHECK(hipGetLastError());
    return EXG_OK;
}

// The C entry of a format: Args is its exg_*_scan_args (the same fields, kColumns column and validity pointers)
template <class R, class Args>
static int line_rows_scan(const Args *a) {
    if (!a || !a->d_result || !a->d_workspace || ((uintptr_t)a->d_workspace & 255) || (a->n_bytes && !a->d_input) ||
        ((uintptr_t)a->d_input & 15) || a->lead > a->n_bytes) {
        set_error("%s: bad arguments (null pointer, unaligned input or workspace, or lead > n_bytes)", R::kName);
        return EXG_E_INVALID_ARG;
    }
    if (a->flags & ~EXG_F_ALL) {
        set_error("%s: unknown flag bits 0x%x", R::kName, a->flags & ~EXG_F_ALL);
        return EXG_E_INVALID_ARG;
    }
    if (a->algo == EXG_ALGO_FUSED_INDEX || a->algo > EXG_ALGO_FUSED_INDEX) {
        set_error("%s: algo %u is not one of the %s scan's (EXG_ALGO_FUSED_INDEX is exg_vcf_scan's alone)", R::kName, a->algo, R::kLabel);
        return EXG_E_INVALID_ARG;
    }
    const FastqWsLayout l = fastq_ws_layout(a->n_bytes, a->workspace_bytes);
    if (a->workspace_bytes < fastq_ws_layout(a->n_bytes, 0).off_nl_pos + 64) {
        set_error("%s: workspace too small", R::kName);
        return EXG_E_INVALID_ARG;
    }
    LineRowsDev<R::kColumns> dev;
    dev.d_in = (const uint8_t *)a->d_input;
    dev.n_bytes = a->n_bytes;
    dev.lead = a->lead;
    dev.first_line_index = 0;
    dev.payload_base = a->payload_base;
    dev.flags = a->flags;
    dev.pad = 0;
    for (int c = 0; c < R::kColumns; c++) {
        dev.d_col[c] = a->d_columns[c];
        dev.d_valid[c] = nullptr;
    }
    hipStream_t stream = (hipStream_t)a->stream;
    const size_t vb = a->flags & EXG_F_NO_STORE ? 0 : (size_t)((a->capacity_records + 63) / 64) * 8;
    for (int b = 0; b < R::kValidBits; b++) {  // only the columns that have validity words and are produced
        const int c = R::valid_col(b);
        if (!a->d_columns[c]) continue;
        dev.d_valid[c] = a->d_validity[c];
        if (vb && dev.d_valid[c]) EXG_HIP_CHECK(hipMemsetAsync(dev.d_valid[c], 0, vb, stream));
    }
    dev.capacity = a->capacity_records;
    uint8_t *ws = (uint8_t *)a->d_workspace;
    if (a->algo == EXG_ALGO_MULTIPASS) return run_line_rows_general<R>(dev, ws, l, a->d_result, stream);
    return run_line_rows_fused<R>(dev, ws, l, a->d_result, stream);  // EXG_ALGO_AUTO, EXG_ALGO_FUSED, EXG_ALGO_FUSED_FULL: one scan
}

}  // namespace exg
