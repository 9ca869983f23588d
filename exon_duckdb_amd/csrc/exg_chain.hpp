// exg_chain.hpp — finding delimiter-less binary records (BAM: exg_bam.hip, BCF: exg_bcf.hip) on decoded bytes in HBM.
//
// Record k + 1 begins where record k says it ends: one dependent load per record.  The chain is broken up by SPECULATION and
// repaired by a STITCH, so that the result is exactly the serial chain from byte 0:
//
//   k_speculate  one wavefront per 32 KiB tile: all lanes test candidate offsets for a plausible record (the format's test);
//                from the first hit one lane walks the chain to the tile's end and notes entry, exit (the first start at or
//                behind the tile's end), record count and how the walk stopped.
//   k_stitch     one workgroup, the tile table staged through LDS 2048 tiles at a time: the chain from byte 0 visits tile
//                t = cur / 32 KiB; the tile's speculated walk is taken when its entry is exactly `cur`, else the tile is
//                walked again from `cur` (rewalked).  Tiles a long record jumps over are never looked at.  The running
//                row count is every visited tile's first row: no separate scan.  One wavefront does it, 64 tiles at a step
//                where every one of them is entered exactly where it was speculated (the usual case), else tile by tile.
//   k_index      one thread per visited tile: the record offsets, from the true entry.
//
// Speculation is never a source of truth: a tile's walk is used only when the true chain arrives at its entry, and a walk is
// a pure function of its entry.  Bytes that look like a record cost a second walk, not a row.
//
// A format F (passed by value) has
//   __device__ int step(const uint8_t *in, uint64_t n, uint64_t s, uint64_t *next) const
//       0: a complete record at s (*next = the one behind it), 1: the tail (no complete record at s), > 1: the chain ends here
//   __device__ uint64_t next(const uint8_t *in, uint64_t s) const      the same for a record known to be complete
//   __device__ bool plausible(const uint8_t *in, uint64_t n, uint64_t s) const
// and the stitch ends with fin(rows, cur, rewalked, stopped) on one thread.
#pragma once
#include "exg_common.hpp"

namespace exg {
namespace chain {

static constexpr uint32_t kTileBytes = 32768;
static constexpr uint64_t kNone = ~0ull;
static constexpr uint32_t kStitchChunk = 2048;

struct Tiles {
    uint64_t *spec_entry, *spec_exit, *true_entry, *row_base;
    uint32_t *spec_cnt, *spec_stop, *cnt;
    uint64_t tiles;
};
inline uint64_t tiles_of(uint64_t n) { return n / kTileBytes + 1; }

#if defined(__HIPCC__)

__device__ __forceinline__ uint32_t ld32(const uint8_t *p) {  // (records are byte aligned)
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// the records that begin in [s, hi): a pure function of s
template <class F>
__device__ void walk(const F &f, const uint8_t *in, uint64_t n, uint64_t s, uint64_t hi, uint32_t *cnt, uint64_t *exit, uint32_t *stop) {
    uint32_t c = 0, st = 0;
    while (s < hi) {
        uint64_t nx = 0;
        st = (uint32_t)f.step(in, n, s, &nx);
        if (st) break;
        c++;
        s = nx;
    }
    *cnt = c, *exit = s, *stop = st;
}

template <class F>
__global__ __launch_bounds__(256) void k_speculate(const uint8_t *__restrict__ in, uint64_t n, F f, Tiles w) {
    const uint64_t t = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= w.tiles) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t lo = t * kTileBytes, hi = lo + kTileBytes < n ? lo + kTileBytes : n;
    uint64_t entry = kNone;
    if (t == 0) {
        entry = 0;  // the buffer begins at a record start
    } else {
        for (uint64_t base = lo; base < hi; base += 64) {
            const uint64_t cand = base + lane;
            const bool ok = cand < hi && f.plausible(in, n, cand);
            const unsigned long long m = __ballot(ok);
            if (m) {
                entry = base + (uint64_t)__builtin_ctzll(m);
                break;
            }
        }
    }
    if (lane) return;
    uint32_t cnt = 0, stop = 0;
    uint64_t exit = entry;
    if (entry != kNone) walk(f, in, n, entry, hi, &cnt, &exit, &stop);
    w.spec_entry[t] = entry, w.spec_exit[t] = exit, w.spec_cnt[t] = cnt, w.spec_stop[t] = stop;
}

template <class F, class Fin>
__global__ __launch_bounds__(256) void k_stitch(const uint8_t *__restrict__ in, uint64_t n, F f, Tiles w, Fin fin) {
    __shared__ uint64_t s_entry[kStitchChunk], s_exit[kStitchChunk];
    __shared__ uint32_t s_cnt[kStitchChunk], s_stop[kStitchChunk];
    __shared__ uint64_t s_cur, s_rows, s_rewalked;
    __shared__ uint32_t s_done, s_stopped;
    if (threadIdx.x == 0) s_cur = 0, s_rows = 0, s_rewalked = 0, s_done = 0, s_stopped = 0;
    __syncthreads();
    for (uint64_t c0 = 0; c0 < w.tiles; c0 += kStitchChunk) {
        if (s_done) break;  // (uniform: written before the barrier below)
        if (s_cur / kTileBytes >= c0 + kStitchChunk) continue;  // a record jumped over the whole chunk
        for (uint32_t i = threadIdx.x; i < kStitchChunk && c0 + i < w.tiles; i += 256) {
            s_entry[i] = w.spec_entry[c0 + i], s_exit[i] = w.spec_exit[c0 + i];
            s_cnt[i] = w.spec_cnt[c0 + i], s_stop[i] = w.spec_stop[c0 + i];
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            // wave 0, every lane with the same cur / rows (what differs per lane is said so).  The common case — the chain enters 64
            // tiles in a row exactly where they were speculated — is taken 64 tiles at a step: lane l holds tile t + l and checks
            // that its walk ends where tile t + l + 1's begins; anything else goes one tile at a time
            const uint32_t lane = threadIdx.x;
            const uint64_t loaded = w.tiles - c0 < kStitchChunk ? w.tiles - c0 : kStitchChunk;
            uint64_t cur = s_cur, rows = s_rows, rewalked = s_rewalked;
            for (;;) {
                if (cur >= n) {
                    s_done = 1;
                    break;
                }
                const uint64_t t = cur / kTileBytes;
                if (t >= c0 + kStitchChunk) break;
                const uint32_t i = (uint32_t)(t - c0);
                if (i + 64 < loaded) {
                    const uint64_t e = s_entry[i + lane], x = s_exit[i + lane];
                    const uint32_t c = s_cnt[i + lane];
                    const bool ok = s_stop[i + lane] == 0 && x == s_entry[i + lane + 1] && x / kTileBytes == t + lane + 1 && (lane != 0 || e == cur);
                    if (__all(ok)) {
                        const uint32_t incl = wave_incl_sum(c);
                        w.true_entry[t + lane] = e, w.row_base[t + lane] = rows + incl - c, w.cnt[t + lane] = c;
                        rows += __shfl(incl, 63, 64);
                        cur = __shfl((unsigned long long)x, 63, 64);
                        continue;
                    }
                }
                uint32_t cnt = s_cnt[i], stop = s_stop[i];
                uint64_t exit = s_exit[i];
                if (s_entry[i] != cur) {
                    const uint64_t hi = (t + 1) * kTileBytes < n ? (t + 1) * kTileBytes : n;
                    walk(f, in, n, cur, hi, &cnt, &exit, &stop);  // (all lanes the same loads)
                    rewalked++;
                }
                if (!lane) w.true_entry[t] = cur, w.row_base[t] = rows, w.cnt[t] = cnt;
                rows += cnt;
                cur = exit;
                if (stop) {
                    s_done = 1, s_stopped = stop;
                    break;
                }
            }
            if (!lane) s_cur = cur, s_rows = rows, s_rewalked = rewalked;
        }
        __syncthreads();
    }
    if (threadIdx.x) return;
    fin(s_rows, s_cur, s_rewalked, s_stopped);
}

template <class F>
__global__ __launch_bounds__(256) void k_index(const uint8_t *__restrict__ in, F f, Tiles w, uint64_t *rec_off) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= w.tiles) return;
    uint64_t s = w.true_entry[t];
    if (s == kNone) return;
    uint64_t row = w.row_base[t];
    for (uint32_t k = w.cnt[t]; k; k--) {  // (the stitch counted complete records: every length read here lies inside the buffer)
        rec_off[row++] = s;
        s = f.next(in, s);
    }
}

// true_entry = none, speculate, stitch: the caller reads what `fin` wrote and launches index() for the rows found
template <class F, class Fin>
inline hipError_t find(const uint8_t *in, uint64_t n, const F &f, const Tiles &w, const Fin &fin, hipStream_t st) {
    hipError_t e = hipMemsetAsync(w.true_entry, 0xFF, w.tiles * 8, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_speculate<F>), dim3((uint32_t)((w.tiles + 3) / 4)), dim3(256), 0, st, in, n, f, w);
    hipLaunchKernelGGL((k_stitch<F, Fin>), dim3(1), dim3(256), 0, st, in, n, f, w, fin);
    return hipSuccess;
}
template <class F>
inline void index(const uint8_t *in, const F &f, const Tiles &w, uint64_t *rec_off, hipStream_t st) {
    hipLaunchKernelGGL((k_index<F>), dim3((uint32_t)((w.tiles + 255) / 256)), dim3(256), 0, st, in, f, w, rec_off);
}

#endif  // __HIPCC__

}  // namespace chain
}  // namespace exg
