// exg_bzip2.hip — bzip2 on the device (the split of the work: exg_bzip2.hpp).
//
// Decoding follows libbz2 1.0.8 (decompress.c): the same Huffman decode procedure (limit / base / perm, so that a code
// the encoder would never write decodes the same way), the same limits (nGroups 2..6, selectors beyond 18002 read and
// ignored, code lengths 1..20, run lengths below 2^21), the same RLE1 rule at the end of a block (a block that ends on a
// fourth equal byte, where a count byte is due, is a data error), and the same walk over the LF mapping: nblock steps
// from origPtr.  A periodic block (a run of three equal bytes, the RLE1 output of a long run) has an LF mapping of
// several cycles, and libbz2 repeats the cycle that holds origPtr; so does this decoder (the block CRC is what tells a
// damaged mapping).  Randomised blocks (bzip2 < 0.9.5) are refused.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "exg_bzip2.hpp"
#include "exg_common.hpp"
#include "exg_reader.hpp"

namespace exg {
namespace bz2 {

namespace {

constexpr uint64_t kMagicBlock = 0x314159265359ull, kMagicEnd = 0x177245385090ull;
constexpr int kLutBits = 10;
constexpr uint32_t kMaxSelectors = 18002;
constexpr uint32_t kChunk = 8192;    // counting-sort chunk (one wavefront each)
constexpr uint32_t kStride = 256;    // splitter spacing of the LF walk
constexpr uint32_t kPiece = 4096;    // RLE1 piece
constexpr uint32_t kPoly = 0x04C11DB7u;

// candidate status (kOk .. kOverflow are not data errors)
enum : uint32_t {
    kOk = 0,
    kNeedMore = 1,   // the block runs past the end of the window
    kOverflow = 2,   // more symbols than the round's slot holds
    kErrFirst = 8,
    kErrRandomised = 8,
    kErrNoSymbols,
    kErrGroups,
    kErrSelectors,
    kErrCodeLength,
    kErrHuffman,
    kErrNoSelector,
    kErrRunLength,
    kErrBlockSize,
    kErrOrigPtr,
    kErrMagic,
    kErrCycle,
    kErrRunAtEnd,
    kErrBlockCrc,
    kErrStreamCrc,
    kErrNotBzip2,
    kErrTruncated,
};

const char *reason_text(uint32_t s) {
    switch (s) {
    case kErrRandomised: return "randomised block (written by bzip2 < 0.9.5) is not supported";
    case kErrNoSymbols: return "no byte values in use";
    case kErrGroups: return "number of Huffman groups outside 2..6";
    case kErrSelectors: return "bad selector";
    case kErrCodeLength: return "Huffman code length outside 1..20";
    case kErrHuffman: return "bad Huffman code";
    case kErrNoSelector: return "symbols run past the last selector";
    case kErrRunLength: return "run length too large";
    case kErrBlockSize: return "block larger than the stream's level allows";
    case kErrOrigPtr: return "origPtr outside the block";
    case kErrMagic: return "bad block magic";
    case kErrCycle: return "inconsistent BWT mapping";
    case kErrRunAtEnd: return "block ends where a run-length byte is due";
    case kErrBlockCrc: return "block CRC mismatch";
    case kErrStreamCrc: return "stream CRC mismatch";
    default: return "bad block";
    }
}

struct CandOut {  // what the symbol stage leaves per candidate
    uint32_t status, nblock, orig, crc;
    uint64_t end_bit;
};

struct ChainOut {  // what the chaining thread leaves for the host
    uint32_t n_blocks, n_events, status, err_block;
    uint64_t bit_end;
    uint32_t at_header, level, done, pad;
};

// ---------------------------------------------------------------- bit reader (MSB first, aligned 16-byte loads ahead)
// (the 16 bytes in hand are two registers that shift: an indexed array would live in scratch memory, a global access per word)
struct BitReader {
    const uint4 *q;
    uint64_t nbits, pos;
    uint64_t buf;
    int cnt;
    uint64_t wa, wb;  // the words still in hand, first one in the high half of wa
    int wn;           // how many
    uint64_t qi;
    uint4 nxt;
    __device__ static uint64_t pair(uint32_t x, uint32_t y) { return (uint64_t)__builtin_bswap32(x) << 32 | __builtin_bswap32(y); }
    __device__ void init(const void *base, uint64_t nbits_, uint64_t pos0) {
        q = (const uint4 *)base;
        nbits = nbits_;
        const uint64_t w = pos0 >> 5;  // first 32-bit word
        qi = w >> 2;
        const uint4 c = q[qi];
        nxt = q[qi + 1];
        qi += 2;
        wa = pair(c.x, c.y), wb = pair(c.z, c.w), wn = 4;
        for (int i = 0; i < (int)(w & 3); i++) wa = wa << 32 | wb >> 32, wb <<= 32, wn--;
        buf = 0;
        cnt = 0;
        pos = pos0 & ~31ull;
        refill();
        skip((int)(pos0 & 31));
    }
    __device__ uint32_t word() {
        if (wn == 0) {
            wa = pair(nxt.x, nxt.y), wb = pair(nxt.z, nxt.w), wn = 4;
            nxt = q[qi++];
        }
        const uint32_t v = (uint32_t)(wa >> 32);
        wa = wa << 32 | wb >> 32, wb <<= 32, wn--;
        return v;
    }
    __device__ void refill() {
        if (cnt <= 32) {
            buf |= (uint64_t)word() << (32 - cnt);
            cnt += 32;
        }
    }
    __device__ void skip(int k) {
        buf <<= k;
        cnt -= k;
        pos += k;
    }
    // k <= 32 bits; false: past the end of the window
    __device__ bool get(int k, uint32_t *v) {
        if (pos + k > nbits) return false;
        refill();
        *v = k ? (uint32_t)(buf >> (64 - k)) : 0;
        skip(k);
        return true;
    }
    __device__ uint32_t peek(int k) {  // k <= 32
        refill();
        return (uint32_t)(buf >> (64 - k));
    }
};

// ---------------------------------------------------------------- (1) discovery
__global__ void k_discover(const uint32_t *__restrict__ d, uint64_t n, uint64_t bit0, unsigned long long *cand, uint32_t cap, uint32_t *count) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t * 4 >= n) return;
    const uint64_t hi = ((uint64_t)__builtin_bswap32(d[t]) << 32) | __builtin_bswap32(d[t + 1]);
    const uint32_t lo = __builtin_bswap32(d[t + 2]);
    const uint64_t nbits = n * 8;
    for (int o = 0; o < 32; o++) {
        const uint64_t p = t * 32 + o;
        if (p < bit0 || p + 48 > nbits) continue;
        const uint64_t a = (hi << o) | (o ? (uint64_t)lo >> (32 - o) : 0);
        const uint64_t x = a >> 16;
        if (x == kMagicBlock || x == kMagicEnd) {
            const uint32_t i = atomicAdd(count, 1u);
            if (i < cap) cand[i] = (p << 1) | (x == kMagicEnd ? 1 : 0);
        }
    }
}

__global__ void k_rank_sort(const unsigned long long *in, unsigned long long *out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long v = in[i];
    uint32_t r = 0;
    for (uint32_t j = 0; j < n; j++) r += in[j] < v;
    out[r] = v;
}

// ---------------------------------------------------------------- (2) header, tables, symbols: one wavefront per candidate
struct SymShared {
    int32_t limit[6][23], base[6][23];
    uint16_t perm[6][258];
    uint16_t lut[6][1 << kLutBits];  // sym << 5 | length; length 0: longer than kLutBits; 31: bad code
    uint8_t minlen[6];
    uint8_t len[6][258];
    uint8_t selector[kMaxSelectors];
    uint8_t seq_to_unseq[256];
    uint8_t mtf[256];
    uint32_t n_in_use, n_groups, n_selectors, alpha, status, orig, crc;
    uint64_t pos;
};

__device__ __forceinline__ void put_bytes(uint8_t *out, uint32_t at, uint8_t b, uint32_t k) {
    // k copies of b at out[at..): whole dwords in the middle
    uint32_t i = 0;
    while (i < k && ((uintptr_t)(out + at + i) & 3)) out[at + i++] = b;
    const uint32_t w = b * 0x01010101u;
    for (; i + 4 <= k; i += 4) *(uint32_t *)(out + at + i) = w;
    while (i < k) out[at + i++] = b;
}

__global__ void __launch_bounds__(64) k_symbols(const uint8_t *__restrict__ comp, uint64_t nbits, const unsigned long long *__restrict__ cand, uint32_t n_cand,
                                                uint8_t *__restrict__ ll, uint32_t slot, CandOut *outs) {
    __shared__ SymShared S;
    const uint32_t c = blockIdx.x;
    const int lane = threadIdx.x;
    if (c >= n_cand) return;
    const unsigned long long cv = cand[c];
    CandOut *o = outs + c;
    if (cv & 1) {  // end-of-stream magic: nothing to decode
        if (lane == 0) o->status = kOk, o->nblock = 0, o->end_bit = cv >> 1;
        return;
    }
    BitReader br;
    if (lane == 0) {
        uint32_t st = kOk, v = 0;
        br.init(comp, nbits, (cv >> 1) + 48);
        uint32_t crc = 0, rnd = 0, orig = 0;
        auto G = [&](int k) -> uint32_t {
            if (st) return 0;
            if (!br.get(k, &v)) {
                st = kNeedMore;
                return 0;
            }
            return v;
        };
        crc = G(32);
        rnd = G(1);
        orig = G(24);
        if (!st && rnd) st = kErrRandomised;
        // symbol map
        uint32_t in16 = G(16), nin = 0;
        for (int i = 0; i < 16 && !st; i++)
            if (in16 & (0x8000u >> i)) {
                const uint32_t m = G(16);
                for (int j = 0; j < 16; j++)
                    if (m & (0x8000u >> j)) S.seq_to_unseq[nin++] = (uint8_t)(i * 16 + j);
            }
        if (!st && nin == 0) st = kErrNoSymbols;
        const uint32_t alpha = nin + 2;
        uint32_t ng = G(3);
        if (!st && (ng < 2 || ng > 6)) st = kErrGroups;
        uint32_t nsel = G(15);
        if (!st && nsel < 1) st = kErrSelectors;
        uint8_t pos6[6] = {0, 1, 2, 3, 4, 5};
        for (uint32_t i = 0; i < nsel && !st; i++) {
            uint32_t j = 0;
            for (;;) {
                const uint32_t b = G(1);
                if (st || !b) break;
                if (++j >= ng) {
                    st = kErrSelectors;
                    break;
                }
            }
            if (st) break;
            if (i < kMaxSelectors) {  // undo the MTF of the selectors as they come
                const uint8_t tmp = pos6[j];
                for (; j > 0; j--) pos6[j] = pos6[j - 1];
                pos6[0] = tmp;
                S.selector[i] = tmp;
            }
        }
        if (nsel > kMaxSelectors) nsel = kMaxSelectors;
        for (uint32_t t = 0; t < ng && !st; t++) {
            int32_t curr = (int32_t)G(5);
            for (uint32_t i = 0; i < alpha && !st; i++) {
                for (;;) {
                    if (curr < 1 || curr > 20) {
                        st = kErrCodeLength;
                        break;
                    }
                    if (!G(1) || st) break;
                    curr += G(1) ? -1 : 1;
                }
                S.len[t][i] = (uint8_t)curr;
            }
        }
        S.status = st;
        S.n_in_use = nin, S.alpha = alpha, S.n_groups = ng, S.n_selectors = nsel, S.orig = orig, S.crc = crc;
        S.pos = br.pos;
    }
    __syncthreads();
    if (S.status) {
        if (lane == 0) o->status = S.status, o->nblock = 0, o->end_bit = 0;
        return;
    }
    const uint32_t alpha = S.alpha, ng = S.n_groups;
    if ((uint32_t)lane < ng) {  // BZ2_hbCreateDecodeTables
        const int t = lane;
        int minl = 32, maxl = 0;
        for (uint32_t i = 0; i < alpha; i++) minl = min(minl, (int)S.len[t][i]), maxl = max(maxl, (int)S.len[t][i]);
        int pp = 0;
        for (int i = 0; i < 258; i++) S.perm[t][i] = 0xFFFF;
        for (int i = minl; i <= maxl; i++)
            for (uint32_t j = 0; j < alpha; j++)
                if (S.len[t][j] == i) S.perm[t][pp++] = (uint16_t)j;
        int32_t *base = S.base[t], *limit = S.limit[t];
        for (int i = 0; i < 23; i++) base[i] = 0, limit[i] = 0;
        for (uint32_t i = 0; i < alpha; i++) base[S.len[t][i] + 1]++;
        for (int i = 1; i < 23; i++) base[i] += base[i - 1];
        int32_t vec = 0;
        for (int i = minl; i <= maxl; i++) {
            vec += base[i + 1] - base[i];
            limit[i] = vec - 1;
            vec <<= 1;
        }
        for (int i = minl + 1; i <= maxl; i++) base[i] = ((limit[i - 1] + 1) << 1) - base[i];
        S.minlen[t] = (uint8_t)minl;
    }
    __syncthreads();
    for (uint32_t e = lane; e < ng << kLutBits; e += 64) {  // the first kLutBits bits of the same procedure
        const uint32_t t = e >> kLutBits, v = e & ((1u << kLutBits) - 1);
        int zn = S.minlen[t];
        uint16_t ent = 0;
        if (zn <= kLutBits) {
            int32_t zvec = (int32_t)(v >> (kLutBits - zn));
            while (zn <= kLutBits && zvec > S.limit[t][zn]) {
                zn++;
                zvec = (int32_t)(v >> (kLutBits - min(zn, kLutBits)));
            }
            if (zn <= kLutBits) {
                const int32_t k = zvec - S.base[t][zn];
                const uint16_t sym = (k < 0 || k >= 258) ? 0xFFFF : S.perm[t][k];
                ent = sym == 0xFFFF ? 31 : (uint16_t)(sym << 5 | zn);
            }
        }
        S.lut[t][v] = ent;
    }
    __syncthreads();
    if (lane != 0) return;
    // ---- symbols (lane 0): Huffman, RLE2, inverse MTF -> the BWT column
    uint32_t st = kOk;
    br.init(comp, nbits, S.pos);
    const uint32_t eob = S.n_in_use + 1, nsel = S.n_selectors;
    for (uint32_t i = 0; i < 256; i++) S.mtf[i] = (uint8_t)i;
    uint8_t *out = ll + (uint64_t)c * slot;
    uint32_t nblock = 0, group_pos = 0, group_no = 0, gsel = 0;
    bool first_group = true;
    auto next_sym = [&](uint32_t *sym) -> bool {
        if (group_pos == 0) {
            if (!first_group) group_no++;
            first_group = false;
            if (group_no >= nsel) {
                st = kErrNoSelector;
                return false;
            }
            group_pos = 50;
            gsel = S.selector[group_no];
        }
        group_pos--;
        const uint16_t ent = S.lut[gsel][br.peek(kLutBits)];
        int zn = ent & 31;
        if (zn == 31) {
            st = kErrHuffman;
            return false;
        }
        if (zn) {
            *sym = ent >> 5;
        } else {
            zn = max((int)S.minlen[gsel], kLutBits + 1);
            int32_t zvec = (int32_t)br.peek(zn);
            while (zvec > S.limit[gsel][zn]) {
                if (++zn > 20) {
                    st = kErrHuffman;
                    return false;
                }
                zvec = (int32_t)br.peek(zn);
            }
            const int32_t k = zvec - S.base[gsel][zn];
            const uint16_t s = (k < 0 || k >= 258) ? 0xFFFF : S.perm[gsel][k];
            if (s == 0xFFFF) {
                st = kErrHuffman;
                return false;
            }
            *sym = s;
        }
        if (br.pos + zn > br.nbits) {
            st = kNeedMore;
            return false;
        }
        br.skip(zn);
        return true;
    };
    uint32_t sym = 0;
    if (next_sym(&sym)) {
        for (;;) {
            if (sym == eob) break;
            if (sym <= 1) {  // RUNA / RUNB: bijective base 2
                uint32_t es = 0, N = 1;
                bool ok = true;
                do {
                    if (N >= (2u << 20)) {
                        st = kErrRunLength;
                        ok = false;
                        break;
                    }
                    es += (sym + 1) * N;
                    N <<= 1;
                    if (!next_sym(&sym)) {
                        ok = false;
                        break;
                    }
                } while (sym <= 1);
                if (!ok) break;
                const uint8_t uc = S.seq_to_unseq[S.mtf[0]];
                if ((uint64_t)nblock + es > kMaxBlock) {
                    st = kErrBlockSize;
                    break;
                }
                if (nblock + es > slot) {
                    st = kOverflow;
                    break;
                }
                put_bytes(out, nblock, uc, es);
                nblock += es;
                continue;
            }
            if (nblock >= kMaxBlock) {
                st = kErrBlockSize;
                break;
            }
            if (nblock >= slot) {
                st = kOverflow;
                break;
            }
            uint32_t nn = sym - 1;
            const uint8_t v = S.mtf[nn];
            for (; nn > 0; nn--) S.mtf[nn] = S.mtf[nn - 1];
            S.mtf[0] = v;
            out[nblock++] = S.seq_to_unseq[v];
            if (!next_sym(&sym)) break;
        }
    }
    if (!st && S.orig >= nblock) st = kErrOrigPtr;
    o->status = st;
    o->nblock = nblock;
    o->orig = S.orig;
    o->crc = S.crc;
    o->end_bit = br.pos;
}

// ---------------------------------------------------------------- chaining (one thread)
__device__ int find_cand(const unsigned long long *cand, uint32_t n, uint64_t p) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if ((cand[mid] >> 1) < p) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && (cand[lo] >> 1) == p ? (int)lo : -1;
}

__device__ uint32_t get_bits_at(const uint8_t *d, uint64_t p, int k) {  // k <= 32, readable to (p + k + 7) / 8 + 8
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v = v << 8 | d[(p >> 3) + i];
    return (uint32_t)((v << (p & 7)) >> (64 - k));
}

__global__ void k_chain(const uint8_t *comp, uint64_t n, const unsigned long long *cand, uint32_t n_cand, uint32_t n_dec, const CandOut *outs, uint64_t bit0,
                        uint32_t at_header, uint32_t first_stream, uint32_t level, uint32_t slot, uint32_t final_window, uint32_t max_blocks, uint32_t *chained,
                        uint32_t *events, ChainOut *res) {
    if (threadIdx.x || blockIdx.x) return;
    const uint64_t nbits = n * 8;
    uint64_t p = bit0;
    uint32_t m = 0, ne = 0, status = kOk, err_block = 0, done = 0;
    bool first = first_stream != 0;
    for (;;) {
        if (at_header) {
            const uint64_t b = p >> 3;
            if (b >= n) {  // (p is byte aligned here)
                if (final_window) {
                    if (first) status = kErrNotBzip2;
                    done = 1;
                }
                break;
            }
            if (b + 4 > n) {
                if (!final_window) break;
                // bytes behind a stream that are no stream are ignored, like bz2.decompress; the first bytes of a stream
                // header ("B", "BZ", "BZh") are a stream cut short, as bz2.decompress and the bzip2 program read them
                bool head = true;
                for (uint64_t i = b; i < n; i++) head = head && comp[i] == (i == b ? 'B' : i == b + 1 ? 'Z' : 'h');
                status = first ? kErrNotBzip2 : head ? kErrTruncated : kOk;
                done = 1;
                break;
            }
            if (comp[b] != 'B' || comp[b + 1] != 'Z' || comp[b + 2] != 'h' || comp[b + 3] < '1' || comp[b + 3] > '9') {
                if (first) status = kErrNotBzip2;
                done = 1;
                break;
            }
            level = comp[b + 3] - '0';
            p += 32;
            at_header = 0;
            first = false;
            continue;
        }
        if (m >= max_blocks) break;
        const int ci = find_cand(cand, n_cand, p);
        if (ci < 0) {
            if (p + 48 > nbits) {
                if (final_window) status = kErrTruncated;
            } else {
                status = kErrMagic;
            }
            break;
        }
        if ((uint32_t)ci >= n_dec) break;  // (not decoded in this round)
        if (cand[ci] & 1) {                // end of stream: the combined CRC, then padding to a byte
            if (p + 80 > nbits) {
                if (final_window) status = kErrTruncated;
                break;
            }
            events[2 * ne] = 1;
            events[2 * ne + 1] = get_bits_at(comp, p + 48, 32);
            ne++;
            p = (p + 80 + 7) & ~7ull;
            at_header = 1;
            continue;
        }
        const CandOut &o = outs[ci];
        if (o.status == kNeedMore) {
            if (final_window) status = kErrTruncated;
            break;
        }
        if (o.status == kOverflow) {
            if (slot >= level * 100000u) status = kErrBlockSize;
            break;
        }
        if (o.status == kOk && o.nblock > level * 100000u) status = kErrBlockSize;
        else status = o.status;
        if (status) {
            err_block = m;
            break;
        }
        chained[m++] = (uint32_t)ci;
        events[2 * ne] = 0;
        events[2 * ne + 1] = o.crc;
        ne++;
        p = o.end_bit;
    }
    res->n_blocks = m;
    res->n_events = ne;
    res->status = status;
    res->err_block = status ? m : err_block;  // (a refusal is of the block behind the m chained ones, whoever found it)
    res->bit_end = p;
    res->at_header = at_header;
    res->level = level;
    res->done = done;
}

// ---------------------------------------------------------------- (3) inverse BWT
struct BlkInfo {  // one per chained block
    const uint8_t *ll;  // its BWT column (then its BWT output)
    uint32_t nblock, orig, cycle, pad;
};

__global__ void k_gather(const uint32_t *chained, const CandOut *outs, uint8_t *ll, uint32_t slot, uint32_t m, BlkInfo *info) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint32_t c = chained[j];
    info[j].ll = ll + (uint64_t)c * slot;
    info[j].nblock = outs[c].nblock;
    info[j].orig = outs[c].orig;
    info[j].cycle = 0;
}

__global__ void __launch_bounds__(256) k_hist(const BlkInfo *info, uint32_t n_chunks, uint32_t *hist) {
    __shared__ uint32_t h[256];
    const uint32_t j = blockIdx.y, ch = blockIdx.x;
    h[threadIdx.x] = 0;
    __syncthreads();
    const BlkInfo b = info[j];
    const uint32_t lo = ch * kChunk, hi = min(lo + kChunk, b.nblock);
    for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) atomicAdd(&h[b.ll[i]], 1u);
    __syncthreads();
    hist[((uint64_t)j * n_chunks + ch) * 256 + threadIdx.x] = h[threadIdx.x];
}

// per block: hist[ch][c] := cftab[c] + the count of c in the chunks in front of ch
__global__ void __launch_bounds__(256) k_hist_prefix(const BlkInfo *info, uint32_t n_chunks, uint32_t *hist) {
    __shared__ uint32_t tot[256];
    const uint32_t j = blockIdx.x, c = threadIdx.x;
    const uint32_t nch = (info[j].nblock + kChunk - 1) / kChunk;
    uint32_t *H = hist + (uint64_t)j * n_chunks * 256;
    uint32_t run = 0;
    for (uint32_t ch = 0; ch < nch; ch++) {
        const uint32_t v = H[ch * 256 + c];
        H[ch * 256 + c] = run;
        run += v;
    }
    tot[c] = run;
    __syncthreads();
    if (c == 0) {
        uint32_t s = 0;
        for (int i = 0; i < 256; i++) {
            const uint32_t v = tot[i];
            tot[i] = s;
            s += v;
        }
    }
    __syncthreads();
    const uint32_t b0 = tot[c];
    for (uint32_t ch = 0; ch < nch; ch++) H[ch * 256 + c] += b0;
}

// the LF vector, stably: within a wavefront a byte's rank among the lanes below with the same byte comes from ballots
// over its eight bit planes; one lane per distinct byte moves the chunk's counter on.  tt[k] = (i << 8) | byte.
__global__ void __launch_bounds__(64) k_scatter(const BlkInfo *info, uint32_t n_chunks, const uint32_t *hist, uint32_t *tt, uint32_t slot) {
    __shared__ uint32_t ctr[256];
    const uint32_t j = blockIdx.y, ch = blockIdx.x, lane = threadIdx.x;
    const BlkInfo b = info[j];
    const uint32_t lo = ch * kChunk;
    if (lo >= b.nblock) return;
    const uint32_t hi = min(lo + kChunk, b.nblock);
    const uint32_t *H = hist + ((uint64_t)j * n_chunks + ch) * 256;
    for (uint32_t i = lane; i < 256; i += 64) ctr[i] = H[i];
    __syncthreads();
    uint32_t *T = tt + (uint64_t)j * slot;
    const unsigned long long below = (1ull << lane) - 1;
    for (uint32_t base = lo; base < hi; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < hi;
        const uint32_t v = valid ? b.ll[i] : 0;
        unsigned long long same = __ballot(valid);
        for (int bit = 0; bit < 8; bit++) {
            const bool on = (v >> bit) & 1;
            const unsigned long long plane = __ballot(on);
            same &= on ? plane : ~plane;
        }
        const uint32_t rank = __popcll(same & below);
        const uint32_t at = valid ? ctr[v] + rank : 0;
        __builtin_amdgcn_wave_barrier();
        if (valid) {
            T[at] = (i << 8) | v;
            if ((same >> lane) == 1ull) ctr[v] = at + 1;  // the highest lane of its byte
        }
        __builtin_amdgcn_wave_barrier();
    }
}

__device__ __forceinline__ uint32_t n_split(uint32_t nblock) { return (nblock + kStride - 1) / kStride + 1; }
__device__ __forceinline__ uint32_t split_index(uint32_t p, uint32_t orig, uint32_t ns) { return (p % kStride) == 0 ? p / kStride : (p == orig ? ns - 1 : ~0u); }

// pass 1: from every splitter to the next one along the mapping — the length and the successor
__global__ void k_walk_len(const BlkInfo *info, const uint32_t *tt, uint32_t slot, uint32_t split_cap, uint32_t *s_len, uint32_t *s_next, uint32_t *s_off, uint32_t *bad) {
    const uint32_t j = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    const BlkInfo b = info[j];
    const uint32_t ns = n_split(b.nblock);
    if (k >= ns) return;
    const uint64_t sb = (uint64_t)j * split_cap;
    s_off[sb + k] = ~0u;
    const uint32_t s = k == ns - 1 ? b.orig : k * kStride;
    const uint32_t *T = tt + (uint64_t)j * slot;
    uint32_t p = s, len = 0;
    for (;;) {
        p = T[p] >> 8;
        len++;
        if (p >= b.nblock || len > b.nblock) {
            atomicOr(bad, 1u);
            p = b.orig;
            break;
        }
        if ((p % kStride) == 0 || p == b.orig) break;
    }
    s_len[sb + k] = len;
    s_next[sb + k] = p;
}

// the splitters of origPtr's cycle in order: their offsets in the block's output, and the cycle's length
__global__ void k_walk_order(BlkInfo *info, uint32_t m, uint32_t split_cap, const uint32_t *s_len, const uint32_t *s_next, uint32_t *s_off, uint32_t *bad) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const BlkInfo b = info[j];
    const uint32_t ns = n_split(b.nblock);
    const uint64_t sb = (uint64_t)j * split_cap;
    uint32_t p = b.orig, off = 0;
    for (uint32_t steps = 0;; steps++) {
        const uint32_t k = split_index(p, b.orig, ns);
        if (k == ~0u || steps > ns || s_off[sb + k] != ~0u) {
            atomicOr(bad, 1u);
            break;
        }
        s_off[sb + k] = off;
        off += s_len[sb + k];
        p = s_next[sb + k];
        if (p == b.orig) break;
    }
    if (off > b.nblock) atomicOr(bad, 1u), off = b.nblock;
    info[j].cycle = off;
}

// pass 2: the same walks, writing the bytes at their offsets (into the block's column: the mapping holds the bytes now)
__global__ void k_walk_write(const BlkInfo *info, const uint32_t *tt, uint32_t slot, uint32_t split_cap, const uint32_t *s_off) {
    const uint32_t j = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    const BlkInfo b = info[j];
    const uint32_t ns = n_split(b.nblock);
    if (k >= ns) return;
    uint32_t off = s_off[(uint64_t)j * split_cap + k];
    if (off == ~0u) return;
    const uint32_t *T = tt + (uint64_t)j * slot;
    uint8_t *out = (uint8_t *)b.ll;
    uint32_t p = k == ns - 1 ? b.orig : k * kStride;
    for (uint32_t len = 0; len <= b.nblock; len++) {
        const uint32_t e = T[p];
        p = e >> 8;
        if (off < b.cycle) out[off++] = (uint8_t)e;
        if (p >= b.nblock || (p % kStride) == 0 || p == b.orig) break;
    }
}

// libbz2 walks nblock steps from origPtr: a cycle shorter than the block repeats
__global__ void k_repeat(const BlkInfo *info) {
    const uint32_t j = blockIdx.y;
    const BlkInfo b = info[j];
    if (b.cycle == 0 || b.cycle >= b.nblock) return;
    uint8_t *out = (uint8_t *)b.ll;
    for (uint32_t i = b.cycle + blockIdx.x * blockDim.x + threadIdx.x; i < b.nblock; i += gridDim.x * blockDim.x) out[i] = out[i % b.cycle];
}

// ---------------------------------------------------------------- (4) RLE1 undo + CRC
// state r: 0 = free, 1..3 = equal bytes so far, 4 = a count byte is due (the byte in front is the run's)
struct PieceInfo {
    uint32_t len[5];
    uint8_t exit[5], entry, pad[2];
    uint32_t off;  // output offset inside the block
};

__global__ void k_rle_size(const BlkInfo *info, uint32_t piece_cap, PieceInfo *pieces) {
    const uint32_t j = blockIdx.y, q = blockIdx.x * blockDim.x + threadIdx.x;
    const BlkInfo b = info[j];
    const uint32_t lo = q * kPiece;
    if (lo >= b.nblock) return;
    const uint32_t hi = min(lo + kPiece, b.nblock);
    uint32_t r[5] = {0, 1, 2, 3, 4}, len[5] = {0, 0, 0, 0, 0};
    uint32_t prev = lo ? b.ll[lo - 1] : 0;
    const uint8_t *in = b.ll;
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t x = in[i];
#pragma unroll
        for (int s = 0; s < 5; s++) {
            if (r[s] == 4) len[s] += x, r[s] = 0;
            else if (r[s] && x == prev) len[s]++, r[s]++;
            else len[s]++, r[s] = 1;
        }
        prev = x;
    }
    PieceInfo &P = pieces[(uint64_t)j * piece_cap + q];
    for (int s = 0; s < 5; s++) P.len[s] = len[s], P.exit[s] = (uint8_t)r[s];
}

// per block: entry states and offsets of its pieces, its length; then every block's offset in the round's output
__global__ void __launch_bounds__(256) k_rle_compose(const BlkInfo *info, uint32_t m, uint32_t piece_cap, PieceInfo *pieces, unsigned long long *blk_off, uint32_t *bad_block) {
    for (uint32_t j = threadIdx.x; j < m; j += blockDim.x) {
        const BlkInfo b = info[j];
        const uint32_t np = (b.nblock + kPiece - 1) / kPiece;
        uint32_t s = 0;
        unsigned long long off = 0;
        for (uint32_t q = 0; q < np; q++) {
            PieceInfo &P = pieces[(uint64_t)j * piece_cap + q];
            P.entry = (uint8_t)s;
            P.off = (uint32_t)off;
            off += P.len[s];
            s = P.exit[s];
        }
        if (s == 4) atomicMin(bad_block, j);
        blk_off[j + 1] = off;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        blk_off[0] = 0;
        for (uint32_t j = 0; j < m; j++) blk_off[j + 1] += blk_off[j];
    }
}

__device__ uint32_t gf_mul(uint32_t a, uint32_t b) {  // a * b mod P, MSB-first
    uint32_t r = 0;
    for (int i = 31; i >= 0; i--) {
        r = (r & 0x80000000u) ? (r << 1) ^ kPoly : (r << 1);
        if ((b >> i) & 1) r ^= a;
    }
    return r;
}
__device__ uint32_t gf_shift(uint32_t v, uint64_t bytes) {  // v * x^(8 * bytes) mod P
    uint32_t sq = 0x100u;  // x^8
    while (bytes) {
        if (bytes & 1) v = gf_mul(v, sq);
        sq = gf_mul(sq, sq);
        bytes >>= 1;
    }
    return v;
}

__global__ void __launch_bounds__(256) k_rle_write(const BlkInfo *info, uint32_t piece_cap, const PieceInfo *pieces, const unsigned long long *blk_off, uint8_t *out,
                                                   uint32_t *crc_acc) {
    __shared__ uint32_t tab[256];
    {
        uint32_t c = threadIdx.x << 24;
        for (int k = 0; k < 8; k++) c = (c & 0x80000000u) ? (c << 1) ^ kPoly : (c << 1);
        tab[threadIdx.x] = c;
    }
    __syncthreads();
    const uint32_t j = blockIdx.y, q = blockIdx.x * blockDim.x + threadIdx.x;
    const BlkInfo b = info[j];
    const uint32_t lo = q * kPiece;
    if (lo >= b.nblock) return;
    const uint32_t hi = min(lo + kPiece, b.nblock);
    const PieceInfo &P = pieces[(uint64_t)j * piece_cap + q];
    const uint64_t blk_len = blk_off[j + 1] - blk_off[j];
    uint8_t *dst = out + blk_off[j] + P.off;
    uint32_t r = P.entry, prev = lo ? b.ll[lo - 1] : 0, crc = 0, w = 0;
    const uint8_t *in = b.ll;
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t x = in[i];
        if (r == 4) {
            for (uint32_t k = 0; k < x; k++) crc = (crc << 8) ^ tab[(crc >> 24) ^ prev];
            put_bytes(dst, w, (uint8_t)prev, x);
            w += x;
            r = 0;
        } else {
            r = (r && x == prev) ? r + 1 : 1;
            crc = (crc << 8) ^ tab[(crc >> 24) ^ x];
            dst[w++] = (uint8_t)x;
        }
        prev = x;
    }
    // this piece's share of the block CRC: its register contents shifted over the bytes behind it
    uint32_t term = gf_shift(crc, blk_len - P.off - w);
    if (q == 0) term ^= gf_shift(0xFFFFFFFFu, blk_len);
    atomicXor(&crc_acc[j], term);
}

__global__ void k_crc_check(const uint32_t *chained, const CandOut *outs, uint32_t m, const uint32_t *crc_acc, uint32_t *bad_block) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    if (~crc_acc[j] != outs[chained[j]].crc) atomicMin(bad_block, j);
}

// ---------------------------------------------------------------- host side
struct Tmp {
    int dev;
    hipStream_t st;
    void *p = nullptr;
    size_t sz = 0;
    Tmp(int d, hipStream_t s) : dev(d), st(s) {}
    Tmp(const Tmp &) = delete;
    Tmp &operator=(const Tmp &) = delete;
    ~Tmp() { release(); }
    void release() {
        if (!p) return;
        (void)hipStreamSynchronize(st);
        exg_rd::dev_pool()->give(dev, p, sz);
        p = nullptr;
    }
    bool take(size_t bytes) {
        release();
        sz = bytes ? bytes : 16;
        p = exg_rd::dev_pool()->take(dev, sz);
        return p != nullptr;
    }
    template <class T>
    T *as() const { return (T *)p; }
};

#define BZ_HIP(expr)                                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            set_error("bzip2 decode: %s failed: %s", #expr, hipGetErrorString(_e));        \
            return EXG_E_HIP;                                                               \
        }                                                                                   \
    } while (0)

uint32_t grid1(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

}  // namespace

int decode_round(Round &R, void *stream_v, uint64_t *good_bytes) {
    hipStream_t st = (hipStream_t)stream_v;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (good_bytes) *good_bytes = 0;
    R.d_out = nullptr, R.alloc = 0, R.produced = 0, R.n_blocks = 0, R.done = false;
    R.events.clear();
    R.block_end.clear();
    R.bit_end = R.bit0, R.at_header_out = R.at_header, R.level_out = R.level;
    const uint64_t nbits = R.n * 8;
    auto data_error = [&](uint32_t s, uint64_t block) {
        if (s == kErrNotBzip2) set_error("bzip2: not a bzip2 stream (bad stream header)");
        else if (s == kErrTruncated) set_error("bzip2: unexpected end of stream (compressed data ended before the end-of-stream marker)");
        else set_error("bzip2: data error in block %llu: %s", (unsigned long long)block, reason_text(s));
        return EXG_E_PARSE;
    };
    // (1) candidates
    Tmp d_count(dev, st), d_cand(dev, st), d_sorted(dev, st);
    if (!d_count.take(64)) return set_error("bzip2 decode: out of device memory"), EXG_E_HIP;
    uint32_t cap = (uint32_t)std::min<uint64_t>(1u << 20, std::max<uint64_t>(4096, R.n / 4096));
    uint32_t n_cand = 0;
    for (int pass = 0; pass < 2; pass++) {
        if (!d_cand.take((size_t)cap * 8)) return set_error("bzip2 decode: out of device memory"), EXG_E_HIP;
        BZ_HIP(hipMemsetAsync(d_count.p, 0, 4, st));
        if (R.n) k_discover<<<grid1((R.n + 3) / 4, 256), 256, 0, st>>>((const uint32_t *)R.d_comp, R.n, R.bit0, d_cand.as<unsigned long long>(), cap, d_count.as<uint32_t>());
        BZ_HIP(hipGetLastError());
        BZ_HIP(hipMemcpyAsync(&n_cand, d_count.p, 4, hipMemcpyDeviceToHost, st));
        BZ_HIP(hipStreamSynchronize(st));
        if (n_cand <= cap) break;
        cap = n_cand;
    }
    if (!d_sorted.take((size_t)std::max<uint32_t>(n_cand, 1) * 8)) return set_error("bzip2 decode: out of device memory"), EXG_E_HIP;
    if (n_cand) k_rank_sort<<<grid1(n_cand, 256), 256, 0, st>>>(d_cand.as<unsigned long long>(), d_sorted.as<unsigned long long>(), n_cand);
    BZ_HIP(hipGetLastError());
    // (2) symbols of the first candidates the round may hold (+ the end-of-stream magics among them), then the chain
    const uint32_t slot = (uint32_t)(((uint64_t)std::max(1, std::min(9, R.level)) * 100000 + 15) & ~15ull);
    const uint32_t n_dec = (uint32_t)std::min<uint64_t>(n_cand, R.max_blocks == ~0ull ? n_cand : 2 * R.max_blocks + 2);
    Tmp d_ll(dev, st), d_outs(dev, st), d_chain(dev, st), d_events(dev, st), d_res(dev, st);
    if (!d_ll.take((size_t)std::max<uint32_t>(n_dec, 1) * slot + 64) || !d_outs.take((size_t)std::max<uint32_t>(n_dec, 1) * sizeof(CandOut)) ||
        !d_chain.take((size_t)std::max<uint32_t>(n_dec, 1) * 4) || !d_events.take((size_t)std::max<uint32_t>(n_dec, 1) * 8 + 64) || !d_res.take(sizeof(ChainOut)))
        return set_error("bzip2 decode: out of device memory"), EXG_E_HIP;
    if (n_dec) k_symbols<<<n_dec, 64, 0, st>>>((const uint8_t *)R.d_comp, nbits, d_sorted.as<unsigned long long>(), n_dec, d_ll.as<uint8_t>(), slot, d_outs.as<CandOut>());
    BZ_HIP(hipGetLastError());
    const uint32_t maxb = (uint32_t)std::min<uint64_t>(R.max_blocks, 0xFFFFFFFFu);
    k_chain<<<1, 1, 0, st>>>((const uint8_t *)R.d_comp, R.n, d_sorted.as<unsigned long long>(), n_cand, n_dec, d_outs.as<CandOut>(), R.bit0, R.at_header ? 1 : 0,
                             R.first_stream ? 1 : 0, (uint32_t)R.level, slot, R.final_window ? 1 : 0, maxb, d_chain.as<uint32_t>(), d_events.as<uint32_t>(), d_res.as<ChainOut>());
    BZ_HIP(hipGetLastError());
    ChainOut res;
    BZ_HIP(hipMemcpyAsync(&res, d_res.p, sizeof res, hipMemcpyDeviceToHost, st));
    BZ_HIP(hipStreamSynchronize(st));
    std::vector<uint32_t> ev(2 * (size_t)res.n_events);
    if (res.n_events) {
        BZ_HIP(hipMemcpyAsync(ev.data(), d_events.p, ev.size() * 4, hipMemcpyDeviceToHost, st));
        BZ_HIP(hipStreamSynchronize(st));
    }
    const uint32_t m = res.n_blocks;
    d_cand.release();
    // (3) + (4) for the chained blocks
    Tmp d_info(dev, st), d_hist(dev, st), d_tt(dev, st), d_split(dev, st), d_pieces(dev, st), d_boff(dev, st), d_flags(dev, st), d_crc(dev, st);
    uint64_t total = 0;
    uint32_t bad_cycle = 0, bad_block = ~0u, run_block = ~0u;
    std::vector<unsigned long long> boff(m + 1, 0);
    if (m) {
        const uint32_t n_chunks = (slot + kChunk - 1) / kChunk, split_cap = (slot + kStride - 1) / kStride + 1, piece_cap = (slot + kPiece - 1) / kPiece;
        if (!d_info.take((size_t)m * sizeof(BlkInfo)) || !d_hist.take((size_t)m * n_chunks * 256 * 4) || !d_tt.take((size_t)m * slot * 4) ||
            !d_split.take((size_t)m * split_cap * 12) || !d_pieces.take((size_t)m * piece_cap * sizeof(PieceInfo)) || !d_boff.take((size_t)(m + 1) * 8) ||
            !d_flags.take(64) || !d_crc.take((size_t)m * 4))
            return set_error("bzip2 decode: out of device memory"), EXG_E_HIP;
        BlkInfo *info = d_info.as<BlkInfo>();
        uint32_t *flags = d_flags.as<uint32_t>();  // [0] bad mapping, [1] first block ending inside a run, [2] first bad CRC
        const uint32_t init[4] = {0, ~0u, ~0u, 0};
        BZ_HIP(hipMemcpyAsync(flags, init, sizeof init, hipMemcpyHostToDevice, st));
        BZ_HIP(hipMemsetAsync(d_crc.p, 0, (size_t)m * 4, st));
        k_gather<<<grid1(m, 256), 256, 0, st>>>(d_chain.as<uint32_t>(), d_outs.as<CandOut>(), d_ll.as<uint8_t>(), slot, m, info);
        k_hist<<<dim3(n_chunks, m), 256, 0, st>>>(info, n_chunks, d_hist.as<uint32_t>());
        k_hist_prefix<<<m, 256, 0, st>>>(info, n_chunks, d_hist.as<uint32_t>());
        k_scatter<<<dim3(n_chunks, m), 64, 0, st>>>(info, n_chunks, d_hist.as<uint32_t>(), d_tt.as<uint32_t>(), slot);
        uint32_t *s_len = d_split.as<uint32_t>(), *s_next = s_len + (size_t)m * split_cap, *s_off = s_next + (size_t)m * split_cap;
        k_walk_len<<<dim3(grid1(split_cap, 256), m), 256, 0, st>>>(info, d_tt.as<uint32_t>(), slot, split_cap, s_len, s_next, s_off, flags);
        k_walk_order<<<grid1(m, 64), 64, 0, st>>>(info, m, split_cap, s_len, s_next, s_off, flags);
        k_walk_write<<<dim3(grid1(split_cap, 256), m), 256, 0, st>>>(info, d_tt.as<uint32_t>(), slot, split_cap, s_off);
        k_repeat<<<dim3(16, m), 256, 0, st>>>(info);
        k_rle_size<<<dim3(grid1(piece_cap, 64), m), 64, 0, st>>>(info, piece_cap, d_pieces.as<PieceInfo>());
        k_rle_compose<<<1, 256, 0, st>>>(info, m, piece_cap, d_pieces.as<PieceInfo>(), d_boff.as<unsigned long long>(), flags + 1);
        BZ_HIP(hipGetLastError());
        BZ_HIP(hipMemcpyAsync(boff.data(), d_boff.p, (size_t)(m + 1) * 8, hipMemcpyDeviceToHost, st));
        uint32_t fl[2];
        BZ_HIP(hipMemcpyAsync(fl, flags, 8, hipMemcpyDeviceToHost, st));
        BZ_HIP(hipStreamSynchronize(st));
        d_tt.release();  // (the bytes are in the blocks' columns now)
        bad_cycle = fl[0];
        run_block = bad_block = fl[1];
        total = boff[m];
    }
    R.alloc = (size_t)(R.front_reserve + total + 64);
    R.d_out = exg_rd::dev_pool()->take(dev, R.alloc);
    if (!R.d_out) return set_error("bzip2 decode: out of device memory for %llu decoded bytes", (unsigned long long)total), EXG_E_HIP;
    auto drop_out = [&] {
        (void)hipStreamSynchronize(st);
        exg_rd::dev_pool()->give(dev, R.d_out, R.alloc);
        R.d_out = nullptr, R.alloc = 0;
    };
    uint8_t *out = (uint8_t *)R.d_out + R.front_reserve;
    if (hipMemsetAsync(out + total, 0, 64, st) != hipSuccess) {
        drop_out();
        return set_error("bzip2 decode: hipMemsetAsync failed"), EXG_E_HIP;
    }
    if (m) {
        const uint32_t piece_cap = (slot + kPiece - 1) / kPiece;
        k_rle_write<<<dim3(grid1(piece_cap, 256), m), 256, 0, st>>>(d_info.as<BlkInfo>(), piece_cap, d_pieces.as<PieceInfo>(), d_boff.as<unsigned long long>(), out,
                                                                     d_crc.as<uint32_t>());
        k_crc_check<<<grid1(m, 256), 256, 0, st>>>(d_chain.as<uint32_t>(), d_outs.as<CandOut>(), m, d_crc.as<uint32_t>(), d_flags.as<uint32_t>() + 2);
        uint32_t fc = ~0u;
        hipError_t he = hipGetLastError();
        if (he == hipSuccess) he = hipMemcpyAsync(&fc, d_flags.as<uint32_t>() + 2, 4, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he != hipSuccess) {
            drop_out();
            return set_error("bzip2 decode: %s", hipGetErrorString(he)), EXG_E_HIP;
        }
        if (fc != ~0u && (bad_block == ~0u || fc < bad_block)) bad_block = fc;
    } else if (hipStreamSynchronize(st) != hipSuccess) {
        drop_out();
        return set_error("bzip2 decode: hipStreamSynchronize failed"), EXG_E_HIP;
    }
    // blocks in order: an inconsistent mapping, a run cut by the block's end or a CRC mismatch stops the round there
    uint32_t good = m;
    uint32_t why = kOk;
    if (bad_cycle) good = 0, why = kErrCycle;  // (not attributed to a block: the round's rows are all withheld)
    if (bad_block != ~0u && bad_block < good) good = bad_block, why = bad_block == run_block ? kErrRunAtEnd : kErrBlockCrc;
    R.n_blocks = good;
    R.produced = total;
    for (uint32_t j = 0; j < good; j++) R.block_end.push_back(boff[j + 1]);
    for (uint32_t e = 0, b = 0; e < res.n_events; e++) {
        if (ev[2 * e] == 0 && b++ >= good) break;
        R.events.push_back({ev[2 * e], ev[2 * e + 1]});
    }
    if (why) {
        if (good_bytes) *good_bytes = boff[good];
        return data_error(why, R.blocks_before + good);
    }
    if (res.status) {
        if (good_bytes) *good_bytes = total;
        return data_error(res.status, R.blocks_before + res.err_block);
    }
    R.bit_end = res.bit_end;
    R.at_header_out = res.at_header != 0;
    R.level_out = (int)res.level;
    R.done = res.done != 0;
    return EXG_OK;
}

}  // namespace bz2
}  // namespace exg

// ---------------------------------------------------------------- C-ABI: a whole stream (every concatenated stream)
extern "C" int exg_bzip2_decode(const void *d_comp, uint64_t n, void **d_out, uint64_t *produced, void *stream) {
    using namespace exg::bz2;
    if ((!d_comp && n) || !d_out || !produced) {
        exg::set_error("exg_bzip2_decode: null argument");
        return EXG_E_INVALID_ARG;
    }
    *d_out = nullptr;
    *produced = 0;
    hipStream_t st = (hipStream_t)stream;
    int dev = 0;
    (void)hipGetDevice(&dev);
    // the bytes in a padded, aligned buffer of the pool (the kernels read 16-byte words ahead)
    const size_t cap = (size_t)n + 128;
    void *buf = exg_rd::dev_pool()->take(dev, cap);
    if (!buf) {
        exg::set_error("exg_bzip2_decode: out of device memory");
        return EXG_E_HIP;
    }
    std::vector<std::pair<void *, size_t>> parts;  // rounds' outputs (more than one: the whole decode is concatenated)
    std::vector<uint64_t> part_len;
    auto cleanup = [&] {
        (void)hipStreamSynchronize(st);
        exg_rd::dev_pool()->give(dev, buf, cap);
        for (auto &p : parts) exg_rd::dev_pool()->give(dev, p.first, p.second);
        parts.clear();
    };
    hipError_t he = n ? hipMemcpyAsync(buf, d_comp, (size_t)n, hipMemcpyDeviceToDevice, st) : hipSuccess;
    if (he == hipSuccess) he = hipMemsetAsync((uint8_t *)buf + n, 0, 128, st);
    uint8_t head[4] = {0, 0, 0, 0};
    if (he == hipSuccess && n >= 4) he = hipMemcpyAsync(head, d_comp, 4, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) {
        cleanup();
        exg::set_error("exg_bzip2_decode: %s", hipGetErrorString(he));
        return EXG_E_HIP;
    }
    if (n == 0) {  // (bz2.decompress(b"") is b"")
        cleanup();
        void *p = exg_rd::dev_pool()->take(dev, 64);
        if (!p || hipMemsetAsync(p, 0, 64, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            exg::set_error("exg_bzip2_decode: out of device memory");
            return EXG_E_HIP;
        }
        *d_out = p;
        return EXG_OK;
    }
    Round R;
    R.d_comp = buf;
    R.n = n;
    R.level = (n >= 4 && head[3] >= '1' && head[3] <= '9') ? head[3] - '0' : 9;
    // rounds of at most ~2 GB of BWT input (the LF vectors: 4 bytes per byte)
    const uint64_t max_blocks = std::max<uint64_t>(1, (2ull << 30) / ((uint64_t)R.level * 100000));
    uint32_t scrc = 0;
    uint64_t blocks = 0;
    for (;;) {
        R.max_blocks = max_blocks;
        R.blocks_before = blocks;
        int rc = decode_round(R, st, nullptr);
        if (rc) {
            if (R.d_out) exg_rd::dev_pool()->give(dev, R.d_out, R.alloc);
            cleanup();
            return rc;
        }
        for (const Round::Event &e : R.events) {
            if (e.kind == 0) {
                scrc = fold_crc(scrc, e.value);
            } else {
                if (e.value != scrc) {
                    exg_rd::dev_pool()->give(dev, R.d_out, R.alloc);
                    cleanup();
                    exg::set_error("bzip2: data error: stream CRC mismatch (combined CRC %08x, stored %08x)", scrc, e.value);
                    return EXG_E_PARSE;
                }
                scrc = 0;
            }
        }
        blocks += R.n_blocks;
        parts.push_back({R.d_out, R.alloc});
        part_len.push_back(R.produced);
        if (R.done) break;
        if (R.n_blocks == 0 && R.bit_end == R.bit0 && R.at_header_out == R.at_header) {  // (no progress: cannot happen on a whole stream)
            cleanup();
            exg::set_error("bzip2: unexpected end of stream");
            return EXG_E_PARSE;
        }
        R.bit0 = R.bit_end;
        R.at_header = R.at_header_out;
        R.first_stream = false;
        R.level = R.level_out;
    }
    if (parts.size() == 1) {
        *d_out = parts[0].first;
        *produced = part_len[0];
        parts.clear();
        cleanup();
        return EXG_OK;
    }
    uint64_t total = 0;
    for (uint64_t l : part_len) total += l;
    void *o = exg_rd::dev_pool()->take(dev, (size_t)total + 64);
    he = o ? hipSuccess : hipErrorOutOfMemory;
    uint64_t at = 0;
    for (size_t i = 0; i < parts.size() && he == hipSuccess; i++) {
        if (part_len[i]) he = hipMemcpyAsync((uint8_t *)o + at, parts[i].first, (size_t)part_len[i], hipMemcpyDeviceToDevice, st);
        at += part_len[i];
    }
    if (he == hipSuccess) he = hipMemsetAsync((uint8_t *)o + total, 0, 64, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    cleanup();
    if (he != hipSuccess) {
        if (o) exg_rd::dev_pool()->give(dev, o, (size_t)total + 64);
        exg::set_error("exg_bzip2_decode: %s", hipGetErrorString(he));
        return EXG_E_HIP;
    }
    *d_out = o;
    *produced = total;
    return EXG_OK;
}
