// exg_tabix.cpp — host only: the tabix index parser, the region grammar and the chunk planner of exg_tabix.hpp, and their C entry
// exg_tabix_query.  No HIP call and no HIP include: tests/region_host_driver.cpp builds this TU with ASan / UBSan.
#include "exg_tabix.hpp"

#include <string.h>

#include <algorithm>

namespace exg {
void set_error(const char *fmt, ...);  // exg_api.hip (the driver brings its own)

namespace tabix {

namespace {
// a cursor over the index's bytes: every read is checked against what is there
struct Cursor {
    const uint8_t *d;
    uint64_t n, at = 0;
    uint64_t left() const { return n - at; }
    bool i32(int32_t *v) {
        if (left() < 4) return false;
        uint32_t u;
        memcpy(&u, d + at, 4);  // (.tbi is little-endian, like every host this builds for)
        *v = (int32_t)u;
        at += 4;
        return true;
    }
    bool u64(uint64_t *v) {
        if (left() < 8) return false;
        memcpy(v, d + at, 8);
        at += 8;
        return true;
    }
};
bool bad(std::string *err, const std::string &what) {
    *err = "not a usable tabix index: " + what;
    return false;
}
}  // namespace

bool parse_index(const uint8_t *d, uint64_t n, Index *out, std::string *err) {
    *out = Index();
    Cursor c{d, n};
    if (n < 4 || memcmp(d, "TBI\1", 4) != 0) return bad(err, "the magic is not TBI\\1");
    c.at = 4;
    int32_t n_ref = 0, l_nm = 0;
    if (!c.i32(&n_ref) || !c.i32(&out->format) || !c.i32(&out->col_seq) || !c.i32(&out->col_beg) || !c.i32(&out->col_end) || !c.i32(&out->meta) ||
        !c.i32(&out->skip) || !c.i32(&l_nm))
        return bad(err, "truncated in its header");
    if (out->format != 2) return bad(err, "its format is " + std::to_string(out->format) + ", not 2 (VCF)");
    if (n_ref < 0 || l_nm < 0 || (uint64_t)l_nm > c.left()) return bad(err, "the names (" + std::to_string(l_nm) + " bytes) do not fit the bytes that are there");
    // every reference takes a name of one byte at least, and two counts
    if ((uint64_t)n_ref > (uint64_t)l_nm || (uint64_t)n_ref > (c.left() - (uint64_t)l_nm) / 8)
        return bad(err, std::to_string(n_ref) + " references do not fit the bytes that are there");
    out->refs.resize((size_t)n_ref);
    {
        const uint8_t *p = d + c.at, *end = p + l_nm;
        for (int32_t i = 0; i < n_ref; i++) {
            const void *nul = p < end ? memchr(p, 0, (size_t)(end - p)) : nullptr;
            if (!nul) return bad(err, "name " + std::to_string(i) + " does not end inside the names");
            out->refs[(size_t)i].name.assign((const char *)p, (size_t)((const uint8_t *)nul - p));
            p = (const uint8_t *)nul + 1;
        }
        if (p != end) return bad(err, "the names hold more than " + std::to_string(n_ref) + " strings");
        c.at += (uint64_t)l_nm;
    }
    for (int32_t i = 0; i < n_ref; i++) {
        Reference &ref = out->refs[(size_t)i];
        int32_t n_bin = 0;
        if (!c.i32(&n_bin) || n_bin < 0 || (uint64_t)n_bin > c.left() / 8) return bad(err, "the bins of reference " + std::to_string(i) + " do not fit the bytes that are there");
        ref.bins.reserve((size_t)n_bin);
        for (int32_t b = 0; b < n_bin; b++) {
            int32_t id = 0, n_chunk = 0;
            if (!c.i32(&id) || !c.i32(&n_chunk) || n_chunk < 0 || (uint64_t)n_chunk > c.left() / 16)
                return bad(err, "the chunks of bin " + std::to_string(b) + " of reference " + std::to_string(i) + " do not fit the bytes that are there");
            ref.bins.push_back(Bin{(uint32_t)id, ref.chunks.size(), (uint64_t)n_chunk});
            for (int32_t k = 0; k < n_chunk; k++) {
                exg_virtual_chunk ch;
                if (!c.u64(&ch.begin) || !c.u64(&ch.end)) return bad(err, "truncated in a chunk");
                ref.chunks.push_back(ch);
            }
        }
        int32_t n_intv = 0;
        if (!c.i32(&n_intv) || n_intv < 0 || (uint64_t)n_intv > c.left() / 8)
            return bad(err, "the linear index of reference " + std::to_string(i) + " does not fit the bytes that are there");
        ref.ioff.resize((size_t)n_intv);
        for (int32_t k = 0; k < n_intv; k++)
            if (!c.u64(&ref.ioff[(size_t)k])) return bad(err, "truncated in a linear index");
    }
    if (c.left() == 8) {
        out->has_no_coor = true;
        (void)c.u64(&out->n_no_coor);
    } else if (c.left() != 0) {
        return bad(err, std::to_string(c.left()) + " bytes behind the last reference (0, or the 8 of n_no_coor)");
    }
    return true;
}

// `start` or `start-end`: digits only, at most 18 of them each
static bool parse_interval(const std::string &s, int64_t *start, int64_t *end) {
    auto number = [](const std::string &t, int64_t *v) {
        if (t.empty() || t.size() > 18) return false;
        int64_t x = 0;
        for (char ch : t) {
            if (ch < '0' || ch > '9') return false;
            x = x * 10 + (ch - '0');
        }
        *v = x;
        return true;
    };
    const size_t dash = s.find('-');
    *end = kUnbounded;
    if (!number(s.substr(0, dash), start) || *start < 1) return false;
    if (dash == std::string::npos) return true;
    return number(s.substr(dash + 1), end) && *end >= *start;
}

bool parse_region(const Index &idx, const std::string &text, Region *out, std::string *err) {
    auto find = [&](const std::string &name, uint32_t *id) {
        for (size_t i = 0; i < idx.refs.size(); i++)
            if (idx.refs[i].name == name) return *id = (uint32_t)i, true;
        return false;
    };
    *out = Region();
    if (text.empty()) {
        *err = "invalid region '': it is empty";
        return false;
    }
    out->name = text;
    if (find(text, &out->ref_id)) return true;  // G1
    const size_t colon = text.rfind(':');
    int64_t s = 1, e = kUnbounded;
    if (colon != std::string::npos && parse_interval(text.substr(colon + 1), &s, &e)) {  // G2
        out->name = text.substr(0, colon);
        out->start = s, out->end = e;
        if (find(out->name, &out->ref_id)) return true;
    }
    // G3 / G5
    *err = "invalid region '" + text + "': the index holds no reference sequence named '" + out->name + "'";
    return false;
}

void reg2bins(int64_t beg, int64_t end, std::vector<uint32_t> *out) {
    out->clear();
    out->push_back(0);
    end--;
    static const struct {
        uint32_t first;
        int shift;
    } level[5] = {{1, 26}, {9, 23}, {73, 20}, {585, 17}, {4681, 14}};
    for (const auto &l : level)
        for (int64_t k = l.first + (beg >> l.shift); k <= l.first + (end >> l.shift); k++) out->push_back((uint32_t)k);
}

void plan(const Index &idx, const Region &region, std::vector<exg_virtual_chunk> *out) {
    out->clear();
    const Reference &ref = idx.refs[region.ref_id];
    const int64_t beg = std::min<int64_t>(region.start - 1, kMaxPos - 1);                    // P1
    const int64_t end = std::max<int64_t>(std::min<int64_t>(region.end, kMaxPos), beg + 1);  // (end >= start: never empty)
    std::vector<uint32_t> bins;
    reg2bins(beg, end, &bins);
    std::sort(bins.begin(), bins.end());
    const uint64_t min_off = ref.ioff.empty() ? 0 : ref.ioff[(size_t)std::min<uint64_t>((uint64_t)(beg >> 14), ref.ioff.size() - 1)];  // P3
    for (const Bin &b : ref.bins) {
        if (b.id == kPseudoBin || !std::binary_search(bins.begin(), bins.end(), b.id)) continue;  // P2
        for (uint64_t k = 0; k < b.n_chunks; k++) {
            const exg_virtual_chunk &ch = ref.chunks[(size_t)(b.first_chunk + k)];
            if (ch.end > min_off) out->push_back(ch);  // P4
        }
    }
    std::sort(out->begin(), out->end(), [](const exg_virtual_chunk &a, const exg_virtual_chunk &b) { return a.begin != b.begin ? a.begin < b.begin : a.end < b.end; });  // P5
    size_t w = 0;
    for (size_t i = 0; i < out->size(); i++) {  // P6
        if (w && (*out)[i].begin <= (*out)[w - 1].end) (*out)[w - 1].end = std::max((*out)[w - 1].end, (*out)[i].end);
        else (*out)[w++] = (*out)[i];
    }
    out->resize(w);
}

}  // namespace tabix
}  // namespace exg

extern "C" int exg_tabix_query(const uint8_t *index_bytes, uint64_t n, const char *region, exg_virtual_chunk *out, uint64_t cap, uint64_t *n_chunks,
                               exg_region *resolved) {
    namespace tb = exg::tabix;
    if (!index_bytes || !region || !n_chunks || (cap && !out)) {
        exg::set_error("exg_tabix_query: null argument");
        return EXG_E_INVALID_ARG;
    }
    *n_chunks = 0;
    try {  // (extern "C": nothing may leave it)
        tb::Index idx;
        std::string err;
        if (!tb::parse_index(index_bytes, n, &idx, &err)) {
            exg::set_error("exg_tabix_query: %s", err.c_str());
            return EXG_E_PARSE;
        }
        tb::Region reg;
        if (!tb::parse_region(idx, region, &reg, &err)) {
            exg::set_error("exg_tabix_query: %s", err.c_str());
            return EXG_E_INVALID_ARG;
        }
        if (reg.name.size() >= sizeof resolved->name) {
            exg::set_error("exg_tabix_query: the reference name of region '%s' is longer than %zu bytes", region, sizeof resolved->name - 1);
            return EXG_E_INVALID_ARG;
        }
        std::vector<exg_virtual_chunk> chunks;
        tb::plan(idx, reg, &chunks);
        if (resolved) {
            memset(resolved, 0, sizeof *resolved);
            resolved->start = reg.start, resolved->end = reg.end;
            resolved->ref_id = reg.ref_id;
            resolved->name_len = (uint32_t)reg.name.size();
            memcpy(resolved->name, reg.name.data(), reg.name.size());
        }
        *n_chunks = chunks.size();
        if (chunks.size() > cap) {
            if (!out && !cap) return EXG_OK;  // the counting call
            exg::set_error("exg_tabix_query: %llu chunks, room for %llu", (unsigned long long)chunks.size(), (unsigned long long)cap);
            return EXG_E_CAPACITY;
        }
        if (!chunks.empty()) memcpy(out, chunks.data(), chunks.size() * sizeof chunks[0]);
        return EXG_OK;
    } catch (const std::exception &e) {
        exg::set_error("exg_tabix_query: %s", e.what());
        return EXG_E_NOMEM;
    }
}
