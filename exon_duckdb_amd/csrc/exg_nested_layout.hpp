// exg_nested_layout.hpp — the host decisions of the nested VCF builder (exg_vcf_nested_build.cpp) that make no HIP call: what
// a key's value type means at each boundary, the table the kernels look a key's text up in, where every buffer of a column's
// region lies, and which of them stay at home because they are all zeros.  Host only and free of any HIP include: under
// ASan + UBSan in tests/emit_host_driver.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/exon_gpu.h"
#include "exg_vcf_header.hpp"
#include "exg_vcf_keys.hpp"

namespace exg_rd {
namespace vn = exg::vn;

static_assert((int)kKeyFlag == vn::kFlag && (int)kKeyInt == vn::kInt && (int)kKeyFloat == vn::kFloat && (int)kKeyString == vn::kString,
              "the header parser's value types are the emitter's");

// ---- a key's value type at the Arrow boundary, at the chunk boundary, and in the kernels' child vectors -----------------------
struct KeyTypeInfo {
    const char *arrow;  // format letter
    int exg_type;       // EXG_TYPE_*
    size_t elem;        // bytes per element of the DuckDB vector (a byte per BOOLEAN, string_t)
};
inline const KeyTypeInfo &key_type_info(uint8_t type) {
    static const KeyTypeInfo t[4] = {{"b", EXG_TYPE_BOOLEAN, 1}, {"i", EXG_TYPE_INTEGER, 4}, {"f", EXG_TYPE_FLOAT, 4}, {"u", EXG_TYPE_VARCHAR, 16}};
    return t[type <= vn::kFloat ? type : vn::kString];
}
inline size_t key_elem_size(uint8_t type) { return key_type_info(type).elem; }
inline size_t bitmap_bytes(uint64_t m) { return (size_t)((m + 63) / 64) * 8; }

// ---- the header's keys as the kernels find them (exg_vcf_keys.hpp): header order, an open-addressed table of their hashes ------
struct KeyTable {
    std::vector<vn::Key> keys;
    std::vector<uint32_t> slots;  // key index + 1, 0 = empty; a power of two, >= 2 and >= 2 x keys
    std::string names;
    uint32_t n_lists = 0;
};
// false: an id of more than 65 535 bytes (Key::name_len)
inline bool build_key_table(const std::vector<KeyDef> &defs, KeyTable *t) {
    t->keys.assign(defs.size(), vn::Key());
    t->names.clear();
    t->n_lists = 0;
    for (size_t k = 0; k < defs.size(); k++) {
        if (defs[k].id.size() > 0xFFFFu) return false;
        vn::Key &key = t->keys[k];
        key.name_off = (uint32_t)t->names.size();
        key.name_len = (uint16_t)defs[k].id.size();
        key.type = defs[k].type;
        key.is_list = defs[k].is_list ? 1 : 0;
        uint32_t h = vn::kKeyHashSeed;
        for (unsigned char c : defs[k].id) h = vn::key_hash_step(h, c);
        key.hash = h;
        key.list_idx = defs[k].is_list ? (int32_t)t->n_lists++ : -1;
        t->names += defs[k].id;
    }
    size_t n_slots = 2;
    while (n_slots < 2 * t->keys.size()) n_slots <<= 1;
    t->slots.assign(n_slots, 0u);
    for (size_t k = 0; k < t->keys.size(); k++) {  // (the header parser keeps the first definition of an ID: the names are distinct)
        uint32_t sl = vn::key_slot(t->keys[k].hash, (uint32_t)n_slots - 1);
        while (t->slots[sl]) sl = (sl + 1) & ((uint32_t)n_slots - 1);
        t->slots[sl] = (uint32_t)k + 1;
    }
    return true;
}

// ---- where the buffers of a column's region are ---------------------------------------------------------------------------
struct NKeyBuf {  // where the children of one key are in the region of its column
    size_t vals = 0, valid = 0, entries = 0, bases = 0, child_vals = 0, child_valid = 0;
    uint64_t total = 0;  // list keys: child elements of the batch
    bool zero = false;   // no element of the key is valid in this batch: its values / entries and validity did not travel (NVec::zero)
};
struct Layout {  // offsets inside a region: what must be zero first, then what the kernels write whole, then what starts as ones
    struct It {
        size_t *slot, bytes;
    };
    std::vector<It> cat[3];
    size_t end[3] = {0, 0, 0};
    void add(int c, size_t *slot, size_t bytes) { cat[c].push_back(It{slot, bytes}); }
    // the byte ranges of the region that travel: everything but the buffers whose slot is in `skip`, neighbours merged
    std::vector<std::pair<size_t, size_t>> ranges(const std::vector<const size_t *> &skip) const {
        std::vector<std::pair<size_t, size_t>> r;
        for (int c = 0; c < 3; c++)
            for (const It &it : cat[c]) {
                if (std::find(skip.begin(), skip.end(), it.slot) != skip.end()) continue;
                const size_t len = (it.bytes + 63) & ~(size_t)63;
                if (!r.empty() && r.back().first + r.back().second == *it.slot) r.back().second += len;
                else r.emplace_back(*it.slot, len);
            }
        return r;
    }
    size_t finish() {
        size_t off = 0;
        for (int c = 0; c < 3; c++) {
            for (It &it : cat[c]) {
                *it.slot = off;
                off += (it.bytes + 63) & ~(size_t)63;
            }
            end[c] = off;
        }
        return off;
    }
};
// the children of a struct's keys over m elements (rows, or samples), nc DataChunks; totals: the list keys' elements, header order
// (scalar_cat — k_rows stores every row's values and validity words of a header it takes: 1; the wave kernels store what a row /
// sample has: 0)
inline void lay_keys(Layout &lay, const std::vector<KeyDef> &defs, std::vector<NKeyBuf> *bufs, uint64_t m, uint64_t nc, const uint64_t *totals,
                     int scalar_cat) {
    bufs->assign(defs.size(), NKeyBuf());
    uint32_t li = 0;
    for (size_t q = 0; q < defs.size(); q++) {
        NKeyBuf &kb = (*bufs)[q];
        const size_t es = key_elem_size(defs[q].type);
        if (!defs[q].is_list) {
            lay.add(scalar_cat, &kb.vals, m * es + 16);
            lay.add(scalar_cat, &kb.valid, bitmap_bytes(m));
        } else {
            kb.total = totals[li++];
            lay.add(1, &kb.entries, m * 16 + 16);
            lay.add(0, &kb.bases, (nc + 1) * 8);  // (zero first: a batch without samples runs no entries kernel for the FORMAT keys)
            lay.add(scalar_cat, &kb.valid, bitmap_bytes(m));
            lay.add(1, &kb.child_vals, kb.total * es + 16);
            lay.add(2, &kb.child_valid, bitmap_bytes(kb.total));
        }
    }
}
// What is all zeros stays at home: an INFO key that no row of the batch has (h_any: a word per key, nonzero when a row has it;
// a list key: no element in the batch, NKeyBuf::total).  Sets NKeyBuf::zero and returns the slots of the buffers that do not
// travel (Layout::ranges); a list key's `bases` travel all the same
inline std::vector<const size_t *> zero_skip(const std::vector<KeyDef> &defs, std::vector<NKeyBuf> *bufs, const uint32_t *h_any) {
    std::vector<const size_t *> skip;
    for (size_t q = 0; q < defs.size(); q++) {
        NKeyBuf &kb = (*bufs)[q];
        kb.zero = defs[q].is_list ? kb.total == 0 : h_any[q] == 0;
        if (!kb.zero) continue;
        if (defs[q].is_list) skip.push_back(&kb.entries), skip.push_back(&kb.child_vals), skip.push_back(&kb.child_valid);
        else skip.push_back(&kb.vals);
        skip.push_back(&kb.valid);
    }
    return skip;
}

}  // namespace exg_rd
