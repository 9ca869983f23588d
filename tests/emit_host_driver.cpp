// emit_host_driver.cpp — the host decisions of the Arrow / nested emitter that make no HIP call, under ASan + UBSan
// (tests/test_emit_host.py): the region layout of the nested VCF builder, its zero-skip decision, the key table the kernels
// probe (exg_nested_layout.hpp), and the Arrow C data export of a batch's columns (exg_arrow_export.hpp).  Links no HIP library.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "exg_arrow_export.hpp"
#include "exg_nested_layout.hpp"

using namespace exg_rd;

static int n_checks = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        n_checks++;                                                             \
        if (!(cond)) {                                                          \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                            \
        }                                                                       \
    } while (0)

typedef std::vector<std::pair<size_t, size_t>> Ranges;

// ---- Layout, by hand-computed values -----------------------------------------------------------------------------------------
static void test_layout() {
    size_t a = 7, b = 7, c = 7;
    Layout L;
    L.add(1, &a, 100);
    L.add(0, &b, 8);
    L.add(2, &c, 1);
    for (int turn = 0; turn < 2; turn++) {  // (a second finish(), as in the retry turn: the same offsets)
        CHECK(L.finish() == 256);
        CHECK(b == 0 && L.end[0] == 64 && a == 64 && L.end[1] == 192 && c == 192 && L.end[2] == 256);
    }
    CHECK(L.ranges({}) == (Ranges{{0, 256}}));
    CHECK(L.ranges({&a}) == (Ranges{{0, 64}, {192, 64}}));
    CHECK(L.ranges({&b, &c}) == (Ranges{{64, 128}}));
}

// ---- lay_keys over a mixed header ---------------------------------------------------------------------------------------------
static KeyDef key(const std::string &id, uint8_t type, bool is_list) {
    KeyDef k;
    k.id = id;
    k.type = type;
    k.is_list = is_list;
    return k;
}
struct Buf {
    size_t off, bytes;
    int cat;  // the category it must lie in
};
static void test_lay_keys_one(const std::vector<KeyDef> &defs, uint64_t m, uint64_t nc, const uint64_t *totals, int scalar_cat) {
    Layout L;
    std::vector<NKeyBuf> bufs;
    lay_keys(L, defs, &bufs, m, nc, totals, scalar_cat);
    const size_t size = L.finish();
    CHECK(bufs.size() == defs.size());
    std::vector<Buf> all;
    uint32_t li = 0;
    for (size_t q = 0; q < defs.size(); q++) {
        const NKeyBuf &kb = bufs[q];
        const size_t es = defs[q].type == kKeyString ? 16 : defs[q].type == kKeyFlag ? 1 : 4;
        CHECK(key_elem_size(defs[q].type) == es);
        if (!defs[q].is_list) {
            all.push_back(Buf{kb.vals, (size_t)(m * es + 16), scalar_cat});
            all.push_back(Buf{kb.valid, (size_t)((m + 63) / 64 * 8), scalar_cat});
        } else {
            CHECK(kb.total == totals[li]);  // (the list keys take their totals in header order)
            li++;
            all.push_back(Buf{kb.entries, (size_t)(m * 16 + 16), 1});
            all.push_back(Buf{kb.bases, (size_t)((nc + 1) * 8), 0});
            all.push_back(Buf{kb.valid, (size_t)((m + 63) / 64 * 8), scalar_cat});
            all.push_back(Buf{kb.child_vals, (size_t)(kb.total * es + 16), 1});
            all.push_back(Buf{kb.child_valid, (size_t)((kb.total + 63) / 64 * 8), 2});
        }
    }
    for (const Buf &x : all) {
        CHECK(x.off % 64 == 0);
        const size_t lo = x.cat ? L.end[x.cat - 1] : 0;
        CHECK(x.off >= lo && x.off + x.bytes <= L.end[x.cat]);
    }
    std::sort(all.begin(), all.end(), [](const Buf &x, const Buf &y) { return x.off != y.off ? x.off < y.off : x.bytes < y.bytes; });  // (an empty buffer shares its offset with the next)
    for (size_t i = 0; i + 1 < all.size(); i++) CHECK(all[i].off + all[i].bytes <= all[i + 1].off);
    CHECK(all.empty() || all.back().off + all.back().bytes <= size);
    CHECK(L.end[0] <= L.end[1] && L.end[1] <= L.end[2] && L.end[2] == size);
}
static void test_lay_keys() {
    const std::vector<KeyDef> defs = {key("DP", kKeyInt, false), key("DB", kKeyFlag, false), key("ANN", kKeyString, false), key("AF", kKeyFloat, true),
                                      key("CSQ", kKeyString, true)};
    const uint64_t ms[] = {0, 1, 63, 64, 65}, ncs[] = {0, 1, 2}, ts[] = {0, 1, 1000};
    for (uint64_t m : ms)
        for (uint64_t nc : ncs)
            for (uint64_t t0 : ts)
                for (uint64_t t1 : ts)
                    for (int scalar_cat = 0; scalar_cat < 2; scalar_cat++) {
                        const uint64_t totals[2] = {t0, t1};
                        test_lay_keys_one(defs, m, nc, totals, scalar_cat);
                    }
}

// ---- the zero-skip decision of the mirror step -----------------------------------------------------------------------------
static void test_zero_skip() {
    const std::vector<KeyDef> defs = {key("ABSENT", kKeyInt, false), key("EMPTY", kKeyFloat, true), key("HERE", kKeyString, false), key("FULL", kKeyInt, true)};
    const uint64_t totals[2] = {0, 5};
    Layout L;
    std::vector<NKeyBuf> bufs;
    lay_keys(L, defs, &bufs, 100, 2, totals, 1);
    L.finish();
    const uint32_t h_any[4] = {0, 9, 3, 0};  // (a list key is judged by its total, not by its word)
    std::vector<const size_t *> skip = zero_skip(defs, &bufs, h_any);
    std::vector<const size_t *> want = {&bufs[0].vals, &bufs[0].valid, &bufs[1].entries, &bufs[1].child_vals, &bufs[1].child_valid, &bufs[1].valid};
    std::sort(skip.begin(), skip.end());
    std::sort(want.begin(), want.end());
    CHECK(skip == want);  // (not EMPTY's bases, nothing of the keys that are present)
    CHECK(bufs[0].zero && bufs[1].zero && !bufs[2].zero && !bufs[3].zero);
    // what travels: everything but the skipped buffers, and EMPTY's bases among it
    size_t travelling = 0;
    bool bases_travel = false;
    for (const auto &rg : L.ranges(skip)) {
        travelling += rg.second;
        bases_travel = bases_travel || (bufs[1].bases >= rg.first && bufs[1].bases < rg.first + rg.second);
    }
    // (ABSENT: 100 x 4 + 16 -> 448 and 16 -> 64 bytes; EMPTY: entries 1616 -> 1664, child values 16 -> 64, child validity 0, validity 64)
    CHECK(bases_travel && travelling == L.end[2] - (448 + 64 + 1664 + 64 + 0 + 64));
}

// ---- the key table ---------------------------------------------------------------------------------------------------------
// the kernels' lookup: from key_slot(hash, mask) in linear steps.  -1: ended at an empty slot; -2: no empty slot met
static int probe(const KeyTable &t, const std::string &name) {
    uint32_t h = vn::kKeyHashSeed;
    for (unsigned char c : name) h = vn::key_hash_step(h, c);
    const uint32_t mask = (uint32_t)t.slots.size() - 1;
    uint32_t sl = vn::key_slot(h, mask);
    for (size_t i = 0; i < t.slots.size(); i++, sl = (sl + 1) & mask) {
        if (!t.slots[sl]) return -1;
        const vn::Key &k = t.keys[t.slots[sl] - 1];
        if (k.hash == h && k.name_len == name.size() && memcmp(t.names.data() + k.name_off, name.data(), name.size()) == 0) return (int)t.slots[sl] - 1;
    }
    return -2;
}
static void test_key_table() {
    const size_t counts[] = {0, 1, 2, 33, 1000};
    for (size_t nk : counts) {
        std::vector<KeyDef> defs;
        std::string all_names;
        for (size_t k = 0; k < nk; k++) {
            defs.push_back(key((k % 5 == 0 ? "K" : "LONGER_KEY_") + std::to_string(k * 7919), (uint8_t)(k % 4), k % 3 == 1));
            all_names += defs.back().id;
        }
        KeyTable t;
        CHECK(build_key_table(defs, &t));
        const size_t ns = t.slots.size();
        CHECK(ns >= 2 && ns >= 2 * nk && (ns & (ns - 1)) == 0);
        CHECK(t.keys.size() == nk && t.names == all_names);
        int32_t lists = 0;
        for (size_t k = 0; k < nk; k++) {
            CHECK(probe(t, defs[k].id) == (int)k);
            CHECK(std::string(t.names, t.keys[k].name_off, t.keys[k].name_len) == defs[k].id);
            CHECK(t.keys[k].type == defs[k].type && t.keys[k].is_list == (defs[k].is_list ? 1 : 0));
            CHECK(t.keys[k].list_idx == (defs[k].is_list ? lists++ : -1));
        }
        CHECK(t.n_lists == (uint32_t)lists);
        CHECK(probe(t, "NOT_IN_THE_HEADER") == -1 && probe(t, "") == -1 && probe(t, "K") == -1);
        CHECK((size_t)std::count(t.slots.begin(), t.slots.end(), 0u) == ns - nk);
    }
    KeyTable t;
    CHECK(!build_key_table({key(std::string(65536, 'x'), kKeyInt, false)}, &t));
    CHECK(build_key_table({key(std::string(65535, 'x'), kKeyInt, false)}, &t));
    CHECK(t.keys[0].name_len == 65535 && probe(t, std::string(65535, 'x')) == 0);
}

// ---- the value types, once --------------------------------------------------------------------------------------------------
static void test_key_types() {
    CHECK(std::string(key_type_info(kKeyFlag).arrow) == "b" && key_type_info(kKeyFlag).exg_type == EXG_TYPE_BOOLEAN && key_type_info(kKeyFlag).elem == 1);
    CHECK(std::string(key_type_info(kKeyInt).arrow) == "i" && key_type_info(kKeyInt).exg_type == EXG_TYPE_INTEGER && key_type_info(kKeyInt).elem == 4);
    CHECK(std::string(key_type_info(kKeyFloat).arrow) == "f" && key_type_info(kKeyFloat).exg_type == EXG_TYPE_FLOAT && key_type_info(kKeyFloat).elem == 4);
    CHECK(std::string(key_type_info(kKeyString).arrow) == "u" && key_type_info(kKeyString).exg_type == EXG_TYPE_VARCHAR && key_type_info(kKeyString).elem == 16);
}

// ---- export: an AColumn tree built by hand on heap buffers, B = 64, n = 150 ----------------------------------------------
struct Heap {  // what the exported arrays keep alive
    std::vector<std::vector<uint8_t>> blocks;
    const uint8_t *take(size_t bytes) {
        blocks.emplace_back(bytes ? bytes : 1, (uint8_t)0xA5);
        return blocks.back().data();
    }
};
static int heap_deleted = 0;
static AColumn col(AColumn::Kind kind, int64_t length, const uint8_t *validity, const uint8_t *offsets, const uint8_t *data, int elem = 0) {
    AColumn c;
    c.kind = kind;
    c.length = length;
    c.validity = validity;
    c.offsets = offsets;
    c.data = data;
    c.elem_size = elem;
    return c;
}
static const uint8_t *buf(const ArrowArray *a, int i) { return (const uint8_t *)a->buffers[i]; }
static void check_shape(const ArrowArray *a, int64_t length, int64_t n_buffers, int64_t null_count, int64_t n_children) {
    CHECK(a->length == length && a->n_buffers == n_buffers && a->null_count == null_count && a->n_children == n_children && a->offset == 0);
    CHECK(a->release != nullptr && a->dictionary == nullptr);
}
static void test_export() {
    const uint64_t B = 64, n = 150, n_chunks = 3;
    Heap *heap = new Heap();
    std::shared_ptr<void> keep(heap, [](void *p) {
        heap_deleted++;
        delete (Heap *)p;
    });
    const size_t bits = (n + 63) / 64 * 8;
    AColumn root;
    root.kind = AColumn::kStruct;
    std::vector<AColumn> &cols = root.children;
    cols.push_back(col(AColumn::kUtf8Top, n, heap->take(bits), heap->take(n_chunks * (B + 1) * 4), heap->take(300)));
    cols[0].chunk_base = {0, 100, 250, 300};
    cols.push_back(col(AColumn::kPrim, n, nullptr, nullptr, heap->take(n * 8), 8));
    cols.push_back(col(AColumn::kBool, n, heap->take(bits), nullptr, heap->take(bits)));
    cols.push_back(col(AColumn::kList, n, nullptr, heap->take((n + 1) * 4), nullptr));
    cols[3].children.push_back(col(AColumn::kUtf8Abs, 400, nullptr, heap->take(401 * 4), heap->take(999)));
    cols.push_back(col(AColumn::kStruct, n, nullptr, nullptr, nullptr));
    cols[4].children.push_back(col(AColumn::kPrim, n, heap->take(bits), nullptr, heap->take(n * 4), 4));
    cols[4].children.push_back(col(AColumn::kList, n, heap->take(bits), heap->take((n + 1) * 4), nullptr));
    cols[4].children[1].children.push_back(col(AColumn::kPrim, 77, heap->take(16), nullptr, heap->take(77 * 4), 4));
    cols.push_back(col(AColumn::kList, n, nullptr, heap->take((n + 1) * 4), nullptr));
    cols[5].children.push_back(col(AColumn::kStruct, 33, nullptr, nullptr, nullptr));
    cols[5].children[0].children.push_back(col(AColumn::kPrim, 33, nullptr, nullptr, heap->take(33 * 4), 4));

    ArrowArray arr[3];
    for (uint64_t k = 0; k < 3; k++) {
        const uint64_t row0 = k * B, len = std::min<uint64_t>(B, n - row0);
        export_rows(root, row0, len, B, keep, &arr[k]);
        const ArrowArray *a = &arr[k];
        check_shape(a, (int64_t)len, 1, 0, 6);
        CHECK(buf(a, 0) == nullptr);
        const ArrowArray *c0 = a->children[0], *c1 = a->children[1], *c2 = a->children[2], *c3 = a->children[3], *c4 = a->children[4], *c5 = a->children[5];
        check_shape(c0, (int64_t)len, 3, -1, 0);  // kUtf8Top: the chunk's own offsets and where its bytes begin
        CHECK(buf(c0, 0) == cols[0].validity + row0 / 8 && buf(c0, 1) == cols[0].offsets + k * (B + 1) * 4 && buf(c0, 2) == cols[0].data + cols[0].chunk_base[k]);
        check_shape(c1, (int64_t)len, 2, 0, 0);  // kPrim
        CHECK(buf(c1, 0) == nullptr && buf(c1, 1) == cols[1].data + row0 * 8);
        check_shape(c2, (int64_t)len, 2, -1, 0);  // kBool
        CHECK(buf(c2, 0) == cols[2].validity + row0 / 8 && buf(c2, 1) == cols[2].data + row0 / 8);
        check_shape(c3, (int64_t)len, 2, 0, 1);  // kList of kUtf8Abs: the child is the whole array
        CHECK(buf(c3, 0) == nullptr && buf(c3, 1) == cols[3].offsets + row0 * 4);
        check_shape(c3->children[0], 400, 3, 0, 0);
        CHECK(buf(c3->children[0], 1) == cols[3].children[0].offsets && buf(c3->children[0], 2) == cols[3].children[0].data);
        check_shape(c4, (int64_t)len, 1, 0, 2);  // kStruct: its children are sliced like rows
        CHECK(buf(c4, 0) == nullptr);
        const AColumn &s0 = cols[4].children[0], &s1 = cols[4].children[1];
        check_shape(c4->children[0], (int64_t)len, 2, -1, 0);
        CHECK(buf(c4->children[0], 0) == s0.validity + row0 / 8 && buf(c4->children[0], 1) == s0.data + row0 * 4);
        check_shape(c4->children[1], (int64_t)len, 2, -1, 1);
        CHECK(buf(c4->children[1], 0) == s1.validity + row0 / 8 && buf(c4->children[1], 1) == s1.offsets + row0 * 4);
        check_shape(c4->children[1]->children[0], 77, 2, -1, 0);
        CHECK(buf(c4->children[1]->children[0], 0) == s1.children[0].validity && buf(c4->children[1]->children[0], 1) == s1.children[0].data);
        check_shape(c5, (int64_t)len, 2, 0, 1);  // kList of kStruct: the child struct is not sliced, nor what is in it
        CHECK(buf(c5, 1) == cols[5].offsets + row0 * 4);
        check_shape(c5->children[0], 33, 1, 0, 1);
        check_shape(c5->children[0]->children[0], 33, 2, 0, 0);
        CHECK(buf(c5->children[0]->children[0], 1) == cols[5].children[0].children[0].data);
    }
    // the schema of such a stream
    Field f_root, f_list, f_item;
    f_root.format = "+s", f_root.nullable = false;
    f_list.name = "alt", f_list.format = "+l";
    f_item.name = "item", f_item.format = "u";
    f_list.children.push_back(f_item);
    f_root.children = {f_list, f_item};
    ArrowSchema schema;
    export_field(f_root, &schema);
    CHECK(std::string(schema.format) == "+s" && schema.flags == 0 && schema.n_children == 2 && schema.release != nullptr);
    CHECK(std::string(schema.children[0]->name) == "alt" && std::string(schema.children[0]->format) == "+l" && schema.children[0]->flags == ARROW_FLAG_NULLABLE);
    CHECK(schema.children[0]->n_children == 1 && std::string(schema.children[0]->children[0]->format) == "u" && schema.children[1]->n_children == 0);
    CHECK(schema.children[1]->children == nullptr);

    // released in any order: the buffers go with the last array, once
    keep.reset();
    root = AColumn();  // (the arrays do not point into the column tree)
    void (*release_arr)(ArrowArray *) = arr[0].release;
    void (*release_sch)(ArrowSchema *) = schema.release;
    arr[1].release(&arr[1]);
    CHECK(arr[1].release == nullptr && heap_deleted == 0);
    arr[0].release(&arr[0]);
    release_sch(&schema);
    CHECK(arr[0].release == nullptr && schema.release == nullptr && heap_deleted == 0);
    arr[2].release(&arr[2]);
    CHECK(arr[2].release == nullptr && heap_deleted == 1);
    for (ArrowArray &a : arr) release_arr(&a);  // (a second call is a no-op)
    release_sch(&schema);
    release_arr(nullptr);
    CHECK(heap_deleted == 1);
}

int main() {
    test_layout();
    test_lay_keys();
    test_zero_skip();
    test_key_table();
    test_key_types();
    test_export();
    printf("emit host driver: %d checks\n", n_checks);
    return 0;
}
