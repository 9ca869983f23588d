// exg_arrow_export.hpp — the Arrow C data interface over host buffers: a schema tree (Field) and the emitted columns of a
// device batch (AColumn) become ArrowSchema / ArrowArray structs, a record batch being rows [row0, row0 + len) of the batch's
// columns.  Pointer arithmetic only — whoever owns the buffers is a shared_ptr<void> that every exported array holds.  Host
// only and free of any HIP include: under ASan + UBSan in tests/emit_host_driver.cpp.
#pragma once
#include <stdint.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/exon_gpu.h"

namespace exg_rd {

// ---- schema -------------------------------------------------------------------------------------------------------------
struct Field {
    std::string name, format;
    bool nullable = true;
    std::vector<Field> children;
};

// ---- one emitted column (host buffers of a whole device batch) ------------------------------------------------------
struct AColumn {
    enum Kind { kUtf8Top, kUtf8Abs, kPrim, kBool, kList, kStruct } kind = kPrim;
    int elem_size = 0;
    int64_t length = 0;                // elements of the batch-wide array
    const uint8_t *validity = nullptr;  // NULL: no nulls
    const uint8_t *offsets = nullptr;
    const uint8_t *data = nullptr;
    std::vector<uint64_t> chunk_base;  // kUtf8Top
    std::vector<AColumn> children;
};

// ---- ArrowSchema / ArrowArray export -------------------------------------------------------------------------------------
template <class A>
struct Exported {  // private_data of an exported ArrowSchema / ArrowArray: what its pointers point at
    std::string name, format;    // (schema)
    std::shared_ptr<void> keep;  // (array) the batch whose buffers it points into
    const void *buffers[3] = {nullptr, nullptr, nullptr};
    std::vector<A> kids;
    std::vector<A *> kid_ptrs;
    A **link_kids() {  // (once `kids` are all exported)
        for (A &k : kids) kid_ptrs.push_back(&k);
        return kid_ptrs.empty() ? nullptr : kid_ptrs.data();
    }
    static void release(A *a) {
        if (!a || !a->release) return;
        for (int64_t i = 0; i < a->n_children; i++)
            if (a->children[i]->release) a->children[i]->release(a->children[i]);
        delete (Exported *)a->private_data;
        a->release = nullptr;
    }
};
inline void export_field(const Field &f, ArrowSchema *out) {
    auto *p = new Exported<ArrowSchema>();
    p->name = f.name;
    p->format = f.format;
    p->kids.resize(f.children.size());
    for (size_t i = 0; i < f.children.size(); i++) export_field(f.children[i], &p->kids[i]);
    memset(out, 0, sizeof *out);
    out->format = p->format.c_str();
    out->name = p->name.c_str();
    out->flags = f.nullable ? ARROW_FLAG_NULLABLE : 0;
    out->n_children = (int64_t)f.children.size();
    out->children = p->link_kids();
    out->release = Exported<ArrowSchema>::release;
    out->private_data = p;
}
// rows [row0, row0 + len) of a row-space column (chunk = row0 / batch_rows), or the whole array of a child
inline void export_column(const AColumn &c, bool row_space, uint64_t row0, uint64_t len, uint64_t chunk, uint64_t batch_rows,
                          const std::shared_ptr<void> &keep, ArrowArray *out) {
    auto *p = new Exported<ArrowArray>();
    p->keep = keep;
    memset(out, 0, sizeof *out);
    const uint64_t r0 = row_space ? row0 : 0;
    out->length = (int64_t)(row_space ? len : (uint64_t)c.length);
    out->null_count = c.validity ? -1 : 0;
    out->offset = 0;
    p->buffers[0] = c.validity ? c.validity + r0 / 8 : nullptr;
    switch (c.kind) {
        case AColumn::kUtf8Top:
            out->n_buffers = 3;
            p->buffers[1] = c.offsets + chunk * (batch_rows + 1) * 4;
            p->buffers[2] = c.data + c.chunk_base[chunk];
            break;
        case AColumn::kUtf8Abs:
            out->n_buffers = 3;
            p->buffers[1] = c.offsets + r0 * 4;
            p->buffers[2] = c.data;
            break;
        case AColumn::kPrim:
            out->n_buffers = 2;
            p->buffers[1] = c.data + r0 * c.elem_size;
            break;
        case AColumn::kBool:
            out->n_buffers = 2;
            p->buffers[1] = c.data + r0 / 8;
            break;
        case AColumn::kList:
            out->n_buffers = 2;
            p->buffers[1] = c.offsets + r0 * 4;
            break;
        case AColumn::kStruct:
            out->n_buffers = 1;
            break;
    }
    const bool kids_row_space = row_space && c.kind == AColumn::kStruct;
    p->kids.resize(c.children.size());
    for (size_t i = 0; i < c.children.size(); i++) export_column(c.children[i], kids_row_space, row0, len, chunk, batch_rows, keep, &p->kids[i]);
    out->n_children = (int64_t)c.children.size();
    out->children = p->link_kids();
    out->buffers = p->buffers;
    out->release = Exported<ArrowArray>::release;
    out->private_data = p;
}
// one record batch: rows [row0, row0 + len) of a batch's columns — the children of `root`, a kStruct without nulls — as a struct array
inline void export_rows(const AColumn &root, uint64_t row0, uint64_t len, uint64_t batch_rows, const std::shared_ptr<void> &keep, ArrowArray *out) {
    export_column(root, true, row0, len, row0 / batch_rows, batch_rows, keep, out);
}

}  // namespace exg_rd
