// exg_vcf_keys.hpp — what the host's key table (exg_nested_layout.hpp) and the nested kernels (exg_vcf_nested.hpp) must agree
// on: a declared key, its value types, the hash of its text and the first slot of its probe.  No HIP include: the host half
// is compiled by a plain C++ compiler in tests/emit_host_driver.cpp.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define EXG_VN_HD __host__ __device__
#else
#define EXG_VN_HD
#endif

namespace exg {
namespace vn {

enum : uint8_t { kFlag = 0, kInt = 1, kFloat = 2, kString = 3 };  // (= exg::arrow::kVt*, exg_rd::kKey*)

// one declared key (device array, header order)
struct Key {
    uint32_t name_off;  // in KeyTab::names
    uint16_t name_len;
    uint8_t type, is_list;
    uint32_t hash;     // key_hash(name)
    int32_t list_idx;  // index among the list keys of its kind, -1: scalar
};
// host and device agree on the hash (FNV-1a) and the first slot
inline EXG_VN_HD uint32_t key_hash_step(uint32_t h, uint32_t b) { return (h ^ b) * 16777619u; }
static constexpr uint32_t kKeyHashSeed = 2166136261u;
inline EXG_VN_HD uint32_t key_slot(uint32_t h, uint32_t mask) { return (h ^ (h >> 15)) & mask; }

}  // namespace vn
}  // namespace exg
