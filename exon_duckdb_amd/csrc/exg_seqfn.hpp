// exg_seqfn.hpp — the rules of the sequence scalars and the SAM flag predicates, stated ONCE for the device op
// (exg_seqfn.hip), the host scalars (exon_table_function.hpp, which the DuckDB shim registers) and the C-ABI's error text.
// Plain C++: no HIP, no DuckDB; every table is constexpr and usable from host and device code.
//
// Reference: exon/src/exon/sequence_functions/module.cpp:30-370 and rust/src/sam_functions.rs:19-90.
//   complement          A->T T->A C->G G->C                                  (:81-121)
//   reverse_complement  A->C T->G C->A G->T, byte order KEPT: what the reference computes, pinned by
//                       test_scalar_functions.test:43-46 (ATCG -> CGAT, GGGG -> TTTT), not what the name says   (:30-69)
//   transcribe          T->U, A C G kept                                     (:215-253)
//   reverse_transcribe  U->T, A C G kept                                     (:168-205)
//   translate_dna_to_aa length % 3 first, then codons left to right through the 64-entry table of :266-330
//   gc_content          (float)#{G, C} / (float)length, 0 for the empty string; every byte accepted, upper case only (:131-158)
// Any byte outside a mapping's four letters is an error; a lower-case letter or a byte >= 0x80 is simply such a byte.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "exon_gpu.h"

#if defined(__HIPCC__)
#define EXG_SEQ_HD __host__ __device__ inline
#else
#define EXG_SEQ_HD inline
#endif

namespace exg {
namespace seqfn {

// The four letters of every alphabet here differ in bits 1-2: (c >> 1) & 3 is A 0, C 1, T / U 2, G 3.  A mapping is two
// packed words indexed by that code: the letter the code must have come from, and the letter it becomes.
struct ByteMap {
    uint32_t from, to;
};
constexpr uint32_t pack4(char a, char c, char t, char g) {
    return (uint32_t)(uint8_t)a | ((uint32_t)(uint8_t)c << 8) | ((uint32_t)(uint8_t)t << 16) | ((uint32_t)(uint8_t)g << 24);
}
static constexpr uint32_t kDna = pack4('A', 'C', 'T', 'G'), kRna = pack4('A', 'C', 'U', 'G');
EXG_SEQ_HD constexpr ByteMap byte_map(uint32_t op) {
    return op == EXG_SEQ_COMPLEMENT           ? ByteMap{kDna, pack4('T', 'G', 'A', 'C')}
           : op == EXG_SEQ_REVERSE_COMPLEMENT ? ByteMap{kDna, pack4('C', 'A', 'G', 'T')}
           : op == EXG_SEQ_TRANSCRIBE         ? ByteMap{kDna, kRna}
           : op == EXG_SEQ_REVERSE_TRANSCRIBE ? ByteMap{kRna, kDna}
                                              : ByteMap{kDna, kDna};  // (translate: the codon letters)
}
EXG_SEQ_HD constexpr uint32_t base_code(uint32_t c) { return (c >> 1) & 3u; }
EXG_SEQ_HD constexpr bool base_ok(uint32_t from, uint32_t c) { return ((from >> (8 * base_code(c))) & 0xFFu) == c; }
EXG_SEQ_HD constexpr uint32_t base_to(uint32_t to, uint32_t c) { return (to >> (8 * base_code(c))) & 0xFFu; }

// module.cpp:266-330 indexed by base_code(first) * 16 + base_code(second) * 4 + base_code(third)
EXG_SEQ_HD constexpr char codon_aa(uint32_t index) {
    return "KNNKTTTTIIIMRSSRQHHQPPPPLLLLRRRR*YY*SSSSLFFL*CCWEDDEAAAAVVVVGGGG"[index & 63u];
}
EXG_SEQ_HD constexpr bool codon_ok(uint32_t a, uint32_t b, uint32_t c) { return base_ok(kDna, a) && base_ok(kDna, b) && base_ok(kDna, c); }
EXG_SEQ_HD constexpr uint32_t codon_index(uint32_t a, uint32_t b, uint32_t c) {
    return base_code(a) * 16u + base_code(b) * 4u + base_code(c);
}

EXG_SEQ_HD constexpr bool is_gc(uint32_t c) { return (c & 0xFBu) == 0x43u; }  // 'C' 0x43, 'G' 0x47
// one IEEE float32 division of the two converted integers (module.cpp:156)
EXG_SEQ_HD float gc_ratio(uint32_t count, uint32_t length) { return length ? (float)count / (float)length : 0.0f; }

EXG_SEQ_HD constexpr bool is_string_op(uint32_t op) { return op >= EXG_SEQ_COMPLEMENT && op <= EXG_SEQ_TRANSLATE; }
EXG_SEQ_HD constexpr uint64_t output_length(uint32_t op, uint64_t length) { return op == EXG_SEQ_TRANSLATE ? length / 3 : length; }

// SAM flag predicates in the reference's order (sam_functions/module.cpp:143-154): bit k of (uint16_t)flag
static constexpr int kSamFlagCount = 12;
static constexpr const char *kSamFlagNames[kSamFlagCount] = {
    "is_segmented", "is_properly_aligned", "is_unmapped", "is_mate_unmapped", "is_reverse_complemented",
    "is_mate_reverse_complemented", "is_first_segment", "is_last_segment", "is_secondary", "is_quality_control_failed",
    "is_duplicate", "is_supplementary"};
EXG_SEQ_HD constexpr bool sam_flag(uint32_t which, int32_t flag) { return (((uint16_t)flag) >> which) & 1u; }

// the reference's exception text for an EXG_PE_SEQ_* (module.cpp:64, :115, :344, :355); returns the number of bytes written
// (no terminator counted; the byte / the codon goes in raw, as the reference appends it)
inline size_t format_error(uint32_t code, const uint8_t bytes[4], uint64_t length, char *out, size_t cap) {
    if (!cap) return 0;
    int n = 0;
    if (code == EXG_PE_SEQ_LENGTH)
        n = snprintf(out, cap, "Invalid sequence length: %llu", (unsigned long long)length);
    else if (code == EXG_PE_SEQ_CODON)
        n = snprintf(out, cap, "Invalid codon: %c%c%c", bytes[0], bytes[1], bytes[2]);
    else if (code == EXG_PE_SEQ_INVALID_CHARACTER)
        n = snprintf(out, cap, "Invalid character in sequence: %c", bytes[0]);
    else
        out[0] = 0;
    return n < 0 ? 0 : ((size_t)n < cap ? (size_t)n : cap - 1);
}

}  // namespace seqfn
}  // namespace exg
