// exg_vcf_region.hpp — the row rule of vcf_query, stated ONCE for the device predicate (exg_vcf_region.hip: exg_vcf_region_keep)
// and for the host (tests/region_host_driver.cpp runs this same code under ASan / UBSan).  Plain C++: no HIP, no DuckDB; usable
// from host and device code.
//
// A row (chrom, pos, ref, info) overlaps the region (name, start, end), coordinates 1-based and closed, when
//   R1  chrom equals the name byte for byte — the lengths are equal too: `1` is not `10`
//   R2  pos <= end
//   R3  row_end >= start
// row_end [RECALLED: noodles-vcf Record::end]
//   E1  the integer of the INFO key `END=` when there is one: the key stands at the start of INFO or right behind a `;`
//       (`SVEND=` is not it), its value is decimal digits up to the next `;` or the field's end; the first key named END decides
//   E2  `END` without a value, `END=.`, `END=` with nothing, anything that is not digits only, or more than 18 digits: the key
//       counts as absent [DECIDED] (and a second END key behind it is not looked for)
//   E3  no END key: pos + len(ref) - 1
//   E4  a row whose pos lies in [start, end] is kept without a look at INFO [DECIDED] (an END in front of pos would make
//       noodles' interval empty; the row starts in the region and is a row of it)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EXG_REGION_HD __host__ __device__ inline
#else
#define EXG_REGION_HD inline
#endif

namespace exg {
namespace vcf_region {

static constexpr uint32_t kMaxEndDigits = 18;  // below 10^18: fits an int64 with room to spare

// R1
EXG_REGION_HD bool same_name(const uint8_t *chrom, uint32_t chrom_len, const uint8_t *name, uint32_t name_len) {
    if (chrom_len != name_len) return false;
    for (uint32_t i = 0; i < name_len; i++)
        if (chrom[i] != name[i]) return false;
    return true;
}

// E1 / E2: the value of the first `END=` key of info[0, len); false: the key is absent (or counts as absent)
EXG_REGION_HD bool info_end(const uint8_t *info, uint32_t len, int64_t *out) {
    for (uint32_t i = 0; i < len;) {  // i: the first byte of a key
        if (len - i >= 3 && info[i] == 'E' && info[i + 1] == 'N' && info[i + 2] == 'D' && (len - i == 3 || info[i + 3] == '=' || info[i + 3] == ';')) {
            if (len - i == 3 || info[i + 3] == ';') return false;  // `END` without a value
            int64_t v = 0;
            uint32_t j = i + 4, digits = 0;
            for (; j < len && info[j] != ';'; j++, digits++) {
                const uint32_t d = (uint32_t)info[j] - '0';
                if (d > 9 || digits >= kMaxEndDigits) return false;
                v = v * 10 + (int64_t)d;
            }
            if (!digits) return false;
            *out = v;
            return true;
        }
        while (i < len && info[i] != ';') i++;
        i++;  // behind the `;`
    }
    return false;
}

// R2 / R3 for a row whose chrom is the region's (E4: `info` is read only when pos < start)
EXG_REGION_HD bool overlaps(int64_t pos, uint32_t ref_len, const uint8_t *info, uint32_t info_len, int64_t start, int64_t end) {
    if (pos > end) return false;
    if (pos >= start) return true;
    int64_t row_end = 0;
    if (!info_end(info, info_len, &row_end)) row_end = pos + (int64_t)ref_len - 1;
    return row_end >= start;
}

}  // namespace vcf_region
}  // namespace exg
