// exg_sam_header.hpp — where the header of a SAM text ends.  The header is the maximal run of lines at the start of the
// decoded stream whose first byte is '@' (its contents are not parsed: no column needs them — reference names are in every
// record's RNAME); the reader skips it at open, the way the VCF header sets data_base.
// Host only and free of any HIP include: under ASan + UBSan in tests/sam_header_driver.cpp.
#pragma once
#include <stddef.h>
#include <string.h>

namespace exg_rd {

// The offset of the first byte behind the leading lines of d[0, n) that begin with `marker` ('@': SAM, '#': VCF).  n when
// every line begins with it — the caller then cannot tell whether the header goes on behind the bytes it holds: that the
// last of them is a line feed says nothing about the next line — or when the last such line has no line feed inside d[0, n).
inline size_t leading_lines_end(const char *d, size_t n, char marker) {
    size_t pos = 0;
    while (pos < n && d[pos] == marker) {
        const void *nl = memchr(d + pos, '\n', n - pos);
        pos = nl ? (size_t)((const char *)nl - d) + 1 : n;
    }
    return pos;
}
inline size_t sam_header_end(const char *d, size_t n) { return leading_lines_end(d, n, '@'); }

}  // namespace exg_rd
