// exg_gzip.cpp — gzip (RFC 1952) member framing on the host; the DEFLATE streams themselves are
// inflated on the device (exg_inflate.hip).  Replaces the stream framing done inside flate2 /
// noodles-bgzf for the reference (rust/src/arrow_reader.rs:60-91).
//
// BGZF members (and any member whose FEXTRA carries the 'BC' subfield) give their compressed size,
// so the whole file is indexed without decoding and every member is inflated in parallel.  A member
// without it runs to an unknown end: it is returned as the LAST entry with `open_ended` set; the
// caller inflates it, reads how many bytes it consumed, and indexes again from there.
#include <string.h>

#include "exg_common.hpp"

namespace exg {

// CRC-32 (IEEE, reflected) of a header's few bytes: FHCRC is its low 16 bits (RFC 1952 2.3.1)
static uint32_t crc32_bytes(const uint8_t *p, uint64_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}

// The RFC 1952 header of the member at data[pos]: what zlib's inflate accepts, this accepts — the magic, CM = 8, no reserved
// FLG bit, a matching FHCRC — and FEXTRA / FNAME / FCOMMENT of any length are skipped.  *hdr_len: bytes up to the DEFLATE
// stream; *bsize: BSIZE of the LAST 'BC' subfield with SLEN = 2 (BGZF, SAM spec 4.1), or -1.
// EXG_OK; kGzipHeaderShort: the header runs past data[n) (more bytes may complete it); EXG_E_PARSE: invalid (error set).
int gzip_header(const uint8_t *data, uint64_t n, uint64_t pos, uint64_t *hdr_len, int64_t *bsize) {
    *bsize = -1;
    if (n - pos >= 3 && (data[pos] != 0x1f || data[pos + 1] != 0x8b || data[pos + 2] != 8)) {
        set_error("invalid gzip header at byte %llu", (unsigned long long)pos);
        return EXG_E_PARSE;
    }
    if (n - pos < 10) return kGzipHeaderShort;
    const uint8_t flg = data[pos + 3];
    if (flg & 0xE0) {  // zlib: "unknown header flags set"
        set_error("invalid gzip header at byte %llu (reserved FLG bits set)", (unsigned long long)pos);
        return EXG_E_PARSE;
    }
    uint64_t p = pos + 10;
    if (flg & 4) {  // FEXTRA
        if (p + 2 > n) return kGzipHeaderShort;
        const uint64_t xlen = data[p] | ((uint64_t)data[p + 1] << 8);
        p += 2;
        if (p + xlen > n) return kGzipHeaderShort;
        uint64_t q = p;
        while (q + 4 <= p + xlen) {
            const uint64_t slen = data[q + 2] | ((uint64_t)data[q + 3] << 8);
            if (data[q] == 'B' && data[q + 1] == 'C' && slen == 2 && q + 6 <= p + xlen)
                *bsize = (int64_t)(data[q + 4] | ((uint64_t)data[q + 5] << 8));
            q += 4 + slen;
        }
        p += xlen;
    }
    for (int bit = 8; bit <= 16; bit += 8)  // FNAME, FCOMMENT: zero-terminated
        if (flg & bit) {
            while (p < n && data[p]) p++;
            if (p >= n) return kGzipHeaderShort;
            p++;
        }
    if (flg & 2) {  // FHCRC: the low 16 bits of the CRC-32 of the header in front of it (zlib: "header crc mismatch")
        if (p + 2 > n) return kGzipHeaderShort;
        const uint32_t want = data[p] | ((uint32_t)data[p + 1] << 8);
        if ((crc32_bytes(data + pos, p - pos) & 0xFFFFu) != want) {
            set_error("invalid gzip header at byte %llu (header CRC-16 mismatch)", (unsigned long long)pos);
            return EXG_E_PARSE;
        }
        p += 2;
    }
    *hdr_len = p - pos;
    return EXG_OK;
}

}  // namespace exg

extern "C" int exg_gzip_index(const uint8_t *data, uint64_t n, uint64_t start, exg_inflate_member *members, uint64_t cap,
                              uint64_t *n_members, uint64_t *total_out, int *open_ended) {
    if (!data || !members || !n_members || !total_out || !open_ended) {
        exg::set_error("exg_gzip_index: null argument");
        return EXG_E_INVALID_ARG;
    }
    uint64_t pos = start, k = 0, out = *total_out;
    *open_ended = 0;
    while (pos < n) {
        if (n - pos < 18) {
            exg::set_error("invalid gzip header at byte %llu", (unsigned long long)pos);
            return EXG_E_PARSE;
        }
        uint64_t hdr_len = 0;
        int64_t bsize = -1;
        const int hrc = exg::gzip_header(data, n, pos, &hdr_len, &bsize);
        if (hrc == exg::kGzipHeaderShort) goto truncated;
        if (hrc) return hrc;
        const uint64_t p = pos + hdr_len;
        if (k >= cap) {
            exg::set_error("exg_gzip_index: more than %llu members", (unsigned long long)cap);
            return EXG_E_CAPACITY;
        }
        exg_inflate_member &m = members[k];
        m.comp_off = p;
        m.out_off = out;
        if (bsize >= 0) {
            uint64_t end = pos + (uint64_t)bsize + 1;  // BSIZE = total block size - 1
            if (end > n || end < p + 8) goto truncated;
            m.comp_size = end - p;
            uint64_t isize = data[end - 4] | ((uint64_t)data[end - 3] << 8) | ((uint64_t)data[end - 2] << 16) |
                             ((uint64_t)data[end - 1] << 24);
            m.out_cap = isize;
            out += isize;
            pos = end;
            k++;
        } else {
            // unknown compressed size: runs (at most) to the end of the file; ISIZE of the file's last
            // member is in the last 4 bytes (mod 2^32) — a bound only if nothing follows
            m.comp_size = n - p;
            uint64_t isize = data[n - 4] | ((uint64_t)data[n - 3] << 8) | ((uint64_t)data[n - 2] << 16) |
                             ((uint64_t)data[n - 1] << 24);
            // DEFLATE expands at most 1032:1.  A small member (what stays on the one-wavefront path: below 128 KiB of
            // input) gets that bound — `cat a.vcf.gz b.vcf.gz` of highly compressible members must not be reported as
            // corrupt for outgrowing a guessed ratio; a big one is decoded in chunks (exg_inflate_stream sizes its own
            // output), and 8:1 + ISIZE only bounds the fallback with that path switched off
            uint64_t bound = (n - p) < (128u << 10) ? (n - p) * 1032 + 65536 : (n - p) * 8 + 65536;
            m.out_cap = isize > bound ? isize : bound;
            out += m.out_cap;
            k++;
            *open_ended = 1;
            break;
        }
    }
    *n_members = k;
    *total_out = out;
    return EXG_OK;
truncated:
    exg::set_error("truncated gzip member at byte %llu", (unsigned long long)pos);
    return EXG_E_PARSE;
}
