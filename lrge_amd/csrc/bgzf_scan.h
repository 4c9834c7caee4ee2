// bgzf_scan.h -- host side: the block table of a BGZF buffer that is already in memory (SAM/BAM specification, section 4.1).
// Shared by the library (host_inflate.inl) and the host twin (inflate_twin.cpp).
//
// The buffer is accepted only when it is a sequence of gzip members that tile it exactly and every member is a BGZF block:
// 1f 8b 08, no reserved flag bits, FEXTRA with a `BC` subfield of length 2 among the extra subfields (BSIZE = the member's
// size - 1), FNAME / FCOMMENT skipped, FHCRC checked (zlib checks it too), ISIZE <= 65536.  Anything else -- plain or
// multi-member gzip without BC, trailing bytes, a truncated block -- is refused, and the caller decodes on the host.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "inflate_core.h"

struct BgzfBlock {
    uint64_t c_off;     // file offset of the member
    uint64_t o_off;     // offset of its bytes in the decompressed output
    uint32_t d_off;     // deflate data: [c_off + d_off, c_off + d_off + d_len)
    uint32_t d_len;
    uint32_t c_len;     // the whole member (BSIZE + 1)
    uint32_t isize, crc;
};

static inline uint32_t bgzf_u16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
static inline uint32_t bgzf_u32(const uint8_t *p) { return bgzf_u16(p) | bgzf_u16(p + 2) << 16; }

// true: `out` (may be null) holds the block table and *out_len the decompressed size
static inline bool bgzf_scan_blocks(const uint8_t *d, uint64_t n, std::vector<BgzfBlock> *out, uint64_t *out_len) {
    struct Tab { uint32_t t[256]; Tab() { inf_crc_table(t, 0, 1); } };
    static const Tab crc_tab;
    if (out) out->clear();
    uint64_t off = 0, o = 0;
    if (n == 0) return false;
    while (off < n) {
        const uint8_t *h = d + off;
        const uint64_t rem = n - off;
        if (rem < 18 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8) return false;
        const uint32_t flg = h[3];
        if ((flg & 0xE0) || !(flg & 4)) return false;
        const uint32_t xlen = bgzf_u16(h + 10);
        if (12 + (uint64_t)xlen > rem) return false;
        uint64_t bsize = 0;
        bool have_bc = false;
        for (uint32_t x = 0; x + 4 <= xlen;) {
            const uint32_t slen = bgzf_u16(h + 12 + x + 2);
            if (x + 4 + slen > xlen) return false;
            if (h[12 + x] == 'B' && h[12 + x + 1] == 'C' && slen == 2 && !have_bc) { bsize = bgzf_u16(h + 12 + x + 4); have_bc = true; }
            x += 4 + slen;
        }
        if (!have_bc) return false;
        const uint64_t blen = bsize + 1;
        if (blen > rem) return false;
        uint64_t p = 12 + xlen;
        for (uint32_t f = 8; f <= 16; f <<= 1) {          // FNAME, FCOMMENT: zero-terminated, inside the block
            if (!(flg & f)) continue;
            while (p < blen && h[p]) ++p;
            if (p >= blen) return false;
            ++p;
        }
        if (flg & 2) {                                       // FHCRC: low 16 bits of the header's CRC-32
            if (p + 2 > blen || bgzf_u16(h + p) != (inf_crc(crc_tab.t, h, (uint32_t)p) & 0xFFFFu)) return false;
            p += 2;
        }
        if (p + 8 > blen) return false;
        const uint32_t isize = bgzf_u32(h + blen - 4);
        if (isize > INF_MAX_ISIZE) return false;
        if (out) out->push_back(BgzfBlock{off, o, (uint32_t)p, (uint32_t)(blen - 8 - p), (uint32_t)blen, isize, bgzf_u32(h + blen - 8)});
        o += isize;
        off += blen;
    }
    if (out_len) *out_len = o;
    return true;
}
