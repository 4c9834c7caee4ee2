// bgzf_scan.h -- host side: the block table of a BGZF buffer that is already in memory (SAM/BAM specification, section 4.1), and
// the same walk over the whole members at the front of a piece (bgzf_walk_members: what the streamed first pass of host_fastx.inl runs on
// its slots) and fed piece by piece with a carry of its own (BgzfWalk: the test form, run by inflate_twin.cpp and
// tools/stream_check.cpp only -- the library keeps the partial member in its pinned slots, fx_src_bgzf_stream).
// Shared by the library (host_inflate.inl) and the host twin (inflate_twin.cpp).
//
// The buffer is accepted only when it is a sequence of gzip members that tile it exactly and every member is a BGZF block:
// 1f 8b 08, no reserved flag bits, FEXTRA with a `BC` subfield of length 2 among the extra subfields (BSIZE = the member's
// size - 1), FNAME / FCOMMENT skipped, FHCRC checked (zlib checks it too), ISIZE <= 65536.  Anything else -- plain or
// multi-member gzip without BC, trailing bytes, a truncated block -- is refused, and the caller decodes on the host.
#pragma once
#include <stdint.h>
#include <stddef.h>
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

// One member at h, of which `avail` bytes are here -- the body both walks share.  BGZF_MEMBER_OK: *b holds its record (c_off and
// o_off are the caller's to set).  BGZF_MEMBER_MORE: the bytes end inside the member and nothing refuses it so far -- a whole
// buffer is truncated there, a piece waits for the next; *need: the bytes of the member that decide at the earliest.
// BGZF_MEMBER_BAD: not a BGZF block, however many bytes follow
enum { BGZF_MEMBER_OK = 0, BGZF_MEMBER_MORE = 1, BGZF_MEMBER_BAD = 2 };
static inline int bgzf_member(const uint8_t *h, uint64_t avail, BgzfBlock *b, uint64_t *need) {
    struct Tab { uint32_t t[256]; Tab() { inf_crc_table(t, 0, 1); } };
    static const Tab crc_tab;
    *need = 18;
    if (avail < 18) return BGZF_MEMBER_MORE;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8) return BGZF_MEMBER_BAD;
    const uint32_t flg = h[3];
    if ((flg & 0xE0) || !(flg & 4)) return BGZF_MEMBER_BAD;
    const uint32_t xlen = bgzf_u16(h + 10);
    *need = 12 + (uint64_t)xlen;
    if (*need > avail) return BGZF_MEMBER_MORE;
    uint64_t bsize = 0;
    bool have_bc = false;
    for (uint32_t x = 0; x + 4 <= xlen;) {
        const uint32_t slen = bgzf_u16(h + 12 + x + 2);
        if (x + 4 + slen > xlen) return BGZF_MEMBER_BAD;
        if (h[12 + x] == 'B' && h[12 + x + 1] == 'C' && slen == 2 && !have_bc) { bsize = bgzf_u16(h + 12 + x + 4); have_bc = true; }
        x += 4 + slen;
    }
    if (!have_bc) return BGZF_MEMBER_BAD;
    const uint64_t blen = bsize + 1;
    if (blen > *need) *need = blen;
    if (blen > avail) return BGZF_MEMBER_MORE;
    uint64_t p = 12 + xlen;
    for (uint32_t f = 8; f <= 16; f <<= 1) {          // FNAME, FCOMMENT: zero-terminated, inside the block
        if (!(flg & f)) continue;
        while (p < blen && h[p]) ++p;
        if (p >= blen) return BGZF_MEMBER_BAD;
        ++p;
    }
    if (flg & 2) {                                       // FHCRC: low 16 bits of the header's CRC-32
        if (p + 2 > blen || bgzf_u16(h + p) != (inf_crc(crc_tab.t, h, (uint32_t)p) & 0xFFFFu)) return BGZF_MEMBER_BAD;
        p += 2;
    }
    if (p + 8 > blen) return BGZF_MEMBER_BAD;
    const uint32_t isize = bgzf_u32(h + blen - 4);
    if (isize > INF_MAX_ISIZE) return BGZF_MEMBER_BAD;
    *b = BgzfBlock{0, 0, (uint32_t)p, (uint32_t)(blen - 8 - p), (uint32_t)blen, isize, bgzf_u32(h + blen - 8)};
    return BGZF_MEMBER_OK;
}

// The whole members at the front of d[0, n), which lies at file offset `base`: their records appended to `out` (may be null)
// with c_off counted from `c_base` (the file, or the buffer the caller decodes from) and o_off from *o, which moves on.  *used:
// the bytes they take.  BGZF_MEMBER_OK: they tile d.  _MORE: a member starts at d + *used and ends behind d + n (*need as
// bgzf_member).  _BAD: what starts at file offset *bad_off is no BGZF block
static inline int bgzf_walk_members(const uint8_t *d, uint64_t n, uint64_t base, uint64_t c_base, uint64_t *o, std::vector<BgzfBlock> *out, uint64_t *used,
                                    uint64_t *need, uint64_t *bad_off) {
    for (*used = 0; *used < n;) {
        BgzfBlock b;
        const int rc = bgzf_member(d + *used, n - *used, &b, need);
        if (rc == BGZF_MEMBER_BAD) *bad_off = base + *used;
        if (rc != BGZF_MEMBER_OK) return rc;
        b.c_off = c_base + *used; b.o_off = *o;
        if (out) out->push_back(b);
        *o += b.isize;
        *used += b.c_len;
    }
    return BGZF_MEMBER_OK;
}

// true: `out` (may be null) holds the block table and *out_len the decompressed size
static inline bool bgzf_scan_blocks(const uint8_t *d, uint64_t n, std::vector<BgzfBlock> *out, uint64_t *out_len) {
    if (out) out->clear();
    uint64_t o = 0, used = 0, need = 0, bad = 0;
    if (n == 0 || bgzf_walk_members(d, n, 0, 0, &o, out, &used, &need, &bad) != BGZF_MEMBER_OK) return false;
    if (out_len) *out_len = o;
    return true;
}

// The incremental form of the walk as the tests drive it (the library's carry is fx_src_bgzf_stream's, over the same
// bgzf_walk_members): fed consecutive pieces of a file, it yields the records bgzf_scan_blocks
// gives for the whole buffer, under the same rules.  A member that a piece holds only in part stays in `carry` for the next piece.
// feed / end return false once the file is refused: bad_off is the file offset of the member (or of the trailing bytes) that
// refuses it, the same at every piece size -- the start of the first member that is not a whole BGZF block
struct BgzfWalk {
    std::vector<uint8_t> carry;                 // the bytes behind the last whole member
    uint64_t off = 0, o = 0, need = 18, members = 0, bad_off = 0;      // off: the file offset of carry[0]; o: text bytes so far
    bool bad = false;
    bool feed(const uint8_t *p, uint64_t n, std::vector<BgzfBlock> *out) {
        if (bad) return false;
        carry.insert(carry.end(), p, p + n);
        if (carry.size() < need) return true;   // (the member in front cannot be decided yet)
        std::vector<BgzfBlock> unasked;
        if (!out) out = &unasked;
        const size_t before = out->size();
        uint64_t used = 0;
        const int rc = bgzf_walk_members(carry.data(), carry.size(), off, off, &o, out, &used, &need, &bad_off);
        if (rc == BGZF_MEMBER_BAD) { bad = true; return false; }
        if (rc == BGZF_MEMBER_OK) need = 18;
        members += out->size() - before;
        carry.erase(carry.begin(), carry.begin() + (std::ptrdiff_t)used);
        off += used;
        return true;
    }
    // the input is over: no member, a truncated member or trailing bytes refuse the file
    bool end() {
        if (bad) return false;
        if (!carry.empty() || !members) { bad = true; bad_off = off; return false; }
        return true;
    }
};
