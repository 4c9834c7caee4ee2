// xz_core.h -- the rules of the .xz container's payload: the LZMA2 chunk decode (the adaptive range decoder, the LZMA symbol
// grammar, the copies) of one block by one wavefront, and the block checks CRC32 / CRC64 over lane stripes.  Compiled by hipcc
// (k_xz.h) and g++ (xz_twin.cpp) alike; written from the format's descriptions (xz-file-format-1.0.4, the LZMA specification).
//
// A function that runs as a wavefront takes an environment E: lane0() / lane1() bound the lanes the caller stands for (one on the
// device, all 64 in the twin, which therefore walks the same 64-byte steps), sync() separates a step that writes memory the
// wavefront shares from one that reads it, and e.probs / e.stage / e.ring / e.tab are the block's tables (LDS on the device).
// Control is wavefront-uniform: every lane keeps the same decoder state; only the copies are spread over the lanes.
//
// Memory safety by construction: the range decoder reads compressed bytes through the stage only, inside the chunk's csize bytes
// (past them it reads zeros and the chunk fails); a literal or a match is written only below the chunk's usize; a distance is
// checked against the bytes since the last dictionary reset before its source is read; every loop is bounded by one of the two
// sizes, both from the host's chunk table, which lies inside the file and inside the block's reserved text.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define XZ_FN __host__ __device__ static inline
#else
#define XZ_FN static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define XZ_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))   // a value every lane holds: kept in a scalar register
#else
#define XZ_UNI(x) ((uint32_t)(x))
#endif

enum {
    XZ_OK = 0,
    XZ_E_MAGIC = 1,          // no stream header magic where a stream must start
    XZ_E_INPUT = 2,          // the file is shorter than the smallest stream, or a size points outside it (truncation)
    XZ_E_FOOTER = 3,         // no stream footer where the file or a stream must end: truncated, or bytes that are neither a stream nor padding
    XZ_E_RESERVED = 4,       // a reserved bit is set (stream flags, block flags)
    XZ_E_CHECK_ID = 5,       // a check other than none, CRC32, CRC64 (SHA-256, reserved IDs)
    XZ_E_HEADER_CRC = 6,     // the CRC32 of a stream header, a stream footer, an index or a block header
    XZ_E_FLAGS = 7,          // header and footer stream flags differ
    XZ_E_INDEX = 8,          // an index that is no index: indicator, an integer's encoding, record count, sizes, padding, Backward Size
    XZ_E_FILTER = 9,         // a filter other than LZMA2, more than one filter, or LZMA2 properties that are not one byte
    XZ_E_PADDING = 10,       // header, block or stream padding that is not zero bytes, or stream padding no multiple of four
    XZ_E_SIZES = 11,         // a block header's size fields differ from the index record, or the chunks do not sum to the record
    XZ_E_CONTROL = 12,       // an invalid control byte, a first chunk without a dictionary reset, an LZMA chunk with no properties in force
    XZ_E_PROPS = 13,         // lc + lp > 4, or a properties byte above 224
    XZ_E_DICT_SIZE = 14,     // a dictionary size byte above 40
    XZ_E_DIST = 15,          // a distance at or beyond the bytes since the last dictionary reset, or at or beyond the dictionary size
    XZ_E_END_MARKER = 16,    // the end marker (LZMA2 chunks state their size)
    XZ_E_MATCH_CROSS = 17,   // a match that crosses its chunk's uncompressed size
    XZ_E_RC = 18,            // a range decoder whose first byte is not 0, or that does not end with code == 0 exactly at the chunk's compressed size
    XZ_E_CHECK = 19,         // the block's text does not give its stored check
    XZ_E_FEW_BLOCKS = 20,    // fewer blocks than XZ_MIN_BLOCKS (no damage)
    XZ_E_TOO_BIG = 21,       // the text does not fit the device budget (no damage)
};

#define XZ_NL 64u                        // lanes of a wavefront: the step of every copy
#define XZ_PROBS_BASE 1846u
#define XZ_PROBS_MAX (XZ_PROBS_BASE + (768u << 4))   // 14 134 entries of 16 bits: 28 268 bytes
#define XZ_STAGE 2048u                   // compressed bytes staged at a time
#define XZ_RING 4096u                    // the most recent output kept beside the model (a power of two)
#define XZ_FLUSH 512u                    // bytes that may wait in the ring before they go to the text
#define XZ_MATCH_MAX 273u
#define XZ_NEAR (XZ_RING - 1024u)        // a match at most this far back copies ring to ring: its sources are neither unflushed nor overwritten
#define XZ_CHUNK_USIZE_MAX (1u << 21)
#define XZ_CHUNK_CSIZE_MAX (1u << 16)

// the model's layout (entries of 16 bits)
#define XZ_P_IS_MATCH 0u
#define XZ_P_IS_REP 192u
#define XZ_P_IS_REP_G0 204u
#define XZ_P_IS_REP_G1 216u
#define XZ_P_IS_REP_G2 228u
#define XZ_P_IS_REP0_LONG 240u
#define XZ_P_POS_SLOT 432u
#define XZ_P_SPEC_POS 688u
#define XZ_P_ALIGN 802u
#define XZ_P_LEN 818u
#define XZ_P_REP_LEN 1332u
#define XZ_P_LITERAL 1846u

// chunk flags
#define XZ_C_RAW 1u                      // an uncompressed chunk
#define XZ_C_DICT_RESET 2u
#define XZ_C_STATE_RESET 4u

// an LZMA2 chunk of a block, from the host's hop over the chunk headers
struct XzChunk {
    uint64_t at;                         // its control byte in the file
    uint64_t src;                        // its payload in the file
    uint64_t out;                        // its first byte, from the block's first
    uint64_t dict_at;                    // the block position of the last dictionary reset at or in front of it
    uint32_t csize, usize;
    uint32_t dict_size;
    uint8_t flags, lc, lp, pb;           // the properties in force
};
// a block's work of one launch: chunks [c0, c1) of the table, its text, its state slot
struct XzTask { uint64_t text; uint32_t c0, c1, slot, pad; };
// what a block carries from launch to launch beside the model
struct XzSave { uint32_t status, chunk, state, rep[4], pad; };
#define XZ_SLOT_BYTES ((uint32_t)(sizeof(XzSave) + XZ_PROBS_MAX * 2 + 15) & ~15u)

XZ_FN uint32_t xz_le32(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
XZ_FN uint64_t xz_le64(const uint8_t *p) { return xz_le32(p) | (uint64_t)xz_le32(p + 4) << 32; }

// ---- the range decoder over the staged bytes of one chunk ----
struct XzRc {
    const uint8_t *src;                  // the chunk's payload
    uint32_t csize, ip;                  // its size, the next byte
    uint32_t s0, s1;                     // the staged span
    uint32_t range, code;
    uint32_t over;                       // a byte past the chunk was asked for
};

template <class E> XZ_FN void xz_stage(E &e, XzRc &rc) {
    rc.s0 = rc.ip;
    rc.s1 = rc.csize - rc.ip < XZ_STAGE ? rc.csize : rc.ip + XZ_STAGE;
    e.sync();                            // (every lane has read what it needed of the bytes staged before)
    for (uint32_t l = e.lane0(); l < e.lane1(); ++l) for (uint32_t i = rc.s0 + l; i < rc.s1; i += XZ_NL) e.stage[i - rc.s0] = rc.src[i];
    e.sync();
}
template <class E> XZ_FN uint32_t xz_byte(E &e, XzRc &rc) {
    if (rc.ip >= rc.csize) { rc.over = 1; return 0; }
    if (rc.ip >= rc.s1) xz_stage(e, rc);
    return XZ_UNI(e.stage[rc.ip++ - rc.s0]);
}
template <class E> XZ_FN void xz_norm(E &e, XzRc &rc) {
    if (rc.range < (1u << 24)) { rc.range <<= 8; rc.code = rc.code << 8 | xz_byte(e, rc); }
}
template <class E> XZ_FN uint32_t xz_bit(E &e, XzRc &rc, uint32_t i) {
    xz_norm(e, rc);
    const uint32_t p = XZ_UNI(e.probs[i]), bound = (rc.range >> 11) * p;
    if (rc.code < bound) { rc.range = bound; e.probs[i] = (uint16_t)(p + ((2048u - p) >> 5)); return 0; }
    rc.range -= bound; rc.code -= bound; e.probs[i] = (uint16_t)(p - (p >> 5));
    return 1;
}
template <class E> XZ_FN uint32_t xz_tree(E &e, XzRc &rc, uint32_t base, uint32_t bits) {
    uint32_t m = 1;
    for (uint32_t i = 0; i < bits; ++i) m = m << 1 | xz_bit(e, rc, base + m);
    return m - (1u << bits);
}
template <class E> XZ_FN uint32_t xz_tree_rev(E &e, XzRc &rc, uint32_t base, uint32_t bits) {
    uint32_t m = 1, v = 0;
    for (uint32_t i = 0; i < bits; ++i) { const uint32_t b = xz_bit(e, rc, base + m); m = m << 1 | b; v |= b << i; }
    return v;
}
template <class E> XZ_FN uint32_t xz_direct(E &e, XzRc &rc, uint32_t bits) {
    uint32_t v = 0;
    for (uint32_t i = 0; i < bits; ++i) {
        xz_norm(e, rc);
        rc.range >>= 1;
        const uint32_t b = rc.code >= rc.range;
        if (b) rc.code -= rc.range;
        v = v << 1 | b;
    }
    return v;
}
template <class E> XZ_FN uint32_t xz_len(E &e, XzRc &rc, uint32_t base, uint32_t ps) {
    if (!xz_bit(e, rc, base)) return 2 + xz_tree(e, rc, base + 2 + (ps << 3), 3);
    if (!xz_bit(e, rc, base + 1)) return 10 + xz_tree(e, rc, base + 130 + (ps << 3), 3);
    return 18 + xz_tree(e, rc, base + 258, 8);
}

// ---- the output: the ring beside the model, the text behind it ----
struct XzOut {
    uint8_t *o;                          // the block's first byte in the text
    uint64_t pos, flushed;               // bytes of the block so far, of them in the text
    uint32_t prev;                       // the byte at pos - 1 (0 behind a dictionary reset)
};
// the ring's bytes [flushed, pos) into the text
template <class E> XZ_FN void xz_flush(E &e, XzOut &w) {
    e.sync();                            // the ring bytes other lanes wrote
    for (uint32_t l = e.lane0(); l < e.lane1(); ++l)
        for (uint64_t i = w.flushed + l; i < w.pos; i += XZ_NL) w.o[i] = e.ring[i & (XZ_RING - 1)];
    w.flushed = w.pos;
}
// the ring from the text's last bytes (a launch starts, an uncompressed chunk has been copied)
template <class E> XZ_FN void xz_ring_load(E &e, XzOut &w) {
    const uint64_t from = w.pos > XZ_RING ? w.pos - XZ_RING : 0;
    e.sync();                            // the text bytes other lanes wrote
    for (uint32_t l = e.lane0(); l < e.lane1(); ++l)
        for (uint64_t i = from + l; i < w.pos; i += XZ_NL) e.ring[i & (XZ_RING - 1)] = w.o[i];
    e.sync();
    w.flushed = w.pos;
}
// the byte `dist` (1 based) in front of pos: ring or text.  dist <= pos, checked by the caller
template <class E> XZ_FN uint32_t xz_byte_back(E &e, XzOut &w, uint32_t dist) {
    e.sync();                            // a match's bytes are other lanes'
    if (dist <= XZ_RING) return XZ_UNI(e.ring[(w.pos - dist) & (XZ_RING - 1)]);
    return XZ_UNI(w.o[w.pos - dist]);    // (flushed: fewer than XZ_FLUSH + XZ_MATCH_MAX bytes ever wait)
}
// len bytes from dist (1 based) back, by the `j mod dist` rule: every source lies in front of pos, so no step reads what another wrote
template <class E> XZ_FN void xz_match(E &e, XzOut &w, uint32_t dist, uint32_t len) {
    e.sync();                            // the bytes (ring and text) written so far
    const uint32_t last = len - 1 < dist ? len - 1 : (len - 1) % dist;
    if (dist <= XZ_NEAR) {
        w.prev = XZ_UNI(e.ring[(w.pos - dist + last) & (XZ_RING - 1)]);
        for (uint32_t k0 = 0; k0 < len; k0 += XZ_NL)
            for (uint32_t l = e.lane0(); l < e.lane1(); ++l) {
                const uint32_t j = k0 + l;
                if (j >= len) continue;
                // (source and target slots differ: dist + j - j mod dist lies in [1, XZ_NEAR + XZ_MATCH_MAX) and that is below XZ_RING)
                e.ring[(w.pos + j) & (XZ_RING - 1)] = e.ring[(w.pos - dist + (j < dist ? j : j % dist)) & (XZ_RING - 1)];
            }
    } else {                             // dist > XZ_NEAR > len: the sources are in the text (flushed) and do not overlap the match
        const uint8_t *s = w.o + (w.pos - dist);
        w.prev = XZ_UNI(s[last]);
        for (uint32_t k0 = 0; k0 < len; k0 += XZ_NL)
            for (uint32_t l = e.lane0(); l < e.lane1(); ++l) {
                const uint32_t j = k0 + l;
                if (j < len) e.ring[(w.pos + j) & (XZ_RING - 1)] = s[j];
            }
    }
    w.pos += len;
}

// ---- one chunk ----
// an LZMA chunk into the block's text.  st: the LZMA state and the four distances (0 based), carried from chunk to chunk
template <class E> XZ_FN uint32_t xz_lzma_chunk(E &e, const uint8_t *in, const XzChunk &c, XzOut &w, uint32_t &state, uint32_t *rep) {
    XzRc rc;
    rc.src = in + c.src; rc.csize = c.csize; rc.ip = 0; rc.s0 = rc.s1 = 0; rc.over = 0;
    rc.range = 0xFFFFFFFFu; rc.code = 0;
    if (c.csize < 5) return XZ_E_RC;
    if (xz_byte(e, rc) != 0) return XZ_E_RC;
    for (uint32_t i = 0; i < 4; ++i) rc.code = rc.code << 8 | xz_byte(e, rc);
    const uint32_t lc = c.lc, lp_mask = (1u << c.lp) - 1, pb_mask = (1u << c.pb) - 1;
    const uint64_t end = c.out + c.usize;
    uint32_t r0 = rep[0], r1 = rep[1], r2 = rep[2], r3 = rep[3];
    while (w.pos < end) {
        if (rc.over) return XZ_E_RC;
        const uint64_t dpos = w.pos - c.dict_at;
        const uint32_t ps = (uint32_t)dpos & pb_mask;
        if (!xz_bit(e, rc, XZ_P_IS_MATCH + (state << 4) + ps)) {
            const uint32_t pl = XZ_P_LITERAL + 0x300u * ((((uint32_t)dpos & lp_mask) << lc) + (w.prev >> (8 - lc)));
            uint32_t sym = 1;
            if (state < 7) {
                do sym = sym << 1 | xz_bit(e, rc, pl + sym); while (sym < 0x100);
            } else {
                // (state >= 7 follows a match or a rep, which checked r0 against the bytes in front of it)
                uint32_t mb = xz_byte_back(e, w, r0 + 1), offs = 0x100;
                do {
                    mb <<= 1;
                    const uint32_t mbit = mb & offs, b = xz_bit(e, rc, pl + offs + mbit + sym);
                    sym = sym << 1 | b;
                    offs &= b ? mbit : ~mbit;
                } while (sym < 0x100);
            }
            state = state < 4 ? 0 : state < 10 ? state - 3 : state - 6;
            w.prev = sym & 0xFF;
            e.ring[w.pos & (XZ_RING - 1)] = (uint8_t)sym;     // (every lane writes the same byte)
            ++w.pos;
        } else {
            uint32_t len;
            if (!xz_bit(e, rc, XZ_P_IS_REP + state)) {
                r3 = r2; r2 = r1; r1 = r0;
                len = xz_len(e, rc, XZ_P_LEN, ps);
                state = state < 7 ? 7 : 10;
                const uint32_t slot = xz_tree(e, rc, XZ_P_POS_SLOT + ((len < 6 ? len - 2 : 3) << 6), 6);
                if (slot < 4) r0 = slot;
                else {
                    const uint32_t nb = (slot >> 1) - 1;
                    r0 = (2 | (slot & 1)) << nb;
                    if (slot < 14) r0 += xz_tree_rev(e, rc, XZ_P_SPEC_POS + r0 - slot - 1, nb);
                    else {
                        r0 += xz_direct(e, rc, nb - 4) << 4;
                        r0 += xz_tree_rev(e, rc, XZ_P_ALIGN, 4);
                        if (r0 == 0xFFFFFFFFu) return rc.over ? XZ_E_RC : XZ_E_END_MARKER;
                    }
                }
            } else if (!xz_bit(e, rc, XZ_P_IS_REP_G0 + state)) {
                if (!xz_bit(e, rc, XZ_P_IS_REP0_LONG + (state << 4) + ps)) { len = 1; state = state < 7 ? 9 : 11; }
                else { len = xz_len(e, rc, XZ_P_REP_LEN, ps); state = state < 7 ? 8 : 11; }
            } else {
                uint32_t d;
                if (!xz_bit(e, rc, XZ_P_IS_REP_G1 + state)) d = r1;
                else {
                    if (!xz_bit(e, rc, XZ_P_IS_REP_G2 + state)) d = r2;
                    else { d = r3; r3 = r2; }
                    r2 = r1;
                }
                r1 = r0; r0 = d;
                len = xz_len(e, rc, XZ_P_REP_LEN, ps); state = state < 7 ? 8 : 11;
            }
            if (rc.over) return XZ_E_RC;
            if (r0 >= dpos || r0 >= c.dict_size) return XZ_E_DIST;
            if (len > end - w.pos) return XZ_E_MATCH_CROSS;
            xz_match(e, w, r0 + 1, len);
        }
        if (w.pos - w.flushed >= XZ_FLUSH) xz_flush(e, w);
    }
    xz_flush(e, w);
    xz_norm(e, rc);
    if (rc.over || rc.code != 0 || rc.ip != rc.csize) return XZ_E_RC;
    rep[0] = r0; rep[1] = r1; rep[2] = r2; rep[3] = r3;
    return XZ_OK;
}

XZ_FN uint32_t xz_n_probs(uint32_t lc, uint32_t lp) { return XZ_PROBS_BASE + (768u << (lc + lp)); }

// chunks [t.c0, t.c1) of a block: the state comes from the block's slot unless the first chunk resets it, and goes back there.
// Returns the status on every lane; *bad_chunk: the chunk it belongs to
template <class E> XZ_FN uint32_t xz_decode(E &e, const uint8_t *in, const XzChunk *chunks, const XzTask &t, uint8_t *text, uint8_t *slots, uint32_t *bad_chunk) {
    XzSave *sv = (XzSave *)(slots + (uint64_t)t.slot * XZ_SLOT_BYTES);
    uint16_t *saved = (uint16_t *)(sv + 1);
    uint32_t state = XZ_UNI(sv->state), rep[4] = {XZ_UNI(sv->rep[0]), XZ_UNI(sv->rep[1]), XZ_UNI(sv->rep[2]), XZ_UNI(sv->rep[3])};
    uint32_t n_probs = 0;                // the model entries in use (0: none yet)
    XzOut w;
    w.o = text + t.text; w.pos = w.flushed = chunks[t.c0].out;
    w.prev = 0;
    {   // the ring, the byte in front, the model of the launch before
        const XzChunk &c = chunks[t.c0];
        xz_ring_load(e, w);
        if (w.pos > c.dict_at) w.prev = XZ_UNI(e.ring[(w.pos - 1) & (XZ_RING - 1)]);
        if (!(c.flags & XZ_C_STATE_RESET) && c.out) {
            n_probs = XZ_PROBS_MAX;
            for (uint32_t l = e.lane0(); l < e.lane1(); ++l) for (uint32_t i = l; i < XZ_PROBS_MAX; i += XZ_NL) e.probs[i] = saved[i];
            e.sync();
        }
    }
    uint32_t status = XZ_OK;
    uint32_t ci = t.c0;
    for (; ci < t.c1; ++ci) {
        const XzChunk &c = chunks[ci];
        if (c.flags & XZ_C_DICT_RESET) w.prev = 0;
        if (c.flags & XZ_C_RAW) {
            const uint8_t *s = in + c.src;
            for (uint32_t l = e.lane0(); l < e.lane1(); ++l) for (uint32_t i = l; i < c.usize; i += XZ_NL) w.o[w.pos + i] = s[i];
            w.pos += c.usize;
            w.prev = XZ_UNI(s[c.usize - 1]);
            xz_ring_load(e, w);
            continue;
        }
        if (c.flags & XZ_C_STATE_RESET) {
            n_probs = xz_n_probs(c.lc, c.lp);
            e.sync();
            for (uint32_t l = e.lane0(); l < e.lane1(); ++l) for (uint32_t i = l; i < n_probs; i += XZ_NL) e.probs[i] = 1024;
            e.sync();
            state = 0; rep[0] = rep[1] = rep[2] = rep[3] = 0;
        }
        if ((status = xz_lzma_chunk(e, in, c, w, state, rep))) break;
    }
    e.sync();
    for (uint32_t l = e.lane0(); l < e.lane1(); ++l) {
        for (uint32_t i = l; i < XZ_PROBS_MAX; i += XZ_NL) saved[i] = i < n_probs ? e.probs[i] : (uint16_t)1024;
        if (l == 0) { sv->status = status; sv->chunk = ci; sv->state = state; for (uint32_t i = 0; i < 4; ++i) sv->rep[i] = rep[i]; sv->pad = 0; }
    }
    *bad_chunk = ci;
    return status;
}

// ---- the checks ----
#define XZ_CRC64_POLY 0xC96C5795D7870F42ull
XZ_FN uint64_t xz_crc64_entry(uint32_t i) { uint64_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ XZ_CRC64_POLY : c >> 1; return c; }
XZ_FN uint32_t xz_crc32_entry(uint32_t i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1; return c; }
// a(x) * b(x) mod P, reflected; P of 32 or 64 bits in the top bits of a 64-bit word
XZ_FN uint64_t xz_gf2_mul(uint64_t a, uint64_t b, uint64_t poly, uint64_t top) {
    uint64_t p = 0;
    for (uint64_t m = top; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1) ? (b >> 1) ^ poly : b >> 1;
    }
    return p;
}
// crc * x^(8 n) mod P: crc(A || B) = shift(crc(A), |B|) ^ crc(B) (inflate_core.h's inf_crc_shift; here for both widths)
XZ_FN uint64_t xz_crc_shift(uint64_t crc, uint64_t n, bool wide) {
    const uint64_t poly = wide ? XZ_CRC64_POLY : 0xEDB88320ull, top = wide ? 1ull << 63 : 1ull << 31;
    uint64_t x = top >> 8;                                       // x^8
    for (; n; n >>= 1) {
        if (n & 1) crc = xz_gf2_mul(x, crc, poly, top);
        x = xz_gf2_mul(x, x, poly, top);
    }
    return crc;
}
// the CRC32 (wide: CRC64) of d[0, n): the lanes take stripes of ceil(n / 64) bytes, e.tab is the byte table, e.part the lanes' shares
template <class E> XZ_FN uint64_t xz_check(E &e, const uint8_t *d, uint64_t n, bool wide) {
    e.sync();
    for (uint32_t l = e.lane0(); l < e.lane1(); ++l) for (uint32_t i = l; i < 256; i += XZ_NL) e.tab[i] = wide ? xz_crc64_entry(i) : (uint64_t)xz_crc32_entry(i);
    e.sync();
    const uint64_t s = (n + XZ_NL - 1) / XZ_NL;
    for (uint32_t l = e.lane0(); l < e.lane1(); ++l) {
        const uint64_t a = l * s < n ? l * s : n, z = a + s < n ? a + s : n;
        uint64_t c = wide ? ~0ull : 0xFFFFFFFFull;
        for (uint64_t i = a; i < z; ++i) c = e.tab[(c ^ d[i]) & 0xFF] ^ (c >> 8);
        c = wide ? ~c : (~c & 0xFFFFFFFFull);
        e.part[l] = z > a ? xz_crc_shift(c, n - z, wide) : 0;    // (an empty stripe's CRC is 0)
    }
    e.sync();
    uint64_t c = 0;
    for (uint32_t i = 0; i < XZ_NL; ++i) c ^= e.part[i];
    return c;
}
