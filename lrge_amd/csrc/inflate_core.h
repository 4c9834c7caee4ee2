// inflate_core.h -- RFC 1951 (deflate) decoding: the bit reader, code-length decode, canonical-code tables and the body of
// one deflate block (inf_block: header, stored path, symbol loop), shared bit for bit by the device kernels (k_inflate.h,
// k_gzip.h; hipcc) and the host twins (inflate_twin.cpp, gzip_twin.cpp; g++) that the CPU suite checks against zlib.
// inf_raw decodes one BGZF block with it; gzip_core.h's gz_decode drives it over plain gzip.  Also the CRC-32 of a block
// computed over lane stripes and combined (the twin emulates the 64 stripes, so the combine is checked on the host too).
//
// The decoder is written once against an environment `E` that owns the output and the tables:
//   E::lane, E::nl            this lane and the lane count (twin: 0, 1)
//   E::sync()                 every lane's table writes visible to every lane (kernel: workgroup barrier of one wavefront)
//   E::lt, E::dt, E::ct       InfCode tables (kernel: LDS);  E::lens  320 code lengths (kernel: LDS)
//   E::pos, E::cap            bytes written so far / the block's ISIZE
//   E::full, E::reach()       the status when the output has no room (INF_E_OUTPUT) / the largest legal distance at pos
//   E::lit(b), E::copy(dist, len), E::stored(src, n)   output (kernel: spread over the lanes)
// Every decision is taken on values that are the same in every lane (INF_UNI makes that explicit to the compiler), so
// the bit reader and the symbol decode stay wave-uniform.
//
// Memory safety by construction: the reader never reads outside [p + start, p + end) (bits past the end read as zero
// and are counted; consuming one is an error), output never goes past `cap`, a back-reference never reaches before the
// block's first byte, and every loop is bounded by the input or output size.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define INF_FN __host__ __device__ static inline
#else
#define INF_FN static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define INF_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define INF_UNI(x) ((uint32_t)(x))
#endif

// block status words (one per BGZF block; 0 = the bytes are exact)
enum {
    INF_OK = 0,
    INF_E_BTYPE = 1,        // BTYPE 3
    INF_E_STORED = 2,       // stored block: LEN != ~NLEN, or longer than the input
    INF_E_CODES = 3,        // too many length / distance symbols, bad code-length repeat, over-subscribed or incomplete code
    INF_E_SYMBOL = 4,       // a bit pattern that is no code, length symbol 286 / 287, distance symbol 30 / 31
    INF_E_DIST = 5,         // distance before the block's first byte
    INF_E_INPUT = 6,        // compressed data ends early, or does not end where the block's deflate data ends
    INF_E_OUTPUT = 7,       // more output than ISIZE
    INF_E_SIZE = 8,         // less output than ISIZE
    INF_E_CRC = 9,          // CRC32 of the output differs from the trailer
    INF_E_NOT_RUN = 0xFFFFFFFFu,
};

#define INF_PRIM_BITS 10
#define INF_PRIM (1u << INF_PRIM_BITS)
#define INF_MAX_ISIZE 65536u

// Bit offsets of the input (inf_bitpos, inf_seek) are 32 bits wide: the caller keeps 8 * end < 2^32.
struct InfBits {
    const uint8_t *p;
    uint32_t pos, end;      // next byte to read, one past the last readable byte
    uint32_t cnt, over;     // bits held in buf; zero bits appended past the end (their consumption is an error)
    uint64_t buf;
};

// canonical code: counts per length, symbols in canonical order, and a 2^10-entry primary table (sym << 4 | len;
// 0 = a code longer than 10 bits, or no code: decoded by walking the counts)
struct InfCode {
    uint16_t count[16];
    uint16_t offs[16];
    uint16_t first[16];
    uint16_t nxt[16];       // (scratch of inf_code_prepare)
    uint16_t ncodes, pad;
    uint16_t sym[288];
    uint16_t prim[INF_PRIM];
};

INF_FN void inf_bits_init(InfBits &b, const uint8_t *p, uint32_t start, uint32_t end) {
    b.p = p; b.pos = start; b.end = end; b.cnt = 0; b.over = 0; b.buf = 0;
}

// afterwards at least 32 bits are held
INF_FN void inf_refill(InfBits &b) {
    if (b.cnt > 32) return;
    if (b.pos + 4 <= b.end) {
        const uint32_t w = INF_UNI((uint32_t)b.p[b.pos] | (uint32_t)b.p[b.pos + 1] << 8 | (uint32_t)b.p[b.pos + 2] << 16 | (uint32_t)b.p[b.pos + 3] << 24);
        b.buf |= (uint64_t)w << b.cnt; b.cnt += 32; b.pos += 4;
        return;
    }
    while (b.cnt <= 56) {
        uint32_t c = 0;
        if (b.pos < b.end) c = INF_UNI(b.p[b.pos++]); else b.over += 8;
        b.buf |= (uint64_t)c << b.cnt; b.cnt += 8;
    }
}
INF_FN bool inf_overrun(const InfBits &b) { return b.over > b.cnt; }      // a padding bit was consumed
INF_FN uint32_t inf_peek(const InfBits &b, uint32_t n) { return (uint32_t)(b.buf & ((1ull << n) - 1)); }
INF_FN void inf_drop(InfBits &b, uint32_t n) { b.buf >>= n; b.cnt -= n; }
INF_FN uint32_t inf_get(InfBits &b, uint32_t n) { const uint32_t v = inf_peek(b, n); inf_drop(b, n); return v; }

// the bit offset of the next unread bit (not past an overrun), and the reader put on a bit offset
INF_FN uint32_t inf_bitpos(const InfBits &b) { return b.pos * 8u - (b.cnt - b.over); }
INF_FN void inf_seek(InfBits &b, uint32_t bit) {
    b.pos = bit >> 3; b.cnt = 0; b.over = 0; b.buf = 0;
    inf_refill(b);
    inf_drop(b, bit & 7);
}

INF_FN uint32_t inf_rev(uint32_t c, uint32_t len) { uint32_t r = 0; for (uint32_t i = 0; i < len; ++i) { r = r << 1 | (c & 1); c >>= 1; } return r; }

// counts, canonical order and first codes (on the device every lane computes the same values and writes them alike: the
// lanes run in lockstep, so a read-modify-write of one address by all of them stores the same value once).
// `strict`: the code-length code, which must be complete; the others may be incomplete only with a single 1-bit code
// (zlib's rule), and may be empty (a decode then fails).
INF_FN int inf_code_prepare(InfCode *h, const uint8_t *lens, uint32_t n, bool strict) {
    // (the counters live in the table itself, not in a local array: on the device that would be scratch memory)
    for (uint32_t l = 0; l < 16; ++l) h->count[l] = 0;
    for (uint32_t s = 0; s < n; ++s) h->count[lens[s] & 15]++;
    h->count[0] = 0;
    int left = 1;
    uint32_t maxl = 0;
    for (uint32_t l = 1; l < 16; ++l) { const uint32_t c = INF_UNI(h->count[l]); left = left * 2 - (int)c; if (left < 0) return INF_E_CODES; if (c) maxl = l; }
    if (left > 0 && maxl != 0 && (strict || maxl != 1)) return INF_E_CODES;
    uint32_t off = 0, code = 0, prev = 0;
    for (uint32_t l = 0; l < 16; ++l) {
        const uint32_t c = INF_UNI(h->count[l]);
        h->offs[l] = (uint16_t)off; h->nxt[l] = (uint16_t)off; off += c;
        if (l) code = (code + prev) << 1;
        h->first[l] = (uint16_t)code;
        prev = c;
    }
    h->ncodes = (uint16_t)off;
    for (uint32_t s = 0; s < n; ++s) if (lens[s]) h->sym[h->nxt[lens[s]]++] = (uint16_t)s;
    return INF_OK;
}
INF_FN void inf_code_clear(InfCode *h, uint32_t lane, uint32_t nl) { for (uint32_t j = lane; j < INF_PRIM; j += nl) h->prim[j] = 0; }
INF_FN void inf_code_fill(InfCode *h, const uint8_t *lens, uint32_t lane, uint32_t nl) {
    for (uint32_t k = lane; k < h->ncodes; k += nl) {
        const uint32_t s = h->sym[k], L = lens[s];
        if (L > INF_PRIM_BITS) continue;
        const uint32_t rev = inf_rev(h->first[L] + (k - h->offs[L]), L);
        for (uint32_t j = rev; j < INF_PRIM; j += 1u << L) h->prim[j] = (uint16_t)(s << 4 | L);
    }
}

// one symbol; -1 = no code.  Needs >= 15 bits held.
INF_FN int inf_decode(InfBits &b, const InfCode *h) {
    const uint32_t e = INF_UNI(h->prim[inf_peek(b, INF_PRIM_BITS)]);
    if (e) { inf_drop(b, e & 15); return (int)(e >> 4); }
    const uint32_t bits = inf_peek(b, 15);
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len < 16; ++len) {
        code |= (bits >> (len - 1)) & 1;
        const uint32_t c = INF_UNI(h->count[len]);
        if (code - first < c) { inf_drop(b, len); return (int)INF_UNI(h->sym[index + code - first]); }
        index += c; first = (first + c) << 1; code <<= 1;
    }
    return -1;
}

INF_FN uint32_t inf_clen_order(uint32_t i) {
    switch (i) {
    case 0: return 16; case 1: return 17; case 2: return 18; case 3: return 0; case 4: return 8; case 5: return 7; case 6: return 9;
    case 7: return 6; case 8: return 10; case 9: return 5; case 10: return 11; case 11: return 4; case 12: return 12; case 13: return 3;
    case 14: return 13; case 15: return 2; case 16: return 14; case 17: return 1; default: return 15;
    }
}

template <class E> INF_FN int inf_tables_build(E &e, InfCode *h, const uint8_t *lens, uint32_t n, bool strict) {
    const int rc = inf_code_prepare(h, lens, n, strict);
    if (rc) return rc;
    inf_code_clear(h, e.lane, e.nl);
    e.sync();
    inf_code_fill(h, lens, e.lane, e.nl);
    e.sync();
    return INF_OK;
}

template <class E> INF_FN int inf_fixed(E &e) {
    for (uint32_t i = 0; i < 288; ++i) e.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    for (uint32_t i = 0; i < 32; ++i) e.lens[288 + i] = 5;     // 30 and 31 complete the code; decoding them is an error
    e.sync();
    int rc = inf_tables_build(e, e.lt, e.lens, 288, false);
    if (!rc) rc = inf_tables_build(e, e.dt, e.lens + 288, 32, false);
    return rc;
}

template <class E> INF_FN int inf_dynamic(E &e, InfBits &b) {
    inf_refill(b);
    const uint32_t nlen = inf_get(b, 5) + 257, ndist = inf_get(b, 5) + 1, ncode = inf_get(b, 4) + 4;
    if (nlen > 286 || ndist > 30) return INF_E_CODES;
    uint8_t *lens = e.lens;
    for (uint32_t i = 0; i < 19; ++i) lens[i] = 0;
    for (uint32_t i = 0; i < ncode; ++i) { inf_refill(b); lens[inf_clen_order(i)] = (uint8_t)inf_get(b, 3); }
    e.sync();
    int rc = inf_tables_build(e, e.ct, lens, 19, true);
    if (rc) return rc;
    const uint32_t total = nlen + ndist;
    uint32_t i = 0;
    while (i < total) {                                   // bounded: every step fills at least one length
        inf_refill(b);
        if (inf_overrun(b)) return INF_E_INPUT;
        const int s = inf_decode(b, e.ct);
        if (s < 0) return INF_E_SYMBOL;
        if (s < 16) { lens[i++] = (uint8_t)s; continue; }
        uint32_t rep, v = 0;
        if (s == 16) { if (i == 0) return INF_E_CODES; v = lens[i - 1]; rep = 3 + inf_get(b, 2); }
        else if (s == 17) rep = 3 + inf_get(b, 3);
        else rep = 11 + inf_get(b, 7);
        if (i + rep > total) return INF_E_CODES;
        for (uint32_t r = 0; r < rep; ++r) lens[i++] = (uint8_t)v;
    }
    if (inf_overrun(b)) return INF_E_INPUT;
    if (lens[256] == 0) return INF_E_CODES;              // no end-of-block code
    e.sync();
    rc = inf_tables_build(e, e.lt, lens, nlen, false);
    if (!rc) rc = inf_tables_build(e, e.dt, lens + nlen, ndist, false);
    return rc;
}

// One deflate block at the reader's position (header bits included): *last = BFINAL.  INF_OK or a status; the order of the
// checks decides which status a damaged stream gets.  What differs between the callers comes from E at compile time:
// E::full (the status for "no room for this output") and E::reach() (the largest legal distance at e.pos).
template <class E> INF_FN int inf_block(E &e, InfBits &b, bool *last) {
    inf_refill(b);
    if (inf_overrun(b)) return INF_E_INPUT;
    *last = inf_get(b, 1) != 0;
    const uint32_t type = inf_get(b, 2);
    if (type == 3) return INF_E_BTYPE;
    if (type == 0) {
        inf_drop(b, b.cnt & 7);                                  // to a byte boundary
        if (inf_overrun(b)) return INF_E_INPUT;
        const uint32_t q = inf_bitpos(b) >> 3;                   // LEN's byte
        if (q + 4 > b.end) return INF_E_INPUT;
        const uint8_t *h = b.p + q;
        const uint32_t len = INF_UNI((uint32_t)h[0] | (uint32_t)h[1] << 8), nlen = INF_UNI((uint32_t)h[2] | (uint32_t)h[3] << 8);
        if ((len ^ 0xFFFFu) != nlen) return INF_E_STORED;
        if (len > b.end - q - 4) return INF_E_INPUT;
        if (len > e.cap - e.pos) return E::full;
        e.stored(h + 4, len);
        inf_seek(b, 8 * (q + 4 + len));
        return INF_OK;
    }
    const int rc = type == 1 ? inf_fixed(e) : inf_dynamic(e, b);
    if (rc) return rc;
    for (uint32_t guard = 0; guard <= e.cap; ++guard) {         // every symbol but the last writes a byte
        inf_refill(b);
        if (inf_overrun(b)) return INF_E_INPUT;
        const int s = inf_decode(b, e.lt);
        if (s < 0) return INF_E_SYMBOL;
        if (s < 256) {
            if (e.pos >= e.cap) return E::full;
            e.lit((uint8_t)s);
            continue;
        }
        if (s == 256) return INF_OK;
        const uint32_t ls = (uint32_t)s - 257;
        if (ls >= 29) return INF_E_SYMBOL;
        uint32_t len;
        if (ls < 8) len = ls + 3;
        else if (ls == 28) len = 258;
        else { const uint32_t x = (ls - 8) >> 2, eb = x + 1; len = 3 + (1u << (eb + 2)) + (((ls - 8) & 3) << eb) + inf_get(b, eb); }
        inf_refill(b);
        const int ds = inf_decode(b, e.dt);
        if (ds < 0 || ds >= 30) return INF_E_SYMBOL;
        uint32_t dist;
        if (ds < 4) dist = (uint32_t)ds + 1;
        else { const uint32_t eb = ((uint32_t)ds >> 1) - 1; dist = 1 + ((2u + ((uint32_t)ds & 1)) << eb) + inf_get(b, eb); }
        if (inf_overrun(b)) return INF_E_INPUT;
        if (dist > e.reach()) return INF_E_DIST;
        if (len > e.cap - e.pos) return E::full;
        e.copy(dist, len);
    }
    return E::full;                                              // (the guard: more symbols than the output holds)
}

// The raw deflate stream of one block: input [start, end) of p, output through e.  The stream must end exactly at `end`
// (up to the last byte's padding bits), like a gzip member whose trailer follows.
template <class E> INF_FN int inf_raw(E &e, const uint8_t *p, uint32_t start, uint32_t end) {
    InfBits b;
    inf_bits_init(b, p, start, end);
    const uint32_t max_blocks = (end - start) * 8u / 3u + 1u;      // every deflate block takes at least 3 bits
    bool last = false;
    for (uint32_t blk = 0; blk < max_blocks && !last; ++blk) {
        const int rc = inf_block(e, b, &last);
        if (rc) return rc;
    }
    if (!last) return INF_E_INPUT;
    if (inf_overrun(b)) return INF_E_INPUT;
    if ((inf_bitpos(b) + 7) >> 3 != end) return INF_E_INPUT;       // bytes consumed, the last one's padding bits included
    if (e.pos != e.cap) return INF_E_SIZE;
    return INF_OK;
}

// ---- CRC-32 (reflected, 0xEDB88320) over lane stripes ----
#define INF_CRC_POLY 0xEDB88320u
INF_FN uint32_t inf_crc_entry(uint32_t i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ INF_CRC_POLY : c >> 1; return c; }
INF_FN void inf_crc_table(uint32_t *t, uint32_t lane, uint32_t nl) { for (uint32_t i = lane; i < 256; i += nl) t[i] = inf_crc_entry(i); }
// standard CRC-32 (init and final xor ~0) of n bytes
INF_FN uint32_t inf_crc(const uint32_t *t, const uint8_t *d, uint32_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) c = t[(c ^ d[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}
// a(x) * b(x) mod P, reflected (zlib's multmodp)
INF_FN uint32_t inf_gf2_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1) ? (b >> 1) ^ INF_CRC_POLY : b >> 1;
    }
    return p;
}
// crc * x^(8 n) mod P: the CRC of A moved past n more bytes.  crc(A || B) = inf_crc_shift(crc(A), |B|) ^ crc(B), so the
// CRC of the stripes S_0 .. S_k is the XOR over i of inf_crc_shift(crc(S_i), bytes after S_i).
// The byte count is 64 bits wide for gzip members above 4 GiB; a block's stripes stay below 17 steps (n <= 65536).
INF_FN uint32_t inf_crc_shift(uint32_t crc, uint64_t n) {
    uint32_t x = 1u << 23;                                       // x^8
    for (; n; n >>= 1) {
        if (n & 1) crc = inf_gf2_mul(x, crc);
        x = inf_gf2_mul(x, x);
    }
    return crc;
}
// lane `lane`'s share of the block's CRC (stripes of ceil(n / nl) bytes); the XOR of every lane's value is the CRC
INF_FN uint32_t inf_crc_stripe(const uint32_t *t, const uint8_t *d, uint32_t n, uint32_t lane, uint32_t nl) {
    const uint32_t s = (n + nl - 1) / nl;
    const uint32_t a = lane * s < n ? lane * s : n, z = a + s < n ? a + s : n;
    return inf_crc_shift(inf_crc(t, d + a, z - a), n - z);
}
