// bz_core.h -- the bit-level rules of one bzip2 stream: the MSB-first bit reader, the two 48-bit magics, the entropy decode of
// one block (symbol map, selectors, delta-coded code lengths, canonical tables, Huffman + move-to-front + RUNA/RUNB into the BWT
// column L), the inverse BWT (counting scatter into packed links, the walk), the run-length layer in front of the BWT ("RLE1":
// four equal bytes, then a count byte), bzip2's CRC (MSB first, polynomial 0x04c11db7), and the marks at which a block's walk and
// run-length layer can be entered again with the seeded decode of one segment.  Compiled by hipcc (k_bzip2.h) and g++
// (bz_twin.h) alike; written from the format's description.
//
// The block decode is written for one wavefront with wavefront-uniform control: every lane walks the same bits and takes the
// same branches; `lane` / `nl` spread the loops that have independent iterations (table build, move-to-front shift, run fill)
// and sync() separates a step that writes shared tables from the one that reads them.  The twin runs it with nl = 1.
//
// Every loop is bounded by a maximum of the format: BZ_MAX_SELECTORS selectors of BZ_GROUP symbols, `bs` bytes of L (the level's
// block size), BZ_MAX_CODE bits per code, the input's length.  A start that is no block ends with a status.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define BZ_FN __host__ __device__ static inline
#define BZ_MEM __host__ __device__
#else
#define BZ_FN static inline
#define BZ_MEM
#endif
#ifdef __clang__
#define BZ_UNROLL _Pragma("unroll")
#else
#define BZ_UNROLL
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define BZ_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define BZ_UNI(x) ((uint32_t)(x))
#endif

enum {
    BZ_OK = 0,
    BZ_E_MAGIC = 1,         // no "BZh1".."BZh9" stream header, or no block magic at the start of a block
    BZ_E_INPUT = 2,         // the input ends inside the block or the stream trailer
    BZ_E_RANDOMISED = 3,    // the block's randomised bit is set (bzip2 0.9.0 and older)
    BZ_E_GROUPS = 4,        // nGroups outside 2..6, no selector or more than BZ_MAX_SELECTORS, no symbol in use
    BZ_E_SELECTOR = 5,      // a selector names a table the block does not have
    BZ_E_LENGTH = 6,        // a code length outside 1..20
    BZ_E_CODE = 7,          // bits that are no code of the table
    BZ_E_SIZE = 8,          // more bytes than the level's block size
    BZ_E_NO_EOB = 9,        // the selectors ran out before the end-of-block symbol
    BZ_E_ORIGPTR = 10,      // origPtr >= n (an empty block included)
    BZ_E_BLOCK_CRC = 11,    // the block's bytes do not give its stored CRC
    BZ_E_STREAM_CRC = 12,   // the combined CRC differs
    BZ_E_TRAILING = 13,     // bytes behind the stream (a second stream included)
    BZ_E_CHAIN = 14,        // a block ends where neither a block nor the end of the stream starts
    BZ_E_RUN = 15,          // a block stops behind four equal bytes, where their count byte belongs (libbz2 gives an error)
    BZ_E_ENTRY = 16,        // a block entered at its marks (bz_segment) does not arrive where the seek map says
};

#define BZ_BLOCK_MAGIC 0x314159265359ull
#define BZ_END_MAGIC 0x177245385090ull
#define BZ_END_FLAG (1ull << 63)      // a candidate of the finder: bit 63 set = the end-of-stream magic
#define BZ_MAX_SELECTORS 18002u
#define BZ_MAX_CODE 20u
#define BZ_GROUP 50u
#define BZ_ALPHA 258u
#define BZ_TABS 6u
#define BZ_LSTRIDE (BZ_MAX_CODE + 2)  // limit / base entries per table
#define BZ_PAD 64u                    // bytes readable behind the compressed input on the device (zeros)

// ---- bits, MSB first ----
// bytes [q, q + 8) as one big-endian word, zero past the end
BZ_FN uint64_t bz_be64(const uint8_t *p, uint64_t n, uint64_t q) {
    uint64_t w = 0;
    if (q + 8 <= n) {
        __builtin_memcpy(&w, p + q, 8);
        return __builtin_bswap64(w);
    }
    for (uint32_t i = 0; i < 8; ++i) w = w << 8 | (q + i < n ? p[q + i] : 0u);
    return w;
}

struct BzBits {
    const uint8_t *p;
    uint64_t n, pos;        // bytes of input, the next bit
    uint64_t w, wq;         // bytes [wq, wq + 8) of the input
};
BZ_FN void bz_bits_init(BzBits &b, const uint8_t *p, uint64_t n, uint64_t pos) { b.p = p; b.n = n; b.pos = pos; b.wq = pos >> 3; b.w = bz_be64(p, n, b.wq); }
// the 32 bits at the reader's position, zero past the end
BZ_FN uint32_t bz_peek32(BzBits &b) {
    const uint64_t q = b.pos >> 3;
    if (q < b.wq || q > b.wq + 3) { b.wq = q; b.w = bz_be64(b.p, b.n, q); }
    const uint32_t used = (uint32_t)(b.pos - 8 * b.wq);           // 0..31
    return (uint32_t)(b.w >> (32 - used));
}
// k bits, 1 <= k <= 32 (past the end: zeros; the caller checks bz_over)
BZ_FN uint32_t bz_get(BzBits &b, uint32_t k) { const uint32_t v = bz_peek32(b) >> (32 - k); b.pos += k; return BZ_UNI(v); }
BZ_FN bool bz_over(const BzBits &b) { return b.pos > 8 * b.n; }

// what starts at shift s (0..7) of the 8 big-endian bytes w: 1 the block magic, 2 the end-of-stream magic, 0 neither
BZ_FN uint32_t bz_magic_in(uint64_t w, uint32_t s) {
    const uint64_t v = (w << s) >> 16;
    return v == BZ_BLOCK_MAGIC ? 1u : v == BZ_END_MAGIC ? 2u : 0u;
}

// ---- CRC ----
BZ_FN uint32_t bz_crc_entry(uint32_t i) { uint32_t c = i << 24; for (int k = 0; k < 8; ++k) c = (c & 0x80000000u) ? (c << 1) ^ 0x04c11db7u : c << 1; return c; }
BZ_FN void bz_crc_table(uint32_t *t, uint32_t lane, uint32_t nl) { for (uint32_t i = lane; i < 256; i += nl) t[i] = bz_crc_entry(i); }
BZ_FN uint32_t bz_rotl1(uint32_t c) { return c << 1 | c >> 31; }

// ---- the entropy decode of one block ----
// the tables of one block (LDS on the device)
struct BzTabs {
    int32_t limit[BZ_TABS * BZ_LSTRIDE], base[BZ_TABS * BZ_LSTRIDE];
    uint32_t cnt[256];                      // bytes of L by value
    uint16_t perm[BZ_TABS * BZ_ALPHA];
    uint8_t len[BZ_TABS * BZ_ALPHA];
    uint8_t minl[8], maxl[8];
    uint16_t npp[8];
    uint8_t mtf[256];                       // the move-to-front list, as byte values
    uint8_t sel[BZ_MAX_SELECTORS + 2];
};
// the result of one block decode
struct BzRes { uint64_t end_bit; uint32_t status, n, orig, crc; };

// E: BzTabs *t; uint32_t lane, nl; void sync(); static constexpr uint32_t PER (>= 256 / nl)
// index idx (>= 1) of the list moves to the front; returns its byte
template <class E> BZ_FN uint32_t bz_mtf_front(E &e, uint32_t idx) {
    uint8_t *m = e.t->mtf;
    const uint32_t b = m[idx];
    uint8_t keep[E::PER];
BZ_UNROLL
    for (uint32_t k = 0; k < E::PER; ++k) { const uint32_t j = e.lane + k * e.nl; if (j > idx) break; keep[k] = j ? m[j - 1] : (uint8_t)b; }
    e.sync();
BZ_UNROLL
    for (uint32_t k = 0; k < E::PER; ++k) { const uint32_t j = e.lane + k * e.nl; if (j > idx) break; m[j] = keep[k]; }
    e.sync();
    return BZ_UNI(b);
}

// the canonical decode table of coding table g from its lengths: for a code of i bits, value v: v <= limit[i] says the code
// ends here, perm[v - base[i]] is its symbol
BZ_FN void bz_make_table(BzTabs *t, uint32_t g, uint32_t alpha) {
    const uint8_t *len = t->len + g * BZ_ALPHA;
    uint16_t *perm = t->perm + g * BZ_ALPHA;
    int32_t *limit = t->limit + g * BZ_LSTRIDE, *base = t->base + g * BZ_LSTRIDE;
    uint32_t lo = BZ_MAX_CODE, hi = 1;
    for (uint32_t i = 0; i < alpha; ++i) { lo = len[i] < lo ? len[i] : lo; hi = len[i] > hi ? len[i] : hi; }
    int32_t vec = 0;
    uint32_t pp = 0;
    for (uint32_t i = lo; i <= hi; ++i) {
        base[i] = vec - (int32_t)pp;
        for (uint32_t s = 0; s < alpha; ++s) if (len[s] == i) perm[pp++] = (uint16_t)s;
        limit[i] = base[i] + (int32_t)pp - 1;
        vec = (limit[i] + 1) << 1;
    }
    t->minl[g] = (uint8_t)lo; t->maxl[g] = (uint8_t)hi; t->npp[g] = (uint16_t)pp;
}

// One block from bit `start` of p[0, n): the bytes of the BWT column into L (at most bs), their counts into e.t->cnt.
// r.end_bit: the bit behind the end-of-block symbol.  r.status != BZ_OK: nothing else of r counts.
template <class E> BZ_FN void bz_decode_block(E &e, const uint8_t *p, uint64_t n, uint64_t start, uint32_t bs, uint8_t *L, BzRes &r) {
    BzTabs *t = e.t;
    BzBits b;
    bz_bits_init(b, p, n, start);
    r.end_bit = start; r.n = 0; r.orig = 0; r.crc = 0;
#define BZ_FAIL(s) do { r.status = (s); return; } while (0)
    if (bz_get(b, 24) != (uint32_t)(BZ_BLOCK_MAGIC >> 24) || bz_get(b, 24) != (uint32_t)(BZ_BLOCK_MAGIC & 0xFFFFFF)) BZ_FAIL(BZ_E_MAGIC);
    r.crc = bz_get(b, 32);
    if (bz_get(b, 1)) BZ_FAIL(BZ_E_RANDOMISED);
    r.orig = bz_get(b, 24);
    // the symbol map: 16 ranges of 16 byte values
    const uint32_t ranges = bz_get(b, 16);
    uint32_t in_use = 0;
    for (uint32_t i = 0; i < 16; ++i) {
        if (!(ranges >> (15 - i) & 1)) continue;
        const uint32_t bits = bz_get(b, 16);
        for (uint32_t j = 0; j < 16; ++j) if (bits >> (15 - j) & 1) { if (e.lane == 0) t->mtf[in_use] = (uint8_t)(16 * i + j); ++in_use; }
    }
    for (uint32_t i = e.lane; i < 256; i += e.nl) t->cnt[i] = 0;
    if (bz_over(b)) BZ_FAIL(BZ_E_INPUT);
    if (in_use == 0) BZ_FAIL(BZ_E_GROUPS);
    const uint32_t alpha = in_use + 2, eob = in_use + 1;
    const uint32_t groups = bz_get(b, 3), n_sel = bz_get(b, 15);
    if (groups < 2 || groups > BZ_TABS || n_sel < 1 || n_sel > BZ_MAX_SELECTORS) BZ_FAIL(BZ_E_GROUPS);
    // the selectors: unary positions in a move-to-front list of the tables
    {
        uint32_t order = 0x543210;                                  // four bits per entry, the front in the low bits
        for (uint32_t i = 0; i < n_sel; ++i) {
            uint32_t j = 0;
            while (j < groups && bz_get(b, 1)) ++j;
            if (j >= groups) BZ_FAIL(BZ_E_SELECTOR);
            const uint32_t g = order >> (4 * j) & 15, low = order & ((1u << (4 * j)) - 1);
            order = (order & ~((1u << (4 * j + 4)) - 1)) | low << 4 | g;
            if (e.lane == 0) t->sel[i] = (uint8_t)g;
            if (bz_over(b)) BZ_FAIL(BZ_E_INPUT);
        }
    }
    // the code lengths, delta coded
    for (uint32_t g = 0; g < groups; ++g) {
        uint32_t cur = bz_get(b, 5);
        for (uint32_t i = 0; i < alpha; ++i) {
            for (;;) {
                if (cur < 1 || cur > BZ_MAX_CODE) BZ_FAIL(BZ_E_LENGTH);
                if (!bz_get(b, 1)) break;
                cur = bz_get(b, 1) ? cur - 1 : cur + 1;
                if (bz_over(b)) BZ_FAIL(BZ_E_INPUT);
            }
            if (e.lane == 0) t->len[g * BZ_ALPHA + i] = (uint8_t)cur;
        }
    }
    if (bz_over(b)) BZ_FAIL(BZ_E_INPUT);
    e.sync();
    for (uint32_t g = e.lane; g < groups; g += e.nl) bz_make_table(t, g, alpha);
    e.sync();
    // the symbols, in groups of BZ_GROUP under one table each
    uint32_t grp = 0, left = 0, nb = 0, run = 0, weight = 1;
    const int32_t *limit = t->limit, *base = t->base;
    const uint16_t *perm = t->perm;
    uint32_t lo = 1, hi = 1, npp = 0;
    for (;;) {
        if (left == 0) {
            if (grp >= n_sel) BZ_FAIL(BZ_E_NO_EOB);
            const uint32_t g = BZ_UNI(t->sel[grp++]);
            left = BZ_GROUP;
            limit = t->limit + g * BZ_LSTRIDE; base = t->base + g * BZ_LSTRIDE; perm = t->perm + g * BZ_ALPHA;
            lo = BZ_UNI(t->minl[g]); hi = BZ_UNI(t->maxl[g]); npp = BZ_UNI(t->npp[g]);
        }
        --left;
        const uint32_t w = BZ_UNI(bz_peek32(b));
        uint32_t zn = lo;
        while (zn <= hi && (int32_t)(w >> (32 - zn)) > (int32_t)BZ_UNI(limit[zn])) ++zn;
        if (zn > hi) BZ_FAIL(BZ_E_CODE);
        const uint32_t at = (w >> (32 - zn)) - BZ_UNI(base[zn]);
        if (at >= npp) BZ_FAIL(BZ_E_CODE);
        const uint32_t sym = BZ_UNI(perm[at]);
        b.pos += zn;
        if (bz_over(b)) BZ_FAIL(BZ_E_INPUT);
        if (sym <= 1) {                                             // RUNA / RUNB: the run length in bijective base 2
            run += weight << sym;
            weight <<= 1;
            if (run > bs) BZ_FAIL(BZ_E_SIZE);                       // (weight <= 2 bs: no overflow)
            continue;
        }
        if (run) {
            if (nb + run > bs) BZ_FAIL(BZ_E_SIZE);
            const uint32_t v = BZ_UNI(t->mtf[0]);
            for (uint32_t j = e.lane; j < run; j += e.nl) L[nb + j] = (uint8_t)v;
            if (e.lane == 0) t->cnt[v] += run;
            nb += run; run = 0; weight = 1;
        }
        if (sym == eob) break;
        if (nb >= bs) BZ_FAIL(BZ_E_SIZE);
        const uint32_t v = bz_mtf_front(e, sym - 1);
        if (e.lane == 0) { L[nb] = (uint8_t)v; t->cnt[v] += 1; }
        ++nb;
    }
    e.sync();
    if (r.orig >= nb) BZ_FAIL(BZ_E_ORIGPTR);
    r.n = nb; r.end_bit = b.pos; r.status = BZ_OK;
#undef BZ_FAIL
}

// ---- the inverse BWT ----
// tt[j] = i << 8 | c for the j-th byte c of the sorted column, which is byte i of L (stable): one word per step of the walk
BZ_FN void bz_scatter(const uint8_t *L, uint32_t n, const uint32_t *cnt, uint32_t *tt) {
    uint32_t cf[256], a = 0;
    for (uint32_t c = 0; c < 256; ++c) { cf[c] = a; a += cnt[c]; }
    for (uint32_t i = 0; i < n; ++i) { const uint32_t at = cf[L[i]]++; if (at < n) tt[at] = i << 8 | L[i]; }
}

// bytes to consecutive addresses, stored four at a time wherever a whole aligned word is written
struct BzOut { uint8_t *p; uint32_t acc, have; };
BZ_FN void bz_out_flush(BzOut &o) {
    if (o.have == 4) __builtin_memcpy(__builtin_assume_aligned(o.p - 4, 4), &o.acc, 4);
    else for (uint32_t i = 0; i < o.have; ++i) (o.p - o.have)[i] = (uint8_t)(o.acc >> (8 * i));
    o.acc = 0; o.have = 0;
}
BZ_FN void bz_out_put(BzOut &o, uint32_t c) {
    o.acc |= c << (8 * o.have);
    ++o.have; ++o.p;
    if (((uintptr_t)o.p & 3) == 0) bz_out_flush(o);
}

// ---- marks: where a block can be entered ----
// A block of n bytes in front of the run-length layer is cut into BZ_MARKS segments of bz_seg(n) steps of the walk.  Mark j stands in
// front of step p_j = j * seg, for p_j < n, and holds what a decode needs to start there: the walk pointer `at`, the state of the
// run-length layer before pre[p_j] is consumed (prev | run << 16; run == 4: pre[p_j] is a count byte), the text bytes pre[0, p_j)
// gave and the running CRC register there.  A census that leaves a seek map records them on its one walk (the sinks below)
#define BZ_MARKS 64u
struct BzMark { uint32_t at, state, off, crc; };
BZ_FN uint32_t bz_seg(uint32_t n) { const uint32_t s = 4 * ((n + 255) / 256); return s < 4 ? 4u : s; }
BZ_FN uint32_t bz_mark_count(uint32_t n) { const uint32_t s = bz_seg(n); return (n + s - 1) / s; }      // the marks a block has (the other slots stay zero)
// the sink a decode without a map passes: nothing is kept, nothing is compiled in
struct BzNoMarks {
    BZ_FN void walk(uint32_t, uint32_t) {}
    BZ_FN void rle(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) {}
};
// the recording sink: m[0, BZ_MARKS) of one block, step `next` is mark j's
struct BzMarkRec {
    BzMark *m; uint32_t seg, j, next;
    BZ_MEM BzMarkRec(BzMark *m_, uint32_t n) : m(m_), seg(bz_seg(n)), j(0), next(0) {}
    BZ_MEM void walk(uint32_t i, uint32_t at) { if (i == next) { m[j++].at = at; next += seg; } }
    BZ_MEM void rle(uint32_t i, uint32_t prev, uint32_t run, uint32_t off, uint32_t crc) {
        if (i == next) { BzMark &k = m[j++]; k.state = prev | run << 16; k.off = off; k.crc = crc; next += seg; }
    }
};

// n steps from orig: the block's bytes in front of the run-length layer.  False: a link leaves the block (tt is not a scatter's)
template <class M> BZ_FN bool bz_walk(const uint32_t *tt, uint32_t n, uint32_t orig, uint8_t *pre, M &&mk) {
    BzOut o{pre, 0, 0};
    uint32_t at = orig;
    for (uint32_t i = 0; i < n; ++i) {
        if (at >= n) return false;
        mk.walk(i, at);
        const uint32_t e = tt[at];
        bz_out_put(o, e & 255);
        at = e >> 8;
    }
    bz_out_flush(o);
    return true;
}
BZ_FN bool bz_walk(const uint32_t *tt, uint32_t n, uint32_t orig, uint8_t *pre) { return bz_walk(tt, n, orig, pre, BzNoMarks()); }

// ---- the run-length layer: four equal bytes, then a count byte of 0..255 more of them ----
struct BzRle { uint32_t prev, run; };                               // the last byte (256: none) and how often it stands
#define BZ_RUN_OPEN (1ull << 63)
// the length of the text of pre[0, n); | BZ_RUN_OPEN when pre stops where a count byte belongs
BZ_FN uint64_t bz_rle_len(const uint8_t *pre, uint32_t n) {
    BzRle s{256, 0};
    uint64_t k = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = pre[i];
        if (s.run == 4) { k += c; s.run = 0; s.prev = 256; continue; }
        if (c == s.prev) ++s.run; else { s.prev = c; s.run = 1; }
        ++k;
    }
    return s.run == 4 ? k | BZ_RUN_OPEN : k;
}
// the text to out; returns its CRC
template <class M> BZ_FN uint32_t bz_rle_write(const uint8_t *pre, uint32_t n, const uint32_t *crc_tab, uint8_t *out, M &&mk) {
    BzRle s{256, 0};
    BzOut o{out, 0, 0};
    uint32_t crc = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = pre[i];
        mk.rle(i, s.prev, s.run, (uint32_t)(o.p - out), crc);
        if (s.run == 4) {
            for (uint32_t j = 0; j < c; ++j) { bz_out_put(o, s.prev); crc = crc << 8 ^ crc_tab[crc >> 24 ^ s.prev]; }
            s.run = 0; s.prev = 256;
            continue;
        }
        if (c == s.prev) ++s.run; else { s.prev = c; s.run = 1; }
        bz_out_put(o, c);
        crc = crc << 8 ^ crc_tab[crc >> 24 ^ c];
    }
    bz_out_flush(o);
    return ~crc;
}
BZ_FN uint32_t bz_rle_write(const uint8_t *pre, uint32_t n, const uint32_t *crc_tab, uint8_t *out) { return bz_rle_write(pre, n, crc_tab, out, BzNoMarks()); }

// ---- the seeded decode of one segment (k_bz_marks_text; the twin runs the same body lane by lane) ----
// From mark `mk`, `steps` steps of the walk through tt[0, n), every byte fed straight through the run-length layer and the CRC into
// the block's text at out + mk.off; the bytes in front of the run-length layer are never stored.  `lim`: the text offset the segment
// must not pass (the next mark's, the block's length behind the last).  *end: where the segment arrived, for the caller's
// comparison with the next mark.  False: a link leaves the block, or the text would pass lim -- nothing was loaded from tt at an
// index >= n, nothing stored outside out[mk.off, lim)
BZ_FN bool bz_segment(const uint32_t *tt, uint32_t n, const BzMark &mk, uint32_t steps, const uint32_t *crc_tab, uint8_t *out, uint32_t lim, BzMark *end) {
    uint32_t at = mk.at, prev = mk.state & 0xFFFFu, run = mk.state >> 16, off = mk.off, crc = mk.crc;
    bool good = off <= lim;
    BzOut o{out + off, 0, 0};
    for (uint32_t i = 0; good && i < steps; ++i) {
        if (at >= n) { good = false; break; }
        const uint32_t e = tt[at], c = e & 255;
        at = e >> 8;
        if (run == 4) {
            if (c > lim - off) { good = false; break; }
            for (uint32_t j = 0; j < c; ++j) { bz_out_put(o, prev & 255); crc = crc << 8 ^ crc_tab[crc >> 24 ^ (prev & 255)]; }
            off += c; run = 0; prev = 256;
            continue;
        }
        if (off >= lim) { good = false; break; }
        if (c == prev) ++run; else { prev = c; run = 1; }
        bz_out_put(o, c);
        crc = crc << 8 ^ crc_tab[crc >> 24 ^ c];
        ++off;
    }
    bz_out_flush(o);
    end->at = at; end->state = prev | run << 16; end->off = off; end->crc = crc;
    return good;
}
// lane j of a block of n bytes (text length len, origPtr orig, stored CRC crc) whose marks are m[0, BZ_MARKS): its segment, and the
// comparison at its end -- with mark j + 1, or behind the last segment with origPtr, the text length, a closed run and the stored CRC.
// True: the segment's text stands and continues into the next
BZ_FN bool bz_segment_lane(const uint32_t *tt, uint32_t n, uint32_t orig, uint32_t crc, uint32_t len, const BzMark *m, uint32_t j, const uint32_t *crc_tab, uint8_t *out) {
    const uint32_t seg = bz_seg(n), p = j * seg;
    if (p >= n) return true;                                         // an idle lane
    const bool last = p + seg >= n;
    const BzMark mk = m[j];
    BzMark want, got;
    if (last) { want.at = orig; want.off = len; want.crc = ~crc; want.state = 0; }
    else want = m[j + 1];
    if (mk.off > want.off || want.off > len) return false;
    if (!bz_segment(tt, n, mk, last ? n - p : seg, crc_tab, out, want.off, &got)) return false;
    if (last) return got.at == want.at && got.off == want.off && got.crc == want.crc && (got.state >> 16) != 4;
    return got.at == want.at && got.off == want.off && got.crc == want.crc && got.state == want.state;
}
