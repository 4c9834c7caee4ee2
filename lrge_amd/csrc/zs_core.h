// zs_core.h -- the bit-level rules of Zstandard (RFC 8878): the forward reader of the FSE table descriptions and the backward
// reader of the entropy streams, the FSE decode table, the Huffman description (direct and FSE-compressed weights) and its table,
// the literals and sequences headers, the literal streams, the sequence stream with the block's repeat-offset transfer function,
// the execution of a block's sequences with deferred sources, the ordered resolve of those and XXH64.  Compiled by hipcc
// (k_zstd.h) and g++ (zs_twin.cpp) alike; written from the format's description.
//
// Every function that runs as a wavefront takes an environment E: lane0() / lane1() bound the lanes the caller stands for (one
// on the device, all 64 in the twin, which therefore walks the same 64-byte steps), slot(i) names a lane's private temporary,
// sync() separates a step that writes shared state from one that reads it, and e.t is the block's tables (LDS on the device).
// Every index that comes from the stream is bounded before use; damage gives a ZS_E_* status.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define ZS_FN __host__ __device__ static inline
#else
#define ZS_FN static inline
#endif

enum {
    ZS_OK = 0,
    ZS_E_MAGIC = 1,          // neither a frame nor a skippable frame where one must start (bytes behind the last frame included)
    ZS_E_INPUT = 2,          // the file ends inside a frame or a block
    ZS_E_RESERVED = 3,       // a reserved bit is set (frame header descriptor, sequence modes)
    ZS_E_DICT = 4,           // a dictionary ID other than 0
    ZS_E_WINDOW = 5,         // a window above 2^27 bytes
    ZS_E_BLOCK_TYPE = 6,     // block type 3
    ZS_E_BLOCK_SIZE = 7,     // a block, its literals or its output above Block_Maximum_Size; a compressed block below 3 bytes
    ZS_E_LIT_HEADER = 8,     // a literals section that does not fit its block, or compressed literals of no byte
    ZS_E_ACCURACY = 9,       // an accuracy log above the format's limit
    ZS_E_FSE = 10,           // an FSE table description that does not sum up, or names too many symbols
    ZS_E_WEIGHTS = 11,       // Huffman weights that do not sum to a power of two, above 11 bits, or without two of weight 1
    ZS_E_BITSTREAM = 12,     // a bitstream without its end mark, or not consumed exactly
    ZS_E_NO_TABLE = 13,      // treeless literals or a repeat mode with nothing in front of it in the frame
    ZS_E_SYMBOL = 14,        // an RLE mode symbol, or a decoded code, above the largest of its alphabet
    ZS_E_LITERALS = 15,      // the sequences ask for more literals than the block has
    ZS_E_OFFSET = 16,        // an offset of 0, beyond the bytes the frame has produced, or beyond the window
    ZS_E_CONTENT_SIZE = 17,  // the frame's text is not of its Frame_Content_Size
    ZS_E_CHECKSUM = 18,      // the frame's text does not give its stored checksum
    ZS_E_SEQ_HEADER = 19,    // a sequences section that does not fit its block, or bytes behind Number_of_Sequences == 0
    ZS_E_TOO_BIG = 20,       // the text does not fit the device budget (no damage)
};

#define ZS_BLOCK_MAX 131072u
#define ZS_WINDOW_MAX (1u << 27)
#define ZS_HUF_LOG_MAX 11u
#define ZS_LL_LOG_MAX 9u
#define ZS_OF_LOG_MAX 8u
#define ZS_ML_LOG_MAX 9u
#define ZS_LL_SYMS 36u
#define ZS_OF_SYMS 32u
#define ZS_ML_SYMS 53u
#define ZS_PAD 64u               // bytes readable behind the compressed input on the device (zeros)
#define ZS_NL 64u                // lanes of a wavefront: the step of the literal and match copies

ZS_FN uint32_t zs_hibit(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }   // v > 0
ZS_FN uint32_t zs_le16(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8; }
ZS_FN uint32_t zs_le24(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16; }
ZS_FN uint32_t zs_le32(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
ZS_FN uint64_t zs_le64(const uint8_t *p) { return zs_le32(p) | (uint64_t)zs_le32(p + 4) << 32; }

// k (<= 32) bits at bit `at` (may be negative) of the little-endian number p[0, n): bits outside it are zero
ZS_FN uint32_t zs_bits_at(const uint8_t *p, uint32_t n, int64_t at, uint32_t k) {
    if (k == 0) return 0;
    uint32_t lead = 0;
    if (at < 0) {                                     // the low -at bits of the field lie in front of the stream
        if (-at >= (int64_t)k) return 0;
        lead = (uint32_t)-at; k -= lead; at = 0;
    }
    const uint64_t q = (uint64_t)at >> 3;
    uint64_t w = 0;
    for (uint32_t i = 0; i < 6; ++i) if (q + i < n) w |= (uint64_t)p[q + i] << (8 * i);
    const uint32_t v = (uint32_t)((w >> (at & 7)) & ((1ull << k) - 1));
    return v << lead;
}

// ---- a backward stream: p[0, n), read from the bit under the end mark of its last byte down to bit 0 ----
// (the reader keeps eight bytes of the stream in a register and loads again only when a field leaves them: one load per 32 to 64
// bits instead of one per field)
struct ZsBack { const uint8_t *p; uint32_t n; int64_t pos, wq; uint64_t w; };      // pos: bits left (negative: read past the start); w: bytes [wq, wq + 8)
// bytes [q, q + 8) of p[0, n) as a little-endian word, zero outside
ZS_FN uint64_t zs_word_at(const uint8_t *p, uint32_t n, int64_t q) {
    uint64_t w = 0;
    if (q >= 0 && q + 8 <= (int64_t)n) { __builtin_memcpy(&w, p + q, 8); return w; }
    for (int64_t i = 0; i < 8; ++i) if (q + i >= 0 && q + i < (int64_t)n) w |= (uint64_t)p[q + i] << (8 * i);
    return w;
}
ZS_FN bool zs_back_init(ZsBack &b, const uint8_t *p, uint32_t n) {
    b.p = p; b.n = n; b.pos = 0; b.wq = 0; b.w = 0;
    if (n == 0 || p[n - 1] == 0) return false;
    b.pos = (int64_t)8 * (n - 1) + zs_hibit(p[n - 1]);
    b.wq = (int64_t)n - 8; b.w = zs_word_at(p, n, b.wq);
    return true;
}
// the k (<= 32) bits under the reader's position; bits in front of the stream are zero
ZS_FN uint32_t zs_back_peek(ZsBack &b, uint32_t k) {
    if (k == 0) return 0;
    const int64_t at = b.pos - k;
    if (at < 8 * b.wq || at + k > 8 * b.wq + 64) {
        b.wq = ((at + k + 7) >> 3) - 8;             // (the field at the top of the word: the fields below it are in it too)
        b.w = zs_word_at(b.p, b.n, b.wq);
    }
    return (uint32_t)((b.w >> (at - 8 * b.wq)) & ((1ull << k) - 1));
}
ZS_FN uint32_t zs_back_get(ZsBack &b, uint32_t k) { const uint32_t v = zs_back_peek(b, k); b.pos -= k; return v; }

// ---- FSE ----
struct ZsFse { uint16_t base; uint8_t sym, nb; };                  // one state: its symbol, the bits to read, the next state's base

// the table description at p[0, n) for an alphabet of max_syms symbols and at most max_log bits: norm[] (-1: "less than 1"),
// *log, *used bytes.  ZS_OK or a status
ZS_FN uint32_t zs_fse_read(const uint8_t *p, uint32_t n, uint32_t max_log, uint32_t max_syms, int16_t *norm, uint32_t *log, uint32_t *used) {
    if (n == 0) return ZS_E_FSE;
    int64_t at = 0;
    const uint32_t al = zs_bits_at(p, n, at, 4) + 5; at += 4;
    if (al > max_log) return ZS_E_ACCURACY;
    int32_t rem = 1 << al;
    uint32_t s = 0;
    while (rem > 0 && s < max_syms) {
        const uint32_t bits = zs_hibit((uint32_t)rem + 1) + 1;
        uint32_t v = zs_bits_at(p, n, at, bits); at += bits;
        const uint32_t low = (1u << (bits - 1)) - 1, thr = (1u << bits) - 1 - ((uint32_t)rem + 1);
        if ((v & low) < thr) { --at; v &= low; }
        else if (v > low) v -= thr;
        const int32_t pr = (int32_t)v - 1;
        rem -= pr < 0 ? -pr : pr;
        if (rem < 0) return ZS_E_FSE;
        norm[s++] = (int16_t)pr;
        if (pr == 0) {
            for (;;) {
                if (at > (int64_t)8 * n) return ZS_E_FSE;
                const uint32_t r = zs_bits_at(p, n, at, 2); at += 2;
                for (uint32_t i = 0; i < r; ++i) { if (s >= max_syms) return ZS_E_FSE; norm[s++] = 0; }
                if (r != 3) break;
            }
        }
        if (at > (int64_t)8 * n) return ZS_E_FSE;
    }
    if (rem != 0) return ZS_E_FSE;
    for (uint32_t i = s; i < max_syms; ++i) norm[i] = 0;
    *log = al; *used = (uint32_t)((at + 7) >> 3);
    if (*used > n) return ZS_E_FSE;
    return ZS_OK;
}

// the decode table of 1 << log states from norm[0, syms); next[syms] is scratch.  false: the spread does not close
ZS_FN bool zs_fse_build(const int16_t *norm, uint32_t syms, uint32_t log, ZsFse *tab, uint16_t *next) {
    const uint32_t size = 1u << log, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
    uint32_t high = size;
    for (uint32_t s = 0; s < syms; ++s) if (norm[s] == -1) { if (high == 0) return false; tab[--high].sym = (uint8_t)s; next[s] = 1; }
    uint32_t pos = 0;
    for (uint32_t s = 0; s < syms; ++s) {
        if (norm[s] <= 0) continue;
        next[s] = (uint16_t)norm[s];
        for (int32_t i = 0; i < norm[s]; ++i) {
            if (pos >= high) return false;
            tab[pos].sym = (uint8_t)s;
            do pos = (pos + step) & mask; while (pos >= high);
        }
    }
    if (pos != 0) return false;
    for (uint32_t i = 0; i < size; ++i) {
        const uint32_t d = next[tab[i].sym]++;
        const uint32_t nb = log - zs_hibit(d);
        tab[i].nb = (uint8_t)nb;
        tab[i].base = (uint16_t)((d << nb) - size);
    }
    return true;
}

// the predefined distributions
ZS_FN int32_t zs_default_norm(uint32_t which, uint32_t s) {
    if (which == 0) return s >= 32 ? -1 : s == 0 ? 4 : s == 1 || s == 25 ? 3 : (s >= 13 && s <= 15) || s >= 27 ? 1 : 2;
    if (which == 1) return s >= 24 ? -1 : s >= 6 && s <= 8 ? 2 : 1;
    return s >= 46 ? -1 : s == 0 ? 1 : s == 1 ? 4 : s == 2 ? 3 : s <= 8 ? 2 : 1;
}
ZS_FN uint32_t zs_ll_base(uint32_t c) { return c < 16 ? c : c < 20 ? 16 + 2 * (c - 16) : c < 22 ? 24 + 4 * (c - 20) : c < 24 ? 32 + 8 * (c - 22) : c == 24 ? 48 : 1u << (c - 19); }
ZS_FN uint32_t zs_ll_bits(uint32_t c) { return c < 16 ? 0 : c < 20 ? 1 : c < 22 ? 2 : c < 24 ? 3 : c == 24 ? 4 : c - 19; }
ZS_FN uint32_t zs_ml_base(uint32_t c) {
    return c < 32 ? c + 3 : c < 36 ? 35 + 2 * (c - 32) : c < 38 ? 43 + 4 * (c - 36) : c < 40 ? 51 + 8 * (c - 38) : c < 42 ? 67 + 16 * (c - 40) : c == 42 ? 99 : (1u << (c - 36)) + 3;
}
ZS_FN uint32_t zs_ml_bits(uint32_t c) { return c < 32 ? 0 : c < 36 ? 1 : c < 38 ? 2 : c < 40 ? 3 : c < 42 ? 4 : c == 42 ? 5 : c - 36; }

// ---- what the head of a compressed block says (k_zs_heads: one lane per block) ----
struct ZsHead {
    uint32_t status;
    uint32_t lit_type, streams, regen;      // literals: 0 raw, 1 RLE, 2 Huffman, 3 treeless
    uint32_t lit_at, lit_len;               // the payload behind the literals header, from the block's first byte (the Huffman description included)
    uint32_t huf_len;                       // bytes of the Huffman description (type 2)
    uint32_t nseq, modes;                   // modes: LL << 4 | OF << 2 | ML, each 0 predefined, 1 RLE, 2 FSE, 3 repeat
    uint32_t tab_at[3];                     // where the description (or the RLE symbol) of LL, OF, ML stands
    uint32_t bits_at, bits_len;             // the sequence bitstream
};

// bytes of the Huffman description at p[0, n): 0 when it does not fit
ZS_FN uint32_t zs_huf_desc_len(const uint8_t *p, uint32_t n) {
    if (n == 0) return 0;
    const uint32_t len = p[0] < 128 ? 1u + p[0] : 1u + ((p[0] - 127u) + 1) / 2;
    return len <= n ? len : 0;
}

ZS_FN void zs_block_head(const uint8_t *p, uint32_t n, uint32_t bmax, ZsHead &h) {
    h = ZsHead{};
    if (n < 3) { h.status = ZS_E_BLOCK_SIZE; return; }
    const uint32_t type = p[0] & 3, sf = (p[0] >> 2) & 3;
    uint32_t hdr, regen, comp = 0, streams = 1;
    if (type < 2) {
        if (sf == 0 || sf == 2) { hdr = 1; regen = p[0] >> 3; }
        else if (sf == 1) { hdr = 2; regen = zs_le16(p) >> 4; }
        else { hdr = 3; regen = zs_le24(p) >> 4; }
        comp = type == 0 ? regen : 1;
    } else {
        if (sf < 2) { hdr = 3; const uint32_t v = zs_le24(p) >> 4; regen = v & 1023; comp = v >> 10; streams = sf == 0 ? 1 : 4; }
        else if (sf == 2) { if (n < 4) { h.status = ZS_E_LIT_HEADER; return; } hdr = 4; const uint32_t v = zs_le32(p) >> 4; regen = v & 16383; comp = v >> 14; streams = 4; }
        else { if (n < 5) { h.status = ZS_E_LIT_HEADER; return; } hdr = 5; const uint64_t v = (zs_le32(p) | (uint64_t)p[4] << 32) >> 4; regen = (uint32_t)(v & 262143); comp = (uint32_t)(v >> 18); streams = 4; }
        if (regen == 0 || comp == 0) { h.status = ZS_E_LIT_HEADER; return; }
    }
    if (regen > bmax) { h.status = ZS_E_BLOCK_SIZE; return; }
    if ((uint64_t)hdr + comp > n) { h.status = ZS_E_LIT_HEADER; return; }
    h.lit_type = type; h.streams = streams; h.regen = regen; h.lit_at = hdr; h.lit_len = comp;
    if (type == 2 && !(h.huf_len = zs_huf_desc_len(p + hdr, comp))) { h.status = ZS_E_LIT_HEADER; return; }
    uint32_t at = hdr + comp;
    if (at >= n) { h.status = ZS_E_SEQ_HEADER; return; }
    uint32_t nseq = p[at++];
    if (nseq == 0) { if (at != n) h.status = ZS_E_SEQ_HEADER; return; }
    if (nseq >= 128) {
        if (nseq == 255) { if (at + 2 > n) { h.status = ZS_E_SEQ_HEADER; return; } nseq = zs_le16(p + at) + 0x7F00; at += 2; }
        else { if (at + 1 > n) { h.status = ZS_E_SEQ_HEADER; return; } nseq = ((nseq - 128) << 8) + p[at++]; }
    }
    h.nseq = nseq;
    if (at >= n) { h.status = ZS_E_SEQ_HEADER; return; }
    const uint32_t mb = p[at++];
    if (mb & 3) { h.status = ZS_E_RESERVED; return; }
    h.modes = mb >> 2;
    for (uint32_t t = 0; t < 3; ++t) {
        const uint32_t mode = (h.modes >> (4 - 2 * t)) & 3;
        h.tab_at[t] = at;
        if (mode == 1) { if (at >= n) { h.status = ZS_E_SEQ_HEADER; return; } ++at; }
        else if (mode == 2) {
            int16_t norm[ZS_ML_SYMS];
            uint32_t log, used;
            const uint32_t st = zs_fse_read(p + at, n - at, t == 0 ? ZS_LL_LOG_MAX : t == 1 ? ZS_OF_LOG_MAX : ZS_ML_LOG_MAX, t == 0 ? ZS_LL_SYMS : t == 1 ? ZS_OF_SYMS : ZS_ML_SYMS,
                                           norm, &log, &used);
            if (st) { h.status = st; return; }
            at += used;
        }
    }
    if (at >= n) { h.status = ZS_E_SEQ_HEADER; return; }
    h.bits_at = at; h.bits_len = n - at;
}

// ---- a block as the rounds hand it to the kernels ----
struct ZsTabSrc { uint64_t at; uint32_t len, mode; };      // a table's defining bytes in the file: mode 0 predefined, 1 RLE, 2 FSE
struct ZsBlock {
    uint64_t src;                   // the block's content in the file
    uint32_t size, type;            // Block_Size (RLE: the regenerated size); 0 raw, 1 RLE, 2 compressed
    uint32_t bmax, window;          // of its frame
    uint64_t frame_pos;             // bytes of the frame's text in front of the block
    uint64_t out;                   // the block's first byte in the text
    uint64_t lit_off, seq_off;      // in the round's literals (bytes) and sequences (triples)
    uint64_t huf_at; uint32_t huf_len, pad0;
    ZsTabSrc tab[3];
    uint32_t rep[3];                // the repeat offsets in front of the block
    uint32_t out_size;
    ZsHead h;
};
struct ZsSeq { uint32_t ll, ml, ofv; };
// an element of the repeat-offset transfer function: src 0: the constant `val`; src 1..3: incoming r_src minus `val`
struct ZsRepEl { uint32_t src, val; };
struct ZsSeqRes { uint32_t status, out_size, lit_used, pad; ZsRepEl f[3]; };

ZS_FN void zs_rep_identity(ZsRepEl *f) { for (uint32_t i = 0; i < 3; ++i) { f[i].src = i + 1; f[i].val = 0; } }
// one sequence's step on the symbolic state; false: a constant offset of 0
ZS_FN bool zs_rep_step(ZsRepEl *f, uint32_t ofv, uint32_t ll) {
    if (ofv > 3) { f[2] = f[1]; f[1] = f[0]; f[0].src = 0; f[0].val = ofv - 3; return true; }
    const uint32_t idx = ofv - (ll != 0);          // 0: r1 stays in front; 1: r2; 2: r3; 3: r1 - 1
    if (idx == 0) return true;
    ZsRepEl x;
    if (idx == 3) {
        x = f[0];
        if (x.src == 0) { if (x.val <= 1) return false; --x.val; } else ++x.val;
    } else x = f[idx];
    if (idx != 1) f[2] = f[1];
    f[1] = f[0]; f[0] = x;
    return true;
}
// the same step on numbers; returns the offset the sequence uses (0: damage)
ZS_FN uint32_t zs_rep_resolve(uint32_t *r, uint32_t ofv, uint32_t ll) {
    if (ofv > 3) { r[2] = r[1]; r[1] = r[0]; r[0] = ofv - 3; return r[0]; }
    const uint32_t idx = ofv - (ll != 0);
    if (idx == 0) return r[0];
    const uint32_t x = idx == 3 ? r[0] - 1 : r[idx];
    if (x == 0) return 0;
    if (idx != 1) r[2] = r[1];
    r[1] = r[0]; r[0] = x;
    return x;
}
// a block's function on the state in front of it; false: an element of 0 or below
ZS_FN bool zs_rep_apply(const ZsRepEl *f, const uint32_t *in, uint32_t *out) {
    for (uint32_t i = 0; i < 3; ++i) {
        if (f[i].src == 0) out[i] = f[i].val;
        else { const uint32_t v = in[f[i].src - 1]; if (v <= f[i].val) return false; out[i] = v - f[i].val; }
        if (out[i] == 0) return false;
    }
    return true;
}

// ---- the tables of one block (LDS on the device) ----
struct ZsTabs {
    uint16_t huf[1u << ZS_HUF_LOG_MAX];    // sym | nb << 8
    ZsFse ll[1u << ZS_LL_LOG_MAX], of[1u << ZS_OF_LOG_MAX], ml[1u << ZS_ML_LOG_MAX];
    ZsFse wt[64];                           // the weights' own FSE table (accuracy log <= 6)
    uint8_t weight[256];
    uint32_t start[256];
    int16_t norm[3][ZS_ML_SYMS + 3];
    uint16_t next[3][ZS_ML_SYMS + 3];
    uint32_t log[3];
    uint32_t huf_log, status, n_sym;
    uint64_t acc[4];
};

// the Huffman description p[0, n) into t.weight / t.n_sym / t.huf_log (one lane)
ZS_FN uint32_t zs_huf_weights(ZsTabs &t, const uint8_t *p, uint32_t n) {
    if (n == 0) return ZS_E_WEIGHTS;
    uint32_t nw = 0;
    if (p[0] >= 128) {
        nw = p[0] - 127;
        if (1 + (nw + 1) / 2 > n) return ZS_E_WEIGHTS;
        for (uint32_t i = 0; i < nw; ++i) t.weight[i] = (i & 1) ? p[1 + i / 2] & 15 : p[1 + i / 2] >> 4;
    } else {
        const uint32_t len = p[0];
        if (len == 0 || 1 + len > n) return ZS_E_WEIGHTS;
        uint32_t log, used;
        // (weights above 11 are refused below, so a description that names a symbol above 11 is refused here)
        const uint32_t st = zs_fse_read(p + 1, len, 6, ZS_HUF_LOG_MAX + 1, t.norm[0], &log, &used);
        if (st) return st == ZS_E_ACCURACY ? (uint32_t)ZS_E_ACCURACY : (uint32_t)ZS_E_WEIGHTS;
        if (!zs_fse_build(t.norm[0], ZS_HUF_LOG_MAX + 1, log, t.wt, t.next[0])) return ZS_E_WEIGHTS;
        ZsBack b;
        if (!zs_back_init(b, p + 1 + used, len - used)) return ZS_E_BITSTREAM;
        uint32_t s1 = zs_back_get(b, log), s2 = zs_back_get(b, log);
        if (b.pos < 0) return ZS_E_BITSTREAM;
        for (;;) {
            if (nw + 2 > 255) return ZS_E_WEIGHTS;
            t.weight[nw++] = t.wt[s1].sym;
            s1 = t.wt[s1].base + zs_back_get(b, t.wt[s1].nb);
            if (b.pos < 0) { t.weight[nw++] = t.wt[s2].sym; break; }
            t.weight[nw++] = t.wt[s2].sym;
            s2 = t.wt[s2].base + zs_back_get(b, t.wt[s2].nb);
            if (b.pos < 0) { t.weight[nw++] = t.wt[s1].sym; break; }
        }
    }
    uint32_t total = 0, ones = 0;
    for (uint32_t i = 0; i < nw; ++i) {
        const uint32_t w = t.weight[i];
        if (w > ZS_HUF_LOG_MAX) return ZS_E_WEIGHTS;
        if (w) total += 1u << (w - 1);
        ones += w == 1;
    }
    if (total == 0) return ZS_E_WEIGHTS;
    const uint32_t log = zs_hibit(total) + 1;
    if (log > ZS_HUF_LOG_MAX) return ZS_E_WEIGHTS;
    const uint32_t rest = (1u << log) - total;
    if (rest & (rest - 1)) return ZS_E_WEIGHTS;
    const uint32_t last = zs_hibit(rest) + 1;
    t.weight[nw++] = (uint8_t)last;
    ones += last == 1;
    if (ones < 2 || (ones & 1)) return ZS_E_WEIGHTS;
    // where every symbol's entries start: by weight, then by symbol
    uint32_t at = 0;
    for (uint32_t w = 1; w <= log; ++w)
        for (uint32_t s = 0; s < nw; ++s) if (t.weight[s] == w) { t.start[s] = at; at += 1u << (w - 1); }
    t.n_sym = nw; t.huf_log = log;
    return ZS_OK;
}

// E: ZsTabs *t; lane0(), lane1(), slot(i), sync()
// the literals of block B into lit[0, regen).  Returns the status on every lane
template <class E> ZS_FN uint32_t zs_literals(E &e, const uint8_t *in, uint64_t n_in, const ZsBlock &B, uint8_t *lit) {
    ZsTabs &t = *e.t;
    const ZsHead &h = B.h;
    const uint8_t *p = in + B.src + h.lit_at;
    if (h.lit_type == 0) { for (uint32_t l = e.lane0(); l < e.lane1(); ++l) for (uint32_t i = l; i < h.regen; i += ZS_NL) lit[i] = p[i]; return ZS_OK; }
    if (h.lit_type == 1) { const uint8_t v = p[0]; for (uint32_t l = e.lane0(); l < e.lane1(); ++l) for (uint32_t i = l; i < h.regen; i += ZS_NL) lit[i] = v; return ZS_OK; }
    if (B.huf_len == 0 || B.huf_at + B.huf_len > n_in) return ZS_E_NO_TABLE;
    e.sync();
    if (e.lane0() == 0) t.status = zs_huf_weights(t, in + B.huf_at, B.huf_len);
    e.sync();
    if (t.status) return t.status;
    const uint32_t log = t.huf_log;
    for (uint32_t l = e.lane0(); l < e.lane1(); ++l)
        for (uint32_t s = l; s < t.n_sym; s += ZS_NL) {
            const uint32_t w = t.weight[s];
            if (!w) continue;
            const uint16_t v = (uint16_t)(s | (log + 1 - w) << 8);
            for (uint32_t i = 0, k = 1u << (w - 1); i < k; ++i) t.huf[t.start[s] + i] = v;
        }
    e.sync();
    const uint8_t *q = p + (h.lit_type == 2 ? h.huf_len : 0);
    const uint32_t len = h.lit_len - (h.lit_type == 2 ? h.huf_len : 0);
    uint32_t size[4] = {len, 0, 0, 0}, from[4] = {0, 0, 0, 0}, count[4] = {h.regen, 0, 0, 0};
    if (h.streams == 4) {
        if (len < 10) return ZS_E_BITSTREAM;
        const uint32_t seg = (h.regen + 3) / 4;
        if (3 * seg > h.regen) return ZS_E_BITSTREAM;
        size[0] = zs_le16(q); size[1] = zs_le16(q + 2); size[2] = zs_le16(q + 4);
        if (6 + size[0] + size[1] + size[2] > len) return ZS_E_BITSTREAM;
        size[3] = len - 6 - size[0] - size[1] - size[2];
        from[0] = 6; from[1] = from[0] + size[0]; from[2] = from[1] + size[1]; from[3] = from[2] + size[2];
        count[0] = count[1] = count[2] = seg; count[3] = h.regen - 3 * seg;
    }
    if (e.lane0() == 0) t.status = ZS_OK;
    e.sync();
    for (uint32_t l = e.lane0(); l < e.lane1() && l < h.streams; ++l) {
        ZsBack b;
        uint32_t st = ZS_OK;
        if (!zs_back_init(b, q + from[l], size[l])) st = ZS_E_BITSTREAM;
        else {
            uint8_t *o = lit + (h.streams == 4 ? l * count[0] : 0);
            for (uint32_t i = 0; i < count[l]; ++i) {
                const uint32_t v = t.huf[zs_back_peek(b, log)];
                o[i] = (uint8_t)v;
                b.pos -= v >> 8;
                if (b.pos < 0) break;
            }
            if (b.pos != 0) st = ZS_E_BITSTREAM;
        }
        if (st) t.status = st;
    }
    e.sync();
    return t.status;
}

// table `which` (0 LL, 1 OF, 2 ML) from its source; one lane
ZS_FN uint32_t zs_seq_table(ZsTabs &t, uint32_t which, const uint8_t *in, uint64_t n_in, const ZsTabSrc &s) {
    ZsFse *tab = which == 0 ? t.ll : which == 1 ? t.of : t.ml;
    const uint32_t syms = which == 0 ? ZS_LL_SYMS : which == 1 ? ZS_OF_SYMS : ZS_ML_SYMS;
    const uint32_t max_log = which == 0 ? ZS_LL_LOG_MAX : which == 1 ? ZS_OF_LOG_MAX : ZS_ML_LOG_MAX;
    if (s.mode == 1) {
        if (s.at >= n_in) return ZS_E_INPUT;
        if (in[s.at] >= syms) return ZS_E_SYMBOL;
        tab[0].sym = in[s.at]; tab[0].nb = 0; tab[0].base = 0;
        t.log[which] = 0;
        return ZS_OK;
    }
    uint32_t log = which == 1 ? 5 : 6, used = 0;
    if (s.mode == 0) for (uint32_t i = 0; i < syms; ++i) t.norm[which][i] = (int16_t)(i < (which == 0 ? 36u : which == 1 ? 29u : 53u) ? zs_default_norm(which, i) : 0);
    else {
        if (s.mode != 2 || s.at + s.len > n_in) return ZS_E_NO_TABLE;
        const uint32_t st = zs_fse_read(in + s.at, s.len, max_log, syms, t.norm[which], &log, &used);
        if (st) return st;
    }
    if (!zs_fse_build(t.norm[which], syms, log, tab, t.next[which])) return ZS_E_FSE;
    t.log[which] = log;
    return ZS_OK;
}

// the sequences of block B into seq[0, nseq), with the block's output size and its repeat-offset function
template <class E> ZS_FN void zs_sequences(E &e, const uint8_t *in, uint64_t n_in, const ZsBlock &B, ZsSeq *seq, ZsSeqRes &r) {
    ZsTabs &t = *e.t;
    const ZsHead &h = B.h;
    r = ZsSeqRes{};
    zs_rep_identity(r.f);
    r.out_size = h.regen;
    if (h.nseq == 0) return;
    e.sync();
    if (e.lane0() == 0) t.status = ZS_OK;
    e.sync();
    for (uint32_t l = e.lane0(); l < e.lane1() && l < 3; ++l) { const uint32_t st = zs_seq_table(t, l, in, n_in, B.tab[l]); if (st) t.status = st; }
    e.sync();
    if (t.status) { r.status = t.status; return; }
    if (e.lane0() != 0) return;
    ZsBack b;
    if (!zs_back_init(b, in + B.src + h.bits_at, h.bits_len)) { r.status = ZS_E_BITSTREAM; return; }
    uint32_t sl = zs_back_get(b, t.log[0]), so = zs_back_get(b, t.log[1]), sm = zs_back_get(b, t.log[2]);
    if (b.pos < 0) { r.status = ZS_E_BITSTREAM; return; }
    uint64_t out = 0, lits = 0;
    for (uint32_t i = 0; i < h.nseq; ++i) {
        const uint32_t cl = t.ll[sl].sym, co = t.of[so].sym, cm = t.ml[sm].sym;
        if (cl >= ZS_LL_SYMS || co >= ZS_OF_SYMS || cm >= ZS_ML_SYMS) { r.status = ZS_E_SYMBOL; return; }
        const uint32_t ofv = (1u << co) + zs_back_get(b, co);
        const uint32_t ml = zs_ml_base(cm) + zs_back_get(b, zs_ml_bits(cm));
        const uint32_t ll = zs_ll_base(cl) + zs_back_get(b, zs_ll_bits(cl));
        if (i + 1 < h.nseq) {
            sl = t.ll[sl].base + zs_back_get(b, t.ll[sl].nb);
            sm = t.ml[sm].base + zs_back_get(b, t.ml[sm].nb);
            so = t.of[so].base + zs_back_get(b, t.of[so].nb);
        }
        if (b.pos < 0) { r.status = ZS_E_BITSTREAM; return; }
        seq[i].ll = ll; seq[i].ml = ml; seq[i].ofv = ofv;
        lits += ll; out += ml;
        if (lits > h.regen) { r.status = ZS_E_LITERALS; return; }
        if (lits + out > B.bmax) { r.status = ZS_E_BLOCK_SIZE; return; }
        if (!zs_rep_step(r.f, ofv, ll)) { r.status = ZS_E_OFFSET; return; }
    }
    if (b.pos != 0) { r.status = ZS_E_BITSTREAM; return; }
    r.lit_used = (uint32_t)lits;
    r.out_size = (uint32_t)(h.regen + out);
}

// ---- execution ----
// block B's bytes into text[B.out, B.out + B.out_size) and their origins into org[0, B.out_size): 0 for a final byte, else the
// distance back from the block's first byte to the byte it equals.  Returns the status on every lane
template <class E> ZS_FN uint32_t zs_execute(E &e, const uint8_t *in, const ZsBlock &B, const uint8_t *lit, const ZsSeq *seq, uint8_t *text, uint32_t *org) {
    uint8_t *o = text + B.out;
    if (B.type == 0) { for (uint32_t l = e.lane0(); l < e.lane1(); ++l) for (uint32_t i = l; i < B.size; i += ZS_NL) { o[i] = in[B.src + i]; org[i] = 0; } return ZS_OK; }
    if (B.type == 1) { const uint8_t v = in[B.src]; for (uint32_t l = e.lane0(); l < e.lane1(); ++l) for (uint32_t i = l; i < B.size; i += ZS_NL) { o[i] = v; org[i] = 0; } return ZS_OK; }
    uint32_t r[3] = {B.rep[0], B.rep[1], B.rep[2]};
    uint32_t op = 0, lp = 0;
    for (uint32_t s = 0; s < B.h.nseq; ++s) {
        const ZsSeq q = seq[s];
        if ((uint64_t)lp + q.ll > B.h.regen || (uint64_t)op + q.ll + q.ml > B.out_size) return ZS_E_BLOCK_SIZE;
        for (uint32_t l = e.lane0(); l < e.lane1(); ++l) for (uint32_t i = l; i < q.ll; i += ZS_NL) { o[op + i] = lit[lp + i]; org[op + i] = 0; }
        op += q.ll; lp += q.ll;
        const uint32_t off = zs_rep_resolve(r, q.ofv, q.ll);
        if (off == 0 || off > B.frame_pos + op || off > B.window) return ZS_E_OFFSET;
        const int64_t from = (int64_t)op - off;        // the match's first source byte, from the block's first byte
        for (uint32_t k0 = 0; k0 < q.ml; k0 += ZS_NL) {
            e.sync();                                   // the bytes of the steps before are written
            for (uint32_t l = e.lane0(); l < e.lane1(); ++l) {
                const uint32_t j = k0 + l;
                if (j >= q.ml) continue;
                const int64_t sp = from + (off >= ZS_NL ? j : j % off);
                e.tb[e.slot(l)] = sp < 0 ? (uint8_t)0 : o[sp];
                e.to[e.slot(l)] = sp < 0 ? (uint32_t)-sp : org[sp];
            }
            e.sync();
            for (uint32_t l = e.lane0(); l < e.lane1(); ++l) {
                const uint32_t j = k0 + l;
                if (j >= q.ml) continue;
                o[op + j] = e.tb[e.slot(l)]; org[op + j] = e.to[e.slot(l)];
            }
        }
        op += q.ml;
    }
    const uint32_t rest = B.h.regen - lp;
    if ((uint64_t)op + rest != B.out_size) return ZS_E_BLOCK_SIZE;
    for (uint32_t l = e.lane0(); l < e.lane1(); ++l) for (uint32_t i = l; i < rest; i += ZS_NL) { o[op + i] = lit[lp + i]; org[op + i] = 0; }
    return ZS_OK;
}

// the deferred bytes of one block, lanes [l0, l1) of nl: the blocks in front of it are final
ZS_FN void zs_resolve_block(uint8_t *text, const uint32_t *org, uint64_t out, uint32_t size, uint32_t l0, uint32_t l1, uint32_t nl) {
    for (uint32_t l = l0; l < l1; ++l)
        for (uint32_t i = l; i < size; i += nl) { const uint32_t d = org[i]; if (d) text[out + i] = text[out - d]; }
}

// ---- XXH64, seed 0 ----
#define ZS_P1 0x9E3779B185EBCA87ull
#define ZS_P2 0xC2B2AE3D27D4EB4Full
#define ZS_P3 0x165667B19E3779F9ull
#define ZS_P4 0x85EBCA77C2B2AE63ull
#define ZS_P5 0x27D4EB2F165667C5ull
ZS_FN uint64_t zs_rotl(uint64_t x, uint32_t r) { return x << r | x >> (64 - r); }
ZS_FN uint64_t zs_xxh_round(uint64_t acc, uint64_t w) { return zs_rotl(acc + w * ZS_P2, 31) * ZS_P1; }
ZS_FN uint64_t zs_xxh_merge(uint64_t h, uint64_t v) { return (h ^ zs_xxh_round(0, v)) * ZS_P1 + ZS_P4; }
// the end of a hash: h already holds the merged accumulators (or ZS_P5) plus the length; p[i, n) are the bytes behind the last stripe
ZS_FN uint64_t zs_xxh_finish(uint64_t h, const uint8_t *p, uint64_t i, uint64_t n) {
    for (; i + 8 <= n; i += 8) h = zs_rotl(h ^ zs_xxh_round(0, zs_le64(p + i)), 27) * ZS_P1 + ZS_P4;
    if (i + 4 <= n) { h = zs_rotl(h ^ (uint64_t)zs_le32(p + i) * ZS_P1, 23) * ZS_P2 + ZS_P3; i += 4; }
    for (; i < n; ++i) h = zs_rotl(h ^ p[i] * ZS_P5, 11) * ZS_P1;
    h ^= h >> 33; h *= ZS_P2; h ^= h >> 29; h *= ZS_P3; h ^= h >> 32;
    return h;
}
// lanes 0..3 hold the four accumulators over the 32-byte stripes; every lane returns the hash
template <class E> ZS_FN uint64_t zs_xxh64(E &e, const uint8_t *p, uint64_t n) {
    ZsTabs &t = *e.t;
    const uint64_t stripes = n / 32;
    e.sync();
    for (uint32_t l = e.lane0(); l < e.lane1() && l < 4; ++l) {
        uint64_t a = l == 0 ? ZS_P1 + ZS_P2 : l == 1 ? ZS_P2 : l == 2 ? 0 : 0 - ZS_P1;
        uint64_t s = 0;
        for (; s + 8 <= stripes; s += 8) {              // eight loads in flight, then the chain
            uint64_t w[8];
            for (uint32_t i = 0; i < 8; ++i) __builtin_memcpy(&w[i], p + 32 * (s + i) + 8 * l, 8);
            for (uint32_t i = 0; i < 8; ++i) a = zs_xxh_round(a, w[i]);
        }
        for (; s < stripes; ++s) a = zs_xxh_round(a, zs_le64(p + 32 * s + 8 * l));
        t.acc[l] = a;
    }
    e.sync();
    uint64_t h;
    if (stripes) {
        h = zs_rotl(t.acc[0], 1) + zs_rotl(t.acc[1], 7) + zs_rotl(t.acc[2], 12) + zs_rotl(t.acc[3], 18);
        for (uint32_t i = 0; i < 4; ++i) h = zs_xxh_merge(h, t.acc[i]);
    } else h = ZS_P5;
    return zs_xxh_finish(h + n, p, 32 * stripes, n);
}

// XXH64 of a frame whose text arrives in parts (a frame that spans rounds of the sliding driver, zs_round.h): the four
// accumulators and the count of bytes they have taken.  `hashed` stays a multiple of 32 until the frame ends: a part takes whole
// stripes only, and the next part starts again at the frame byte `hashed`
struct ZsXxh { uint64_t acc[4]; uint64_t hashed; };
// one part: p[0, n) are the frame's bytes from `hashed` on (0 when `first`: S is not read).  Not `last`: the whole stripes of
// the part go into S, and 0 is returned.  `last`: p[0, n) is all that is left of the frame, and every lane returns the hash of
// its hashed + n bytes -- as zs_xxh64 does, the form below 32 bytes that uses no accumulator included.  Lanes 0..3 as there
template <class E> ZS_FN uint64_t zs_xxh64_part(E &e, ZsXxh &S, const uint8_t *p, uint64_t n, bool first, bool last) {
    ZsTabs &t = *e.t;
    const uint64_t h0 = first ? 0 : S.hashed, stripes = n / 32;
    e.sync();
    for (uint32_t l = e.lane0(); l < e.lane1() && l < 4; ++l) {
        uint64_t a = first ? (l == 0 ? ZS_P1 + ZS_P2 : l == 1 ? ZS_P2 : l == 2 ? 0 : 0 - ZS_P1) : S.acc[l];
        uint64_t s = 0;
        for (; s + 8 <= stripes; s += 8) {
            uint64_t w[8];
            for (uint32_t i = 0; i < 8; ++i) __builtin_memcpy(&w[i], p + 32 * (s + i) + 8 * l, 8);
            for (uint32_t i = 0; i < 8; ++i) a = zs_xxh_round(a, w[i]);
        }
        for (; s < stripes; ++s) a = zs_xxh_round(a, zs_le64(p + 32 * s + 8 * l));
        t.acc[l] = a;
    }
    e.sync();                                           // (every lane has read S.hashed; the accumulators are in t)
    if (!last) {
        for (uint32_t l = e.lane0(); l < e.lane1() && l < 4; ++l) S.acc[l] = t.acc[l];
        if (e.lane0() == 0) S.hashed = h0 + 32 * stripes;
        return 0;
    }
    const uint64_t total = h0 + n;
    uint64_t h;
    if (total >= 32) {
        h = zs_rotl(t.acc[0], 1) + zs_rotl(t.acc[1], 7) + zs_rotl(t.acc[2], 12) + zs_rotl(t.acc[3], 18);
        for (uint32_t i = 0; i < 4; ++i) h = zs_xxh_merge(h, t.acc[i]);
    } else h = ZS_P5;
    return zs_xxh_finish(h + total, p, 32 * stripes, n);
}
