// gzip_core.h -- speculative decoding of plain and multi-member gzip (RFC 1952 members of RFC 1951 deflate): the marker
// decode driver, the block-start predicates of the finder and the CRC shift by table.  Compiled by hipcc (k_gzip.h) and g++
// (gzip_twin.cpp) alike, on top of inflate_core.h: the bit reader, the tables and the deflate block body (inf_block) are the
// ones of the BGZF path (inf_raw / k_inflate).
//
// A chunk is decoded from a bit offset whose 32 KiB window is not known.  The driver emits 16-bit symbols: 0-255 a byte,
// GZ_MARK | i byte i of the unknown window (a back-reference that reaches before the chunk's first symbol; markers are copied
// like bytes).  Windows are propagated and markers resolved later (k_gz_window / k_gz_resolve, or the twin).
//
// Boundaries: the start of every deflate block and of every member header.  A non-final stored block whose padding bits are
// zero decodes the same from every bit offset between its true start and 8 B - 3 (B: the byte of LEN), so it is counted at
// 8 B - 3 (gz_canon), which is where the finder reports it.  The driver stops at the first boundary at or past `stop`.
#pragma once
#include "inflate_core.h"

#ifdef __HIPCC__
#define INF_FN_M __host__ __device__ inline      // a member of an environment both compilers see
#else
#define INF_FN_M inline
#endif

enum {
    GZ_E_HEADER = 10,       // not a gzip member header (magic, method, reserved flags, FHCRC), or trailing bytes
    GZ_E_CRC = 11,          // a member's CRC32 or ISIZE differs from its trailer (checked by the host)
    GZ_E_OVERFLOW = 12,     // more symbols than the chunk's slot
    GZ_E_SEGS = 13,         // more member segments than the chunk's record space
    GZ_E_MARKER = 14,       // a window reference before the member's first byte
};

#define GZ_WIN 32768u
#define GZ_MARK 0x8000u
#define GZ_NONE 0xFFFFFFFFu
#define GZ_SEG_HEAD 1u      // the segment starts with a member header inside the chunk
#define GZ_SEG_TRAIL 2u     // the segment ends with its member's trailer inside the chunk (crc / isize valid)

// one member segment of a chunk: symbols [o0, o1) of the chunk's output
struct GzSeg { uint32_t o0, o1, crc, isize, flags; };
// the result of one chunk decode: status, the boundary it stopped at (or the end of input), symbols and segments written,
// eof = it ended exactly after the last member's trailer at the end of the input
struct GzRes { uint32_t status, end_bit, n_sym, n_seg, eof, pad; };

INF_FN uint32_t gz_u16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
INF_FN uint32_t gz_u32(const uint8_t *p) { return gz_u16(p) | gz_u16(p + 2) << 16; }

// ---- predicates (per lane on the device: no INF_UNI inside) ----
INF_FN bool gz_is_header(const uint8_t *p, uint32_t n, uint32_t q) {
    return q + 10 <= n && p[q] == 0x1f && p[q + 1] == 0x8b && p[q + 2] == 8 && (p[q + 3] & 0xE0) == 0;
}
// bit offset `bit` is a canonical non-final stored block start: bit % 8 == 5, three zero header bits, LEN == ~NLEN
INF_FN bool gz_stored_at(const uint8_t *p, uint32_t n, uint32_t bit) {
    const uint32_t q = bit >> 3;
    if ((bit & 7) != 5 || q + 5 > n || (p[q] & 0xE0)) return false;
    return (gz_u16(p + q + 1) ^ 0xFFFFu) == gz_u16(p + q + 3);
}
// the boundary at `bit` as counted by the stop rule (see the top of the file)
INF_FN uint32_t gz_canon(const uint8_t *p, uint32_t n, uint32_t bit) {
    const uint32_t B = (bit + 10) >> 3;                       // LEN's byte: the first byte boundary after the 3 header bits
    if (B + 4 > n) return bit;
    for (uint32_t q = bit; q < 8 * B; ++q)
        if ((p[q >> 3] >> (q & 7)) & 1) return bit;
    if ((gz_u16(p + B) ^ 0xFFFFu) != gz_u16(p + B + 2)) return bit;
    return 8 * B - 3;
}

// k bits (k <= 24) at bit offset *bit, zero past the end; *bit advances
INF_FN uint32_t gz_bits(const uint8_t *p, uint32_t n, uint32_t *bit, uint32_t k) {
    const uint32_t q = *bit >> 3;
    uint32_t w = 0;
    for (uint32_t i = 0; i < 4; ++i) if (q + i < n) w |= (uint32_t)p[q + i] << (8 * i);
    const uint32_t v = (w >> (*bit & 7)) & ((1u << k) - 1);
    *bit += k;
    return v;
}
// code lengths counted per length: the rule of inf_code_prepare (complete; or incomplete only with maxl <= 1 unless strict)
INF_FN bool gz_kraft(const uint16_t *cnt, bool strict) {
    int left = 1;
    uint32_t maxl = 0;
    for (uint32_t l = 1; l < 16; ++l) { left = left * 2 - (int)cnt[l]; if (left < 0) return false; if (cnt[l]) maxl = l; }
    return !(left > 0 && maxl != 0 && (strict || maxl != 1));
}
// A non-final dynamic-Huffman block header at `bit` that inf_dynamic would accept: HLIT <= 29, HDIST <= 29, a complete
// precode, code lengths that decode without overrun, an end-of-block code, valid literal/length and distance codes.
// Memory from the caller (LDS per lane on the device): tab[128] the precode's lookup table, cnt[32] counts per length.
INF_FN bool gz_is_dynamic(const uint8_t *p, uint32_t n, uint32_t bit, uint8_t *tab, uint16_t *cnt) {
    uint32_t b = bit;
    if (gz_bits(p, n, &b, 3) != 4) return false;                 // BFINAL 0, BTYPE 2
    const uint32_t hlit = gz_bits(p, n, &b, 5), hdist = gz_bits(p, n, &b, 5), ncode = gz_bits(p, n, &b, 4) + 4;
    if (hlit > 29 || hdist > 29) return false;
    uint64_t pl = 0;                                           // 19 precode lengths, 3 bits each, by symbol
    for (uint32_t i = 0; i < ncode; ++i) pl |= (uint64_t)gz_bits(p, n, &b, 3) << (3 * inf_clen_order(i));
    uint32_t left = 0;
    for (uint32_t s = 0; s < 19; ++s) { const uint32_t L = (uint32_t)(pl >> (3 * s)) & 7; if (L) left += 128u >> L; }
    if (left != 128) return false;                             // the precode must be complete
    uint32_t code = 0;
    for (uint32_t L = 1; L < 8; ++L) {                          // canonical codes, reversed into a 7-bit table
        for (uint32_t s = 0; s < 19; ++s) {
            if (((uint32_t)(pl >> (3 * s)) & 7) != L) continue;
            const uint32_t rev = inf_rev(code++, L);
            for (uint32_t j = rev; j < 128; j += 1u << L) tab[j] = (uint8_t)(s << 3 | L);
        }
        code <<= 1;
    }
    for (uint32_t l = 0; l < 32; ++l) cnt[l] = 0;
    const uint32_t nlen = hlit + 257, total = nlen + hdist + 1;
    uint32_t i = 0, prev = 0;
    bool eob = false;
    while (i < total) {
        const uint32_t e = tab[gz_bits(p, n, &b, 7) & 127];
        b -= 7 - (e & 7);
        const uint32_t s = e >> 3;
        uint32_t rep = 1, v = s;
        if (s == 16) { if (i == 0) return false; v = prev; rep = 3 + gz_bits(p, n, &b, 2); }
        else if (s == 17) { v = 0; rep = 3 + gz_bits(p, n, &b, 3); }
        else if (s == 18) { v = 0; rep = 11 + gz_bits(p, n, &b, 7); }
        if (i + rep > total) return false;
        for (uint32_t r = 0; r < rep; ++r, ++i) {
            cnt[(i < nlen ? 0 : 16) + v]++;
            if (i == 256 && v) eob = true;
        }
        prev = v;
        if (b > 8 * n) return false;
    }
    if (b > 8 * n || !eob) return false;
    return gz_kraft(cnt, false) && gz_kraft(cnt + 16, false);
}
// the finder's predicate: a member header, a canonical non-final stored block, or a non-final dynamic block
INF_FN bool gz_is_candidate(const uint8_t *p, uint32_t n, uint32_t bit, uint8_t *tab, uint16_t *cnt) {
    if ((bit & 7) == 0 && gz_is_header(p, n, bit >> 3)) return true;
    if (gz_stored_at(p, n, bit)) return true;
    return gz_is_dynamic(p, n, bit, tab, cnt);
}
// the cheap first test: the 13 header bits of a non-final dynamic block with HLIT, HDIST <= 29, or a byte that can start a
// member header or hold a canonical stored header
INF_FN bool gz_maybe_candidate(const uint8_t *p, uint32_t n, uint32_t bit) {
    uint32_t b = bit;
    const uint32_t h = gz_bits(p, n, &b, 13);
    if ((h & 7) == 4 && ((h >> 3) & 31) <= 29 && ((h >> 8) & 31) <= 29) return true;
    const uint32_t q = bit >> 3;
    return q < n && (((bit & 7) == 0 && p[q] == 0x1f) || ((bit & 7) == 5 && !(p[q] & 0xE0)));
}

// ---- the marker decode driver ----
// header length of the member at byte q, or -(status)
INF_FN int gz_header_len(const uint8_t *p, uint32_t n, uint32_t q) {
    if (q + 10 > n) return -(int)INF_E_INPUT;
    if (!INF_UNI(gz_is_header(p, n, q))) return -(int)GZ_E_HEADER;
    const uint32_t flg = INF_UNI(p[q + 3]);
    uint32_t h = q + 10;
    if (flg & 4) {
        if (h + 2 > n) return -(int)INF_E_INPUT;
        h += 2 + INF_UNI(gz_u16(p + h));
    }
    for (uint32_t f = 8; f <= 16; f <<= 1) {                  // FNAME, FCOMMENT: zero-terminated
        if (!(flg & f)) continue;
        while (h < n && INF_UNI(p[h])) ++h;
        if (h >= n) return -(int)INF_E_INPUT;
        ++h;
    }
    if (flg & 2) {                                             // FHCRC: low 16 bits of the header's CRC-32 (zlib checks it)
        if (h + 2 > n) return -(int)INF_E_INPUT;
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t i = q; i < h; ++i) c = inf_crc_entry((c ^ INF_UNI(p[i])) & 0xFF) ^ (c >> 8);
        if (INF_UNI(gz_u16(p + h)) != (~c & 0xFFFFu)) return -(int)GZ_E_HEADER;
        h += 2;
    }
    if (h > n) return -(int)INF_E_INPUT;
    return (int)(h - q);
}

// Decode p[0, n) from bit `start` until the first boundary at or past `stop` (or the end of the input when `eof`: p[n] is
// the input's end).  E (see inflate_core.h) with output of u16 symbols: E::lit(b), E::copy(dist, len) (a source index
// before 0 is marker GZ_MARK | (GZ_WIN + index)), E::stored(src, n), E::pos, E::cap (E::full: GZ_E_OVERFLOW);
// E::seg(i, s) stores a segment record.  E::own / E::mstart (the member started in this chunk, at this symbol) are set here
// and read by E::reach(): own ? pos - mstart : pos + GZ_WIN.
template <class E> INF_FN void gz_decode(E &e, const uint8_t *p, uint32_t n, bool eof, uint32_t start, uint32_t stop,
                                         uint32_t max_seg, GzRes &r) {
    r.status = INF_OK; r.end_bit = start; r.n_sym = 0; r.n_seg = 0; r.eof = 0; r.pad = 0;
    int rc = INF_OK;
    uint32_t nseg = 0;
    GzSeg cur = {0, 0, 0, 0, 0};
    bool in_member = !((start & 7) == 0 && INF_UNI(gz_is_header(p, n, start >> 3)));
    bool open = in_member;
    e.own = false; e.mstart = 0;
    InfBits b;
    inf_bits_init(b, p, 0, n);
    if (start > 8 * n) rc = INF_E_INPUT; else inf_seek(b, start);
    const uint32_t guard = 8 * n / 3 + 2;                        // every block takes >= 3 bits, every member >= 18 bytes
    bool ended = false;
    for (uint32_t it = 0; !rc && it < guard; ++it) {
        if (inf_overrun(b)) { rc = INF_E_INPUT; break; }
        const uint32_t at = inf_bitpos(b);
        const uint32_t cb = in_member ? INF_UNI(gz_canon(p, n, at)) : at;
        if (!in_member && (at >> 3) == n && eof) { r.eof = 1; r.end_bit = at; ended = true; break; }
        if (cb >= stop) { r.end_bit = cb; ended = true; break; }
        if (!in_member) {
            const int hl = gz_header_len(p, n, at >> 3);
            if (hl < 0) { rc = -hl; break; }
            cur = GzSeg{e.pos, 0, 0, 0, GZ_SEG_HEAD};
            open = true; e.own = true; e.mstart = e.pos; in_member = true;
            inf_seek(b, at + 8u * (uint32_t)hl);
            continue;                                            // the first block's start is a boundary too
        }
        bool last = false;
        rc = inf_block(e, b, &last);
        if (rc) break;
        if (last) {                                              // the trailer, then the next member's header
            if (inf_overrun(b)) { rc = INF_E_INPUT; break; }
            const uint32_t q = (inf_bitpos(b) + 7) >> 3;
            if (q + 8 > n) { rc = INF_E_INPUT; break; }
            cur.o1 = e.pos; cur.crc = INF_UNI(gz_u32(p + q)); cur.isize = INF_UNI(gz_u32(p + q + 4)); cur.flags |= GZ_SEG_TRAIL;
            if (nseg >= max_seg) { rc = GZ_E_SEGS; break; }
            e.seg(nseg++, cur);
            open = false; e.own = false; in_member = false;
            inf_seek(b, 8 * (q + 8));
        }
    }
    if (!rc && !ended) rc = INF_E_INPUT;
    if (!rc && open) {
        cur.o1 = e.pos;
        if (nseg >= max_seg) rc = GZ_E_SEGS; else e.seg(nseg++, cur);
    }
    if (rc) r.end_bit = inf_overrun(b) ? 8 * n : inf_bitpos(b);   // where it failed: the walk tells damage from a short buffer
    r.status = (uint32_t)rc; r.n_sym = e.pos; r.n_seg = nseg;
}

// ---- CRC-32 shifts by table, and the running register ----
// pw[i] = x^(8 * 2^i) mod P, for shifts by table (gz_crc_shift_tab)
INF_FN void gz_crc_powers(uint32_t *pw, uint32_t k) { uint32_t x = 1u << 23; for (uint32_t i = 0; i < k; ++i) { pw[i] = x; x = inf_gf2_mul(x, x); } }
INF_FN uint32_t gz_crc_shift_tab(const uint32_t *pw, uint32_t crc, uint32_t n) {
    for (uint32_t i = 0; n; ++i, n >>= 1) if (n & 1) crc = inf_gf2_mul(pw[i], crc);
    return crc;
}
// CRC-32 register update over n bytes (no init / final xor): crc = ~standard crc while running
INF_FN uint32_t gz_crc_run(const uint32_t *t, uint32_t c, uint8_t byte) { return t[(c ^ byte) & 0xFF] ^ (c >> 8); }

// ---- the seeded decode of one entry of a seek map (fx_seek.h FX_SEEK_GZIP) ----
// An entry is a true boundary whose member state and 32 KiB window are known, so gz_decode from it is an ordinary inflate whose
// history is preloaded: bytes, no markers.  The history is a byte ring of GZ_RING bytes (kernel: LDS) that holds the window in front of
// the entry's first byte; the text leaves it by halves: whenever a half is complete it is folded into the entry's CRC-32 (64 lane
// stripes, shifted and XOR-combined) and written to the entry's place in the staging block in aligned 4-byte words.  The ring is
// indexed by the output address (text position + `skew`, the staging offset's low two bits), so a half's words are aligned in the ring
// and in memory alike; only the entry's first and last word are written as bytes -- the neighbouring entries own their other bytes.
#define GZ_RING 65536u
#define GZ_HALF (GZ_RING / 2)
#define GZ_E_ENTRY 15u       // a seeded decode that ended elsewhere, or with another length or CRC-32, than the map says

// one seeded decode: file bytes comp[c_off, c_off + n) from bit `start` (0..7) to bit `stop` (GZ_NONE with eof: the end of the file, which
// is comp[c_off + n]); the text, `len` bytes of CRC-32 `crc`, to stage[out_off, out_off + len); window `win` of the uploaded windows
// (GZ_NONE: none -- entry 0), of which `valid` bytes belong to the member the entry starts inside (in_member)
struct GzEntryTask { uint64_t c_off, out_off; uint32_t n, start, stop, len, crc, valid, win, eof; };

// T: the tables (InfDevTabs / TwinTabs).  M: the memory side --
//   M::ld(p), M::st(p, v)      a ring byte this wavefront stored moments before (kernel: ld_wave / st_wave)
//   M::word(p, w)              an aligned 4-byte store to the staging block
//   M::wave_xor(c)             the XOR over the wavefront's lanes (twin: its one lane has walked all 64 stripes)
template <class T, class M> struct GzSeedEnv : T {
    static constexpr int full = GZ_E_OVERFLOW;
    uint8_t *ring;
    const uint32_t *crc_tab, *pw;   // the CRC-32 table and gz_crc_powers(32)
    uint8_t *dst;                   // where text byte 0 goes
    uint32_t skew;                  // the low two bits of that address
    uint32_t pos, cap, valid, done; // done: text bytes that have left the ring
    uint32_t crc;                   // ... and their CRC-32
    bool own;
    uint32_t mstart;
    template <class... A> INF_FN_M GzSeedEnv(uint8_t *ring_, const uint32_t *crc_tab_, const uint32_t *pw_, uint8_t *dst_, uint32_t skew_, uint32_t cap_, uint32_t valid_, A &&...a)
        : T(a...), ring(ring_), crc_tab(crc_tab_), pw(pw_), dst(dst_), skew(skew_), pos(0), cap(cap_), valid(valid_), done(0), crc(0), own(false), mstart(0) {}
    INF_FN_M uint8_t *at(uint32_t i) const { return ring + ((i + skew) & (GZ_RING - 1)); }      // text byte i (or, below 0, window byte GZ_WIN + i)
    // the entry's window in front of text byte 0
    INF_FN_M void preload(const uint8_t *win) { for (uint32_t j = this->lane; j < GZ_WIN; j += this->nl) M::st(at(j - GZ_WIN), win[j]); }
    // a member that started in the entry: back to its first byte; else the bytes of the window that belong to the member
    INF_FN_M uint32_t reach() const { return own ? pos - mstart : pos >= GZ_WIN ? GZ_WIN : pos + valid; }
    // text [done, z) leaves the ring (z - done <= GZ_HALF): its CRC by 64 stripes, its bytes in words
    INF_FN_M void leave(uint32_t z) {
        const uint32_t a = done, n = z - a;
        if (!n) return;
        const uint32_t s = (n + 63) / 64;
        uint32_t c = 0;
        for (uint32_t l = this->lane; l < 64; l += this->nl) {
            const uint32_t x = l * s < n ? l * s : n, y = x + s < n ? x + s : n;
            uint32_t r = 0xFFFFFFFFu;
            for (uint32_t i = x; i < y; ++i) r = gz_crc_run(crc_tab, r, M::ld(at(a + i)));
            if (y > x) c ^= gz_crc_shift_tab(pw, ~r, n - y);
        }
        crc = gz_crc_shift_tab(pw, crc, n) ^ M::wave_xor(c);
        uint32_t head = (4u - ((a + skew) & 3u)) & 3u;            // bytes up to the first aligned address
        if (head > n) head = n;
        for (uint32_t j = this->lane; j < head; j += this->nl) dst[a + j] = M::ld(at(a + j));
        const uint32_t nw = (n - head) >> 2;
        for (uint32_t w = this->lane; w < nw; w += this->nl) {
            const uint32_t i = a + head + 4 * w;
            M::word(dst + i, (uint32_t)M::ld(at(i)) | (uint32_t)M::ld(at(i + 1)) << 8 | (uint32_t)M::ld(at(i + 2)) << 16 | (uint32_t)M::ld(at(i + 3)) << 24);
        }
        for (uint32_t j = head + 4 * nw + this->lane; j < n; j += this->nl) dst[a + j] = M::ld(at(a + j));
        done = z;
    }
    // behind every advance of pos by at most a half: the half that is complete leaves
    INF_FN_M void drain() { if ((pos + skew) / GZ_HALF != (done + skew) / GZ_HALF) leave(((pos + skew) & ~(GZ_HALF - 1)) - skew); }
    INF_FN_M void finish() { leave(pos); }
    INF_FN_M void lit(uint8_t b) { if (this->lane == 0) M::st(at(pos), b); ++pos; drain(); }
    INF_FN_M void copy(uint32_t dist, uint32_t len) {
        for (uint32_t c = 0; c < len; c += 64) {                  // len <= 258; j >= dist repeats the first dist bytes (see k_inflate.h)
            for (uint32_t j = c + this->lane; j < len && j < c + 64; j += this->nl) M::st(at(pos + j), M::ld(at(pos - dist + (j < dist ? j : j % dist))));
        }
        pos += len; drain();
    }
    INF_FN_M void stored(const uint8_t *src, uint32_t n) {        // up to 65535 bytes: by pieces that end at a half
        while (n) {
            const uint32_t room = GZ_HALF - ((pos + skew) & (GZ_HALF - 1)), k = n < room ? n : room;
            for (uint32_t j = this->lane; j < k; j += this->nl) M::st(at(pos + j), src[j]);
            pos += k; src += k; n -= k; drain();
        }
    }
    INF_FN_M void seg(uint32_t, const GzSeg &) {}                // (the census checked every member; the entry's CRC covers the bytes)
};

// the entry's decode with its checks: the status word (INF_OK: stage holds the entry's text)
template <class E> INF_FN uint32_t gz_entry_run(E &e, const uint8_t *p, const GzEntryTask &t) {
    GzRes r;
    gz_decode(e, p, t.n, t.eof != 0, t.start, t.stop, GZ_NONE, r);
    if (r.status) return r.status;
    e.finish();
    const bool ended = t.stop == GZ_NONE ? r.eof != 0 : (r.end_bit == t.stop && !r.eof);
    return ended && r.n_sym == t.len && e.crc == t.crc ? (uint32_t)INF_OK : GZ_E_ENTRY;
}
