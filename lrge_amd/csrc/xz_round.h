// xz_round.h -- host side of the block-parallel xz decode: the walk over stream footers, indexes, block headers and LZMA2 chunk
// headers (every container check happens here, before any launch), rounds of consecutive blocks, the launches of a round and the
// block checks.  One template drives both the device (host_xz.inl: kernels of k_xz.h) and the host twin (xz_twin.cpp: the same
// steps as loops over xz_core.h), so the CPU suite tests this logic as the library runs it.
//
// An .xz block starts with a dictionary reset, and the index states every block's sizes: the place of every block's text is
// known before a byte is decoded, no block needs another's text, and a finished round's text may leave the device block at once.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "xz_core.h"

struct XzStats { uint64_t streams, blocks, chunks, raw_chunks, checks_checked, rounds, launches, bytes_out, walk_us; };
struct XzBlock {
    uint64_t at;                    // the block header in the file
    uint64_t check_at;              // its check field
    uint64_t usize;
    uint32_t chunk0, n_chunks;      // its chunks in the table
    uint32_t check;                 // 0 none, 1 CRC32, 4 CRC64
};
struct XzSpan { uint64_t at, len; uint32_t wide, pad; };    // a text span to check: CRC32, or (wide) CRC64

enum { XZ_RUN_OK = 0, XZ_RUN_DEVICE = -2 };
#define XZ_ROUND_MAX 4096u
#define XZ_LAUNCH_DEFAULT ((uint64_t)XZ_CHUNK_USIZE_MAX)
// blocks below which the device loses to liblzma on one thread (BASELINE section 13: 8 blocks 7.0x slower, 64 blocks 1.1x faster)
#define XZ_MIN_BLOCKS_DEFAULT 64u

struct XzCrcTab { uint32_t t[256]; XzCrcTab() { for (uint32_t i = 0; i < 256; ++i) t[i] = xz_crc32_entry(i); } };
static inline uint32_t xz_host_crc32(const uint8_t *d, uint64_t n) {
    static const XzCrcTab tab;
    uint32_t c = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; ++i) c = tab.t[(c ^ d[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}
// a variable-length integer at d[*p, lim): false for an encoding the format forbids
static inline bool xz_vli(const uint8_t *d, uint64_t *p, uint64_t lim, uint64_t *v) {
    *v = 0;
    for (uint32_t i = 0; i < 9; ++i) {
        if (*p >= lim) return false;
        const uint8_t b = d[(*p)++];
        *v |= (uint64_t)(b & 0x7F) << (7 * i);
        if (!(b & 0x80)) return !(b == 0 && i > 0);
    }
    return false;
}
static inline bool xz_zeros(const uint8_t *d, uint64_t a, uint64_t z) { for (; a < z; ++a) if (d[a]) return false; return true; }

// the chunks of one block's payload d[src, src + csize): a hop per chunk header.  XZ_OK or a status with *bad the offset it belongs to
static inline int xz_walk_chunks(const uint8_t *d, uint64_t src, uint64_t csize, uint32_t dict_size, XzBlock &b, std::vector<XzChunk> &chunks, XzStats &st, uint64_t *bad) {
    const uint64_t end = src + csize;
    uint64_t p = src, out = 0, dict_at = 0;
    bool need_dict = true, need_props = true;
    uint8_t lc = 0, lp = 0, pb = 0;
    b.chunk0 = (uint32_t)chunks.size();
    for (;;) {
        *bad = p;
        if (p >= end) return XZ_E_SIZES;                       // no end byte inside the block's bytes
        const uint32_t ctl = d[p];
        if (ctl == 0) {
            if (p + 1 != end || out != b.usize) return XZ_E_SIZES;
            break;
        }
        XzChunk c{};
        c.at = p; c.out = out; c.dict_size = dict_size;
        if (ctl >= 0xE0 || ctl == 1) { need_props = true; need_dict = false; c.flags |= XZ_C_DICT_RESET; dict_at = out; }
        else if (need_dict) return XZ_E_CONTROL;
        if (ctl >= 0x80) {
            if (p + 5 > end) return XZ_E_SIZES;
            c.usize = (((ctl & 0x1F) << 16) | (uint32_t)d[p + 1] << 8 | d[p + 2]) + 1;
            c.csize = ((uint32_t)d[p + 3] << 8 | d[p + 4]) + 1;
            p += 5;
            if (ctl >= 0xC0) {
                if (p >= end) return XZ_E_SIZES;
                uint32_t v = d[p++];
                if (v > 224) return XZ_E_PROPS;
                pb = (uint8_t)(v / 45); v -= pb * 45; lp = (uint8_t)(v / 9); lc = (uint8_t)(v - lp * 9);
                if (lc + lp > 4) return XZ_E_PROPS;
                need_props = false;
                c.flags |= XZ_C_STATE_RESET;
            } else if (need_props) return XZ_E_CONTROL;
            else if (ctl >= 0xA0) c.flags |= XZ_C_STATE_RESET;
        } else {
            if (ctl > 2) return XZ_E_CONTROL;
            if (p + 3 > end) return XZ_E_SIZES;
            c.usize = c.csize = ((uint32_t)d[p + 1] << 8 | d[p + 2]) + 1;
            c.flags |= XZ_C_RAW;
            p += 3;
            ++st.raw_chunks;
        }
        c.src = p; c.dict_at = dict_at; c.lc = lc; c.lp = lp; c.pb = pb;
        if (p + c.csize > end || out + c.usize > b.usize) return XZ_E_SIZES;
        if (chunks.size() >= 0xFFFFFFFEull) return XZ_E_TOO_BIG;
        chunks.push_back(c);
        p += c.csize; out += c.usize;
    }
    b.n_chunks = (uint32_t)chunks.size() - b.chunk0;
    return XZ_OK;
}

// the streams, blocks and chunks of d[0, n): footers and indexes from the file's end backwards, then every block header and chunk
// header in file order.  XZ_OK or a status with *bad the byte offset it belongs to
static inline int xz_walk(const uint8_t *d, uint64_t n, std::vector<XzBlock> &blocks, std::vector<XzChunk> &chunks, XzStats &st, uint64_t *bad) {
    struct Stream { uint64_t at, index_at, index_end; uint32_t check; };
    std::vector<Stream> streams;
    static const uint8_t magic[6] = {0xFD, '7', 'z', 'X', 'Z', 0x00};
    *bad = 0;
    if (n < 32) return n >= 6 && memcmp(d, magic, 6) != 0 ? (int)XZ_E_MAGIC : (int)XZ_E_INPUT;
    if (memcmp(d, magic, 6) != 0) return XZ_E_MAGIC;
    uint64_t e = n;                                            // the streams behind d[0, e) are known
    while (e > 0) {
        uint64_t pad = 0;
        while (e - pad >= 4 && xz_le32(d + e - pad - 4) == 0) pad += 4;
        e -= pad;
        if (e == 0) { *bad = 0; return XZ_E_MAGIC; }           // (padding alone, in front of the first stream)
        *bad = e >= 12 ? e - 12 : 0;
        if (e < 32) return XZ_E_FOOTER;
        const uint8_t *f = d + e - 12;
        if (f[10] != 'Y' || f[11] != 'Z') return d[e - 1] == 0 ? (int)XZ_E_PADDING : (int)XZ_E_FOOTER;   // (a run of zeros that is no multiple of four ends here too)
        if (xz_le32(f) != xz_host_crc32(f + 4, 6)) return XZ_E_HEADER_CRC;
        if (f[8] != 0 || (f[9] & 0xF0)) return XZ_E_RESERVED;
        Stream s{};
        s.check = f[9];
        if (s.check != 0 && s.check != 1 && s.check != 4) return XZ_E_CHECK_ID;
        const uint64_t isize = ((uint64_t)xz_le32(f + 4) + 1) * 4;
        if (isize + 24 > e) return XZ_E_INDEX;
        s.index_end = e - 12; s.index_at = s.index_end - isize;
        // the index: its records say where the stream starts
        *bad = s.index_at;
        if (d[s.index_at] != 0) return XZ_E_INDEX;
        if (xz_le32(d + s.index_end - 4) != xz_host_crc32(d + s.index_at, isize - 4)) return XZ_E_HEADER_CRC;
        uint64_t p = s.index_at + 1, lim = s.index_end - 4, count, body = 0;
        if (!xz_vli(d, &p, lim, &count)) return XZ_E_INDEX;
        if (count > (lim - p) / 2) return XZ_E_INDEX;         // (a record has two bytes or more)
        for (uint64_t i = 0; i < count; ++i) {
            uint64_t unpadded, usize;
            if (!xz_vli(d, &p, lim, &unpadded) || !xz_vli(d, &p, lim, &usize)) return XZ_E_INDEX;
            if (unpadded < 5 || unpadded > s.index_at || usize > ((uint64_t)1 << 62)) return XZ_E_INDEX;
            body += (unpadded + 3) & ~(uint64_t)3;
            if (body > s.index_at) return XZ_E_INDEX;
        }
        if (lim - p > 3 || !xz_zeros(d, p, lim)) return XZ_E_INDEX;
        if (body + 12 > s.index_at) return XZ_E_INDEX;
        s.at = s.index_at - body - 12;
        *bad = s.at;
        if (memcmp(d + s.at, magic, 6) != 0) return XZ_E_MAGIC;
        if (xz_le32(d + s.at + 8) != xz_host_crc32(d + s.at + 6, 2)) return XZ_E_HEADER_CRC;
        if (d[s.at + 6] != f[8] || d[s.at + 7] != f[9]) return XZ_E_FLAGS;
        streams.push_back(s);
        e = s.at;
    }
    std::reverse(streams.begin(), streams.end());
    st.streams = streams.size();
    for (const Stream &s : streams) {
        const uint32_t check_size = s.check == 0 ? 0 : s.check == 1 ? 4 : 8;
        uint64_t ip = s.index_at + 1, count, at = s.at + 12;
        (void)xz_vli(d, &ip, s.index_end, &count);
        for (uint64_t i = 0; i < count; ++i) {
            uint64_t unpadded, usize;
            (void)xz_vli(d, &ip, s.index_end, &unpadded); (void)xz_vli(d, &ip, s.index_end, &usize);
            *bad = at;
            XzBlock b{};
            b.at = at; b.usize = usize; b.check = s.check;
            const uint64_t hsize = ((uint64_t)d[at] + 1) * 4;
            if (d[at] == 0) return XZ_E_INDEX;                  // (an index indicator where a block header must stand)
            if (hsize + check_size >= unpadded) return XZ_E_SIZES;
            if (xz_le32(d + at + hsize - 4) != xz_host_crc32(d + at, hsize - 4)) return XZ_E_HEADER_CRC;
            const uint32_t flags = d[at + 1];
            if (flags & 0x3C) return XZ_E_RESERVED;
            if (flags & 3) return XZ_E_FILTER;
            const uint64_t csize = unpadded - hsize - check_size, hlim = at + hsize - 4;
            uint64_t p = at + 2, v;
            if (flags & 0x40) { if (!xz_vli(d, &p, hlim, &v) || v != csize) return XZ_E_SIZES; }
            if (flags & 0x80) { if (!xz_vli(d, &p, hlim, &v) || v != usize) return XZ_E_SIZES; }
            uint64_t id, psize;
            if (!xz_vli(d, &p, hlim, &id) || id != 0x21 || !xz_vli(d, &p, hlim, &psize) || psize != 1 || p >= hlim) return XZ_E_FILTER;
            const uint32_t db = d[p++];
            if (db > 40) return XZ_E_DICT_SIZE;
            const uint32_t dict_size = db == 40 ? 0xFFFFFFFFu : (2u | (db & 1)) << (db / 2 + 11);
            if (!xz_zeros(d, p, hlim)) return XZ_E_PADDING;
            const uint64_t padded = (unpadded + 3) & ~(uint64_t)3;       // header, payload, padding, check
            b.check_at = at + padded - check_size;
            if (!xz_zeros(d, at + hsize + csize, b.check_at)) { *bad = at + hsize + csize; return XZ_E_PADDING; }
            const int rc = xz_walk_chunks(d, at + hsize, csize, dict_size, b, chunks, st, bad);
            if (rc) return rc;
            if (blocks.size() >= 0xFFFFFFFEull) return XZ_E_TOO_BIG;
            blocks.push_back(b);
            at += padded;
        }
    }
    st.chunks = chunks.size();
    return XZ_OK;
}

// D (the decode backend):
//   bool load(const uint8_t *d, uint64_t n, const XzChunk *c, uint64_t n_chunks)   the compressed input and the chunk table
//   uint32_t default_round(uint64_t block_bytes)                  blocks per round when the caller names none (block_bytes: the largest block's text)
//   bool reserve(uint64_t bytes, uint32_t k)                      room for a round's text behind the text so far, k cleared state slots;
//                                                                 false with over() when the budget does not hold the text
//   bool decode(const XzTask *t, uint32_t m, uint32_t *status, uint32_t *bad_chunk)
//                                                                 one launch: task i decodes its chunks into the round's text
//   bool check(const XzSpan *s, uint32_t m, uint64_t *crc)        of the round's text [s.at, s.at + s.len), the m spans at once
//   const uint8_t *commit(uint64_t bytes)                         the round's text is final: it joins the text so far; the bytes for the sink (nullptr: failure)
// sink(bytes, n) -> bool (false: stop with XZ_RUN_DEVICE)
// Returns XZ_RUN_OK, XZ_RUN_DEVICE or an XZ_E_* status (*bad_off: the byte offset it belongs to).
struct XzCfg { uint64_t round_blocks, launch_bytes, min_blocks; bool check; };
template <class D, class Sink>
static int xz_run(D &dev, const uint8_t *d, uint64_t n, const XzCfg &cfg, Sink &&sink, XzStats &st, uint64_t *bad_off) {
    memset(&st, 0, sizeof st);
    uint64_t bad_dummy = 0;
    uint64_t &bad = bad_off ? *bad_off : bad_dummy;
    bad = 0;
    std::vector<XzBlock> blocks;
    std::vector<XzChunk> chunks;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = xz_walk(d, n, blocks, chunks, st, &bad);
    st.walk_us = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    if (rc) return rc;
    const uint64_t nb = blocks.size();
    if (nb < cfg.min_blocks) { bad = 0; return XZ_E_FEW_BLOCKS; }
    if (!nb) return XZ_RUN_OK;
    if (!dev.load(d, n, chunks.data(), chunks.size())) return XZ_RUN_DEVICE;
    uint64_t largest = 0;
    for (const XzBlock &b : blocks) largest = std::max(largest, b.usize);
    const uint32_t K = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(cfg.round_blocks ? cfg.round_blocks : dev.default_round(largest), 1), XZ_ROUND_MAX);
    const uint64_t per_launch = std::max<uint64_t>(cfg.launch_bytes ? cfg.launch_bytes : XZ_LAUNCH_DEFAULT, 1);
    std::vector<uint64_t> off;                      // where the round's blocks start in its text
    std::vector<uint32_t> next;                     // their next chunk
    std::vector<XzTask> tasks;
    std::vector<uint32_t> status, bad_chunk;
    std::vector<XzSpan> spans;
    std::vector<uint64_t> crc;
    for (uint64_t i = 0; i < nb;) {
        const uint32_t k = (uint32_t)std::min<uint64_t>(K, nb - i);
        const XzBlock *B = &blocks[i];
        ++st.rounds;
        off.assign(k, 0); next.assign(k, 0);
        uint64_t round_bytes = 0;
        for (uint32_t j = 0; j < k; ++j) { off[j] = round_bytes; round_bytes += B[j].usize; next[j] = B[j].chunk0; }
        if (!dev.reserve(round_bytes, k)) return dev.over() ? (int)XZ_E_TOO_BIG : (int)XZ_RUN_DEVICE;
        // launches: every unfinished block takes whole chunks of at most per_launch bytes, one chunk at least
        int fail = XZ_OK;
        uint32_t fail_j = k;
        for (;;) {
            tasks.clear();
            for (uint32_t j = 0; j < (fail ? fail_j : k); ++j) {       // (behind a failed block nothing decides the status any more)
                const uint32_t end = B[j].chunk0 + B[j].n_chunks;
                if (next[j] >= end) continue;
                uint32_t c1 = next[j];
                uint64_t bytes = 0;
                while (c1 < end && (c1 == next[j] || bytes + chunks[c1].usize <= per_launch)) bytes += chunks[c1++].usize;
                tasks.push_back(XzTask{off[j], next[j], c1, j, 0});
                next[j] = c1;
            }
            if (tasks.empty()) break;
            ++st.launches;
            status.assign(tasks.size(), 0); bad_chunk.assign(tasks.size(), 0);
            if (!dev.decode(tasks.data(), (uint32_t)tasks.size(), status.data(), bad_chunk.data())) return XZ_RUN_DEVICE;
            for (size_t a = 0; a < tasks.size(); ++a)
                if (status[a] && tasks[a].slot < fail_j) {
                    fail = (int)status[a]; fail_j = tasks[a].slot;
                    bad = chunks[std::min<uint64_t>(bad_chunk[a], chunks.size() - 1)].at;
                }
        }
        // the first failing block in file order decides: a check in front of it still may
        spans.clear();
        if (cfg.check) for (uint32_t j = 0; j < (fail ? fail_j : k); ++j) if (B[j].check) spans.push_back(XzSpan{off[j], B[j].usize, B[j].check == 4, j});
        if (!spans.empty()) {
            crc.assign(spans.size(), 0);
            if (!dev.check(spans.data(), (uint32_t)spans.size(), crc.data())) return XZ_RUN_DEVICE;
            for (size_t a = 0; a < spans.size(); ++a) {
                const XzBlock &b = B[spans[a].pad];
                ++st.checks_checked;
                if (crc[a] != (spans[a].wide ? xz_le64(d + b.check_at) : (uint64_t)xz_le32(d + b.check_at))) { bad = b.check_at; return XZ_E_CHECK; }
            }
        }
        if (fail) return fail;
        st.blocks += k;
        const uint8_t *bytes = dev.commit(round_bytes);
        if (!bytes) return XZ_RUN_DEVICE;
        if (round_bytes && !sink(bytes, round_bytes)) return XZ_RUN_DEVICE;
        st.bytes_out += round_bytes;
        i += k;
    }
    return XZ_RUN_OK;
}
