// bz_twin.h -- the sequential backend of bz_round.h's bz_run for the host twins (bz_twin.cpp, fastx_twin.cpp; g++): the finder, the block
// decode, the scatter, the walk and the run-length layer of bz_core.h the way the kernels of k_bzip2.h run them, the marks a census with a
// seek map records on the way (BzMarkRec), and the seeded decode of one block at its marks (bz_segment_lane lane by lane, DESIGN
// section 29).  TEST INFRASTRUCTURE, not part of the product library.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "bz_core.h"
#include "bz_round.h"

struct BzTwinEnv {
    static constexpr uint32_t PER = 256;
    BzTabs tabs;
    BzTabs *t = &tabs;
    uint32_t lane = 0, nl = 1;
    void sync() {}
};

// every bit offset of d[0, n) that carries a magic, ascending
static inline void bz_twin_find_all(const uint8_t *d, uint64_t n, std::vector<uint64_t> &cand) {
    for (uint64_t q = 0; q + 6 <= n; ++q) {
        const uint64_t w = bz_be64(d, n, q);
        for (uint32_t s = 0; s < 8; ++s) {
            const uint32_t kind = bz_magic_in(w, s);
            if (kind && 8 * q + s + 48 <= 8 * n) cand.push_back((8 * q + s) | (kind == 2 ? BZ_END_FLAG : 0));
        }
    }
}

struct BzTwin {
    const uint8_t *p = nullptr;
    uint64_t n = 0;
    uint32_t bs = 0;
    std::vector<uint8_t> L, out;
    std::vector<uint32_t> cnt, tt;
    BzTwinEnv env;
    uint32_t crc_tab[256];
    bool keep_marks = false;                         // a recorder will ask for marks (marks_out): finish records every link's
    std::vector<BzMark> marks;
    BzTwin() { bz_crc_table(crc_tab, 0, 1); }
    bool load(const uint8_t *d, uint64_t len) { p = d; n = len; return true; }
    bool find(std::vector<uint64_t> &cand) { bz_twin_find_all(p, n, cand); return true; }
    uint32_t default_round(uint32_t) { return BZ_ROUND_MAX; }
    bool decode(const uint64_t *pos, uint32_t k, uint32_t bs_, BzRes *res) {
        bs = bs_;
        L.resize((size_t)k * bs); cnt.resize((size_t)k * 256);
        for (uint32_t c = 0; c < k; ++c) {
            bz_decode_block(env, p, n, pos[c], bs, L.data() + (size_t)c * bs, res[c]);
            memcpy(&cnt[(size_t)c * 256], env.tabs.cnt, sizeof env.tabs.cnt);
        }
        return true;
    }
    bool finish(BzLink *l, uint32_t m, uint32_t *crc, uint64_t *out_bytes, const uint8_t **bytes) {
        uint64_t total = 0;
        if (keep_marks) marks.assign((size_t)m * BZ_MARKS, BzMark{0, 0, 0, 0});
        for (uint32_t a = 0; a < m; ++a) {
            uint8_t *Lc = L.data() + (size_t)l[a].slot * bs;
            tt.resize(l[a].n);
            bz_scatter(Lc, l[a].n, &cnt[(size_t)l[a].slot * 256], tt.data());
            if (!(keep_marks ? bz_walk(tt.data(), l[a].n, l[a].orig, Lc, BzMarkRec(&marks[(size_t)a * BZ_MARKS], l[a].n)) : bz_walk(tt.data(), l[a].n, l[a].orig, Lc))) return false;
            const uint64_t len = bz_rle_len(Lc, l[a].n);
            l[a].out_off = total; l[a].run_open = (len & BZ_RUN_OPEN) != 0;
            total += len & ~BZ_RUN_OPEN;
        }
        out.resize(total + 4);
        for (uint32_t a = 0; a < m; ++a) {
            const uint8_t *pre = L.data() + (size_t)l[a].slot * bs;
            uint8_t *o = out.data() + l[a].out_off;
            crc[a] = keep_marks ? bz_rle_write(pre, l[a].n, crc_tab, o, BzMarkRec(&marks[(size_t)a * BZ_MARKS], l[a].n)) : bz_rle_write(pre, l[a].n, crc_tab, o);
        }
        *out_bytes = total; *bytes = out.data();
        return true;
    }
    bool marks_out(BzMark *dst, uint32_t m) { memcpy(dst, marks.data(), (size_t)m * BZ_MARKS * sizeof(BzMark)); return true; }
};

// One block entered at its marks, as the device does it: the entropy decode from bit `pos` of d[0, n) (which need not be the census's
// file: a damaged copy), accepted only if n, origPtr, the stored CRC and the length in bits are the map's (bits: end_bit - bit); the
// scatter; the BZ_MARKS lanes of bz_segment_lane into out[0, len) (out + skew is where the text starts; tt is never walked as a whole).
// only_lane < BZ_MARKS: that lane alone.  0, a decode status, or BZ_E_ENTRY
static inline uint32_t bz_twin_seeded(const uint8_t *d, uint64_t n, uint32_t bs, uint64_t pos, uint64_t bits, uint32_t bn, uint32_t orig, uint32_t crc, uint32_t len,
                                      const BzMark *m, uint8_t *out, uint32_t only_lane = BZ_MARKS) {
    static uint32_t crc_tab[256];
    static const bool made = (bz_crc_table(crc_tab, 0, 1), true);
    (void)made;
    BzTwinEnv env;
    std::vector<uint8_t> L(bs);
    BzRes r;
    bz_decode_block(env, d, n, pos, bs, L.data(), r);
    if (r.status != BZ_OK) return r.status;
    if (r.n != bn || r.orig != orig || r.crc != crc || r.end_bit - pos != bits) return BZ_E_ENTRY;
    std::vector<uint32_t> tt(bn);
    bz_scatter(L.data(), bn, env.tabs.cnt, tt.data());
    bool good = true;
    for (uint32_t j = 0; j < BZ_MARKS; ++j)
        if (only_lane >= BZ_MARKS || only_lane == j) good = bz_segment_lane(tt.data(), bn, orig, crc, len, m, j, crc_tab, out) && good;
    return good ? (uint32_t)BZ_OK : (uint32_t)BZ_E_ENTRY;
}
