// gz_twin.h -- the sequential backend of gzip_round.h's gz_run for the host twins (gzip_twin.cpp, fastx_twin.cpp; g++): the finder, the
// marker decodes (gzip_core.h), the window propagation, the resolve and the lane-stripe segment CRCs the way the kernels of k_gzip.h
// do them, and the seeded decode of one entry of a seek map (GzSeedEnv) with the twin's memory side.
// TEST INFRASTRUCTURE, not part of the product library.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "gzip_core.h"
#include "gzip_round.h"
#include "twin_env.h"

#define GZ_TWIN_STRIPE 1024u      // bytes per lane stripe of k_gz_resolve

struct GzTwinEnv : TwinTabs {
    static constexpr int full = GZ_E_OVERFLOW;
    uint16_t *out = nullptr;
    GzSeg *sp = nullptr;
    uint32_t pos = 0, cap = 0;
    bool own = false;                                         // the current member started in this chunk, at symbol mstart
    uint32_t mstart = 0;
    uint32_t reach() const { return own ? pos - mstart : pos + GZ_WIN; }
    void lit(uint8_t b) { out[pos++] = b; }
    void copy(uint32_t dist, uint32_t len) {
        for (uint32_t j = 0; j < len; ++j, ++pos) {
            const int64_t src = (int64_t)pos - dist;
            out[pos] = src >= 0 ? out[src] : (uint16_t)(GZ_MARK | (uint32_t)(GZ_WIN + src));
        }
    }
    void stored(const uint8_t *src, uint32_t n) { for (uint32_t i = 0; i < n; ++i) out[pos++] = src[i]; }
    void seg(uint32_t i, const GzSeg &s) { sp[i] = s; }
};

struct GzTwin {
    const uint8_t *p = nullptr;
    uint32_t n = 0;
    std::vector<uint16_t> sym;
    std::vector<GzSeg> seg;
    std::vector<std::vector<uint16_t>> sym_big;      // retry buffers of the round
    std::vector<std::vector<GzSeg>> seg_big;
    std::vector<uint8_t> carry = std::vector<uint8_t>(GZ_WIN, 0), out;
    uint8_t tab[128]; uint16_t cnt[32];

    bool keep_wins = false;                          // a recorder will ask for windows (windows_out): finish keeps every link's
    std::vector<uint8_t> wins;

    std::vector<GzRes> pending;
    bool load(const uint8_t *d, uint64_t off, uint32_t len) { p = d + off; n = len; return true; }
    void prefetch(const uint8_t *, uint64_t, uint32_t) {}
    bool launch(const GzTask *t, uint32_t nt, bool eof) { pending.resize(nt); return decode(t, nt, eof, pending.data()); }
    bool wait(GzRes *res) { std::copy(pending.begin(), pending.end(), res); return true; }
    bool bytes_ready() { return true; }
    bool find(uint32_t chunk, uint32_t nc, uint32_t lim, uint32_t *cand) {
        for (uint32_t c = 1; c < nc; ++c) {
            const uint32_t b0 = 8 * c * chunk, b1 = 8 * std::min<uint64_t>((uint64_t)(c + 1) * chunk, lim);
            for (uint32_t b = b0; b < b1; ++b)
                if (gz_maybe_candidate(p, n, b) && gz_is_candidate(p, n, b, tab, cnt)) { cand[c] = b; break; }
        }
        return true;
    }
    bool decode(const GzTask *t, uint32_t nt, bool eof, GzRes *res) {
        for (uint32_t i = 0; i < nt; ++i) {
            GzTwinEnv e;
            if (t[i].big) {                                   // (every task of the call in one extra buffer)
                if (sym_big.size() < t[i].big) { sym_big.resize(t[i].big); seg_big.resize(t[i].big); }
                std::vector<uint16_t> &bs = sym_big[t[i].big - 1];
                std::vector<GzSeg> &bg = seg_big[t[i].big - 1];
                if (bs.size() < t[i].sym_off + t[i].cap) bs.resize(t[i].sym_off + t[i].cap);
                if (bg.size() < (uint64_t)t[i].seg_off + t[i].seg_cap) bg.resize((uint64_t)t[i].seg_off + t[i].seg_cap);
                e.out = bs.data() + t[i].sym_off; e.sp = bg.data() + t[i].seg_off;
            } else {
                const uint64_t need = t[i].sym_off + t[i].cap, needs = (uint64_t)t[i].seg_off + t[i].seg_cap;
                if (sym.size() < need) sym.resize(need);
                if (seg.size() < needs) seg.resize(needs);
                e.out = sym.data() + t[i].sym_off; e.sp = seg.data() + t[i].seg_off;
            }
            e.cap = t[i].cap;
            gz_decode(e, p, n, eof, t[i].start, t[i].stop, t[i].seg_cap, res[i]);
        }
        return true;
    }
    bool segs(const GzTask &t, uint32_t k, GzSeg *o) {
        const GzSeg *s = (t.big ? seg_big[t.big - 1].data() : seg.data()) + t.seg_off;
        memcpy(o, s, k * sizeof(GzSeg));
        return true;
    }
    bool finish(const GzLink *l, uint32_t nl, const GzSeg *s, uint32_t, uint64_t out_bytes, uint32_t *seg_crc, uint32_t *marker_err,
                const uint8_t **bytes) {
        static const CrcTab tab;
        out.assign(out_bytes, 0);
        std::vector<uint8_t> w = carry, nw(GZ_WIN);
        wins.clear();
        for (uint32_t k = 0; k < nl; ++k) {
            const GzLink &L = l[k];
            if (keep_wins) wins.insert(wins.end(), w.begin(), w.end());          // (the window chain: what k_gz_window writes to `windows`)
            const uint16_t *sy = (L.big ? sym_big[L.big - 1].data() : sym.data()) + L.sym_off;
            uint8_t *o = out.data() + L.out_off;
            for (uint32_t i = 0; i < L.n_sym; ++i) {                               // resolve (k_gz_resolve)
                const uint32_t v = sy[i];
                if (v >= GZ_MARK && (v & (GZ_WIN - 1)) < GZ_WIN - L.valid && !*marker_err) *marker_err = k + 1;
                o[i] = v < 256 ? (uint8_t)v : w[v & (GZ_WIN - 1)];
            }
            for (uint32_t j = 0; j < GZ_WIN; ++j) {                                // the next window (k_gz_window)
                const uint64_t idx = (uint64_t)L.n_sym + j;                        // in (window ++ chunk)
                nw[j] = idx < GZ_WIN ? w[idx] : o[idx - GZ_WIN];
            }
            w.swap(nw);
            for (uint32_t g = 0; g < L.nseg; ++g) {                                 // segment CRCs over lane stripes
                const GzSeg &G = s[L.seg0 + g];
                uint32_t c = 0;
                for (uint32_t a = G.o0; a < G.o1;) {
                    const uint32_t z = std::min<uint32_t>(G.o1, (a / GZ_TWIN_STRIPE + 1) * GZ_TWIN_STRIPE);
                    c ^= inf_crc_shift(inf_crc(tab.t, o + a, z - a), G.o1 - z);
                    a = z;
                }
                seg_crc[L.seg0 + g] = c;
            }
        }
        carry = w;
        sym_big.clear(); seg_big.clear();
        *bytes = out.data();
        return true;
    }
    bool windows_out(const uint32_t *link, uint32_t k, uint8_t *dst) {
        for (uint32_t i = 0; i < k; ++i) memcpy(dst + (size_t)i * GZ_WIN, wins.data() + (size_t)link[i] * GZ_WIN, GZ_WIN);
        return true;
    }
};

// the twin's memory side of the seeded environment: one lane that walks every stripe, plain bytes, a word as four bytes
struct GzSeedTwinMem {
    static uint8_t ld(const uint8_t *p) { return *p; }
    static void st(uint8_t *p, uint8_t v) { *p = v; }
    static void word(uint8_t *p, uint32_t w) { memcpy(p, &w, 4); }
    static uint32_t wave_xor(uint32_t c) { return c; }
};
typedef GzSeedEnv<TwinTabs, GzSeedTwinMem> GzSeedTwinEnv;

// Entry i of map m decoded from its seed out of file d[0, n) (which need not be the census's: a damaged copy) with window `win`
// (GZ_WIN bytes, null for none) into out[skew, skew + len), `out` 4-byte aligned.  The status word of gz_entry_run; an
// entry whose bytes the file does not hold is INF_E_INPUT
static inline uint32_t gz_twin_entry(const FxSeekMap &m, uint64_t i, const uint8_t *d, uint64_t n, const uint8_t *win, uint8_t *out, uint32_t skew) {
    static const CrcTab tab;
    uint32_t pw[32];
    gz_crc_powers(pw, 32);
    const FxGzEntry &e = m.ent[i];
    const bool last = i + 1 == m.ent.size();
    const uint64_t c0 = e.bit >> 3, c1 = fx_gz_cover_end(m, i);
    if (c1 > n || c0 > c1 || c1 - c0 >= ((uint64_t)1 << 29) || e.len >> 32) return INF_E_INPUT;
    GzEntryTask t = {c0, skew, (uint32_t)(c1 - c0), (uint32_t)(e.bit & 7), last ? GZ_NONE : (uint32_t)(m.ent[i + 1].bit - 8 * c0), (uint32_t)e.len, e.crc, e.valid,
                     win ? 0u : GZ_NONE, last ? 1u : 0u};
    std::vector<uint8_t> ring(GZ_RING, 0xEE);        // (stale bytes a decode must never read: not zeros)
    GzSeedTwinEnv env(ring.data(), tab.t, pw, out + skew, skew & 3, t.len, t.valid);
    if (win) env.preload(win);
    return gz_entry_run(env, d + c0, t);
}


