// gzip_twin.cpp -- the host twin of the speculative gzip decode (g++): gzip_round.h's rounds and chain walk over a sequential
// backend that runs the finder, the marker decodes (gzip_core.h), the window propagation, the resolve and the lane-stripe
// segment CRCs the way the kernels of k_gzip.h do, so the CPU suite checks the whole algorithm against zlib with no GPU
// (tests/test_gzip_twin.py).  TEST INFRASTRUCTURE, not part of the product library.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "gzip_core.h"
#include "gzip_round.h"
#include "twin_env.h"

#define GZ_TWIN_STRIPE 1024u      // bytes per lane stripe of k_gz_resolve

namespace {
struct Env : TwinTabs {
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

struct Twin {
    const uint8_t *p = nullptr;
    uint32_t n = 0;
    std::vector<uint16_t> sym;
    std::vector<GzSeg> seg;
    std::vector<std::vector<uint16_t>> sym_big;      // retry buffers of the round
    std::vector<std::vector<GzSeg>> seg_big;
    std::vector<uint8_t> carry = std::vector<uint8_t>(GZ_WIN, 0), out;
    uint8_t tab[128]; uint16_t cnt[32];

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
            Env e;
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
        for (uint32_t k = 0; k < nl; ++k) {
            const GzLink &L = l[k];
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
};

std::vector<uint8_t> g_out;
}  // namespace

extern "C" {

// the whole algorithm with chunk / round / slot-ratio parameters.  0: the bytes are ready (gzip_twin_result); -1: too many
// symbols for the slots (the library's TOO_MANY); > 0: the INF_E_* / GZ_E_* status, *bad_off the chunk's file offset.
// stats[7]: members, chunks, speculative, rejected, redecoded, overflow retries, bytes out.
int gzip_twin_inflate(const uint8_t *d, uint64_t n, uint64_t chunk, uint64_t round, uint64_t ratio, uint64_t *stats, uint64_t *bad_off) {
    Twin t;
    g_out.clear();
    GzStats st;
    const int rc = gz_run(t, d, n, GzCfg{chunk, round, ratio}, [&](const uint8_t *b, uint64_t k) { g_out.insert(g_out.end(), b, b + k); return true; }, st, bad_off);
    if (stats) { stats[0] = st.members; stats[1] = st.chunks; stats[2] = st.speculative; stats[3] = st.rejected; stats[4] = st.redecoded; stats[5] = st.overflow_retries; stats[6] = st.bytes_out; }
    return rc == GZ_RUN_TOO_MANY ? -1 : rc;
}

uint64_t gzip_twin_result(uint8_t *dst) { if (dst && !g_out.empty()) memcpy(dst, g_out.data(), g_out.size()); return g_out.size(); }

// the finder's candidate for bit range [b0, b1) of d, or GZ_NONE
uint32_t gzip_twin_find(const uint8_t *d, uint32_t n, uint32_t b0, uint32_t b1) {
    uint8_t tab[128]; uint16_t cnt[32];
    for (uint32_t b = b0; b < b1; ++b) if (gz_maybe_candidate(d, n, b) && gz_is_candidate(d, n, b, tab, cnt)) return b;
    return GZ_NONE;
}

// the true boundaries of a serial decode (the stop rule applied one boundary at a time), with their kind: 1 member header,
// 2 canonical non-final stored block, 3 non-final dynamic block, 0 any other block.  Returns the count (or -status).
int gzip_twin_boundaries(const uint8_t *d, uint32_t n, uint32_t *bits, uint32_t *kind, uint32_t cap) {
    std::vector<uint16_t> sym((size_t)n * 1100 + 65536);
    std::vector<GzSeg> seg(4096);
    uint32_t at = 0, k = 0;
    while (k < cap) {
        const bool hdr = (at & 7) == 0 && gz_is_header(d, n, at >> 3);
        uint32_t b = at;
        bits[k] = at;
        kind[k++] = hdr ? 1 : gz_stored_at(d, n, at) ? 2 : gz_bits(d, n, &b, 3) == 4 ? 3 : 0;
        Env e;
        e.out = sym.data(); e.sp = seg.data(); e.cap = (uint32_t)sym.size();
        GzRes r;
        gz_decode(e, d, n, true, at, at + 1, (uint32_t)seg.size(), r);
        if (r.status) return -(int)r.status;
        if (r.eof) return (int)k;
        at = r.end_bit;
    }
    return (int)k;
}

}  // extern "C"
