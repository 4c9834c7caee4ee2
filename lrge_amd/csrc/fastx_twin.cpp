// fastx_twin.cpp -- the host twin of the device record scan (k_fastx.h, host_fastx.inl; g++): the same passes over the same
// core (fastx_core.h) run tile by tile on the CPU -- census, exclusive scans, table scatter, per-record rules, sequence gather --
// with the tile size a parameter, so the CPU suite checks the algorithm against the host parser with records and lines
// straddling tile edges (tests/test_fastx_twin.py).  TEST INFRASTRUCTURE, not part of the product library.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "fastx_core.h"

namespace {
struct Parsed {
    int fmt = FX_FMT_EMPTY;
    std::vector<FxRec> recs;
};
Parsed g;

// the masks of the 16-byte group at p (a multiple of 16), as a lane of the device passes forms them
FxMasks group_at(const uint8_t *t, uint64_t n, uint64_t p) {
    uint8_t b[16] = {0};
    const uint32_t nvalid = (uint32_t)(n - p < 16 ? n - p : 16);
    memcpy(b, t + p, nvalid);
    uint32_t w[4];
    memcpy(w, b, 16);
    return fx_group_masks(w[0], w[1], w[2], w[3], p ? t[p - 1] : '\n', p + 16 < n ? t[p + 16] : FX_EOT, nvalid);
}
uint32_t valid_mask(uint64_t n, uint64_t p) { return n - p < 16 ? (1u << (n - p)) - 1 : 0xFFFFu; }

void scan_exclusive(std::vector<uint32_t> &v) {            // (wraps modulo 2^32, as the device scan does)
    uint32_t s = 0;
    for (uint32_t &x : v) { const uint32_t c = x; x = s; s += c; }
}
}  // namespace

extern "C" {

// 0: proven (fastx_twin_count records), FX_UNPROVEN, FX_TOO_MANY.  `tile`: bytes per tile, a multiple of 16.
int fastx_twin_parse(const uint8_t *t, uint64_t n, uint64_t tile) {
    g = Parsed();
    if (tile < 16 || tile % 16) return -1;
    const uint64_t n_tiles = (n + tile - 1) / tile;
    // pass 1: the census of every tile
    std::vector<uint32_t> c_lf(n_tiles), c_rem(n_tiles), c_hdr(n_tiles);
    for (uint64_t k = 0; k < n_tiles; ++k)
        for (uint64_t p = k * tile; p < n && p < (k + 1) * tile; p += 16) {
            const FxMasks m = group_at(t, n, p);
            c_lf[k] += (uint32_t)__builtin_popcount(m.lf); c_rem[k] += (uint32_t)__builtin_popcount(m.rem); c_hdr[k] += (uint32_t)__builtin_popcount(m.hdr);
        }
    // the summary: totals, the first and last tile with a byte that stays, the exact positions inside them
    FxCensus c;
    memset(&c, 0, sizeof c);
    c.first = c.last = n;
    uint64_t t_first = n_tiles, t_last = n_tiles;
    for (uint64_t k = 0; k < n_tiles; ++k) {
        c.n_lf += c_lf[k]; c.n_rem += c_rem[k]; c.n_hdr += c_hdr[k];
        const uint64_t bytes = n - k * tile < tile ? n - k * tile : tile;
        if (c_rem[k] < bytes) { if (t_first == n_tiles) t_first = k; t_last = k; }
    }
    for (int side = 0; side < 2 && t_first < n_tiles; ++side) {
        const uint64_t k = side ? t_last : t_first;
        for (uint64_t p = k * tile; p < n && p < (k + 1) * tile; p += 16) {
            const uint32_t keep = ~group_at(t, n, p).rem & valid_mask(n, p);
            if (!keep) continue;
            if (!side) { if (c.first == n) c.first = p + (uint64_t)__builtin_ctz(keep); }
            else c.last = p + 31 - (uint64_t)__builtin_clz(keep);
        }
    }
    for (int i = 0; i < 4; ++i) c.head[i] = (uint64_t)i < n ? t[i] : 0;
    c.at_first = c.first < n ? t[c.first] : 0;
    c.tail = n ? t[n - 1] : 0;
    uint32_t verdict;
    const int fmt = fx_format(n, c, &verdict);
    if (verdict) return (int)verdict;
    g.fmt = fmt;
    if (fmt == FX_FMT_EMPTY) return 0;
    if ((verdict = fx_limits(fmt, c))) return (int)verdict;
    // the censuses become offsets
    scan_exclusive(c_lf); scan_exclusive(c_rem); scan_exclusive(c_hdr);
    uint32_t flags = 0;
    if (fmt == FX_FMT_FASTQ) {
        // pass 2: the line starts; the ranks of the first and last non-empty line come out of the same pass
        std::vector<uint64_t> ls(c.n_lf + 1);
        ls[0] = 0;
        uint64_t l0 = 0, l_last = 0;
        for (uint64_t k = 0; k < n_tiles; ++k) {
            uint64_t r = c_lf[k];
            for (uint64_t p = k * tile; p < n && p < (k + 1) * tile; p += 16) {
                const uint32_t lf = group_at(t, n, p).lf;
                if (c.first >= p && c.first < p + 16) l0 = r + (uint64_t)__builtin_popcount(lf & ((1u << (c.first - p)) - 1));
                if (c.last >= p && c.last < p + 16) l_last = r + (uint64_t)__builtin_popcount(lf & ((1u << (c.last - p)) - 1));
                for (uint32_t m = lf; m; m &= m - 1) ls[++r] = p + (uint64_t)__builtin_ctz(m) + 1;
            }
        }
        uint64_t n_lines, n_rec;
        fx_fastq_shape(n, c, l0, l_last, &n_lines, &n_rec);
        if (n_rec >> 32) return FX_TOO_MANY;
        g.recs.resize(n_rec);
        for (uint64_t r = 0; r < n_rec; ++r) flags |= fx_fastq_record(t, n, ls.data(), c.n_lf, n_lines, l0, r, &g.recs[r]);
    } else {
        // pass 2: where every header is and how many removed bytes lie in front of it
        std::vector<uint64_t> hpos(c.n_hdr);
        std::vector<uint32_t> hrem(c.n_hdr);
        for (uint64_t k = 0; k < n_tiles; ++k) {
            uint64_t r = c_hdr[k];
            uint32_t rem = c_rem[k];
            for (uint64_t p = k * tile; p < n && p < (k + 1) * tile; p += 16) {
                const FxMasks m = group_at(t, n, p);
                for (uint32_t h = m.hdr; h; h &= h - 1) {
                    const uint32_t i = (uint32_t)__builtin_ctz(h);
                    hpos[r] = p + i; hrem[r] = rem + (uint32_t)__builtin_popcount(m.rem & ((1u << i) - 1)); ++r;
                }
                rem += (uint32_t)__builtin_popcount(m.rem);
            }
        }
        g.recs.resize(c.n_hdr);
        for (uint64_t i = 0; i < c.n_hdr; ++i) flags |= fx_fasta_record(t, n, hpos.data(), hrem.data(), c.n_hdr, c.n_rem, i, &g.recs[i]);
    }
    if (flags) { g.recs.clear(); return flags & FX_UNPROVEN ? (int)FX_UNPROVEN : (int)FX_TOO_MANY; }
    return 0;
}

uint64_t fastx_twin_count(void) { return g.recs.size(); }
int fastx_twin_format(void) { return g.fmt; }
void fastx_twin_table(FxRec *out) { if (!g.recs.empty()) memcpy(out, g.recs.data(), g.recs.size() * sizeof(FxRec)); }

// the bases of record i into out[0, seq_len), as the device gather forms them: the span in 16-byte groups, removed bytes dropped;
// returns how many bytes were written
uint64_t fastx_twin_seq(const uint8_t *t, uint64_t n, uint64_t i, uint8_t *out) {
    const FxRec &r = g.recs[i];
    const uint64_t a = r.seq_off, b = r.seq_off + r.seq_span;
    uint64_t w = 0;
    for (uint64_t p = a & ~(uint64_t)15; p < b; p += 16) {
        uint32_t keep = ~group_at(t, n, p).rem & valid_mask(n, p);
        if (p < a) keep &= ~((1u << (a - p)) - 1);
        if (b - p < 16) keep &= (1u << (b - p)) - 1;
        for (; keep; keep &= keep - 1) out[w++] = t[p + (uint64_t)__builtin_ctz(keep)];
    }
    return w;
}

}  // extern "C"
