// bz_twin.cpp -- the host twin of the block-parallel bzip2 decode (g++): bz_round.h's rounds and chain over a sequential backend
// that runs the finder, the block decode, the scatter, the walk and the run-length layer of bz_core.h the way the kernels of
// k_bzip2.h do, so the CPU suite checks the whole algorithm against libbz2 with no GPU (tests/test_bzip2_twin.py).
// TEST INFRASTRUCTURE, not part of the product library.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "bz_core.h"
#include "bz_round.h"

namespace {
struct Env {
    static constexpr uint32_t PER = 256;
    BzTabs tabs;
    BzTabs *t = &tabs;
    uint32_t lane = 0, nl = 1;
    void sync() {}
};

// every bit offset of d[0, n) that carries a magic, ascending
void find_all(const uint8_t *d, uint64_t n, std::vector<uint64_t> &cand) {
    for (uint64_t q = 0; q + 6 <= n; ++q) {
        const uint64_t w = bz_be64(d, n, q);
        for (uint32_t s = 0; s < 8; ++s) {
            const uint32_t kind = bz_magic_in(w, s);
            if (kind && 8 * q + s + 48 <= 8 * n) cand.push_back((8 * q + s) | (kind == 2 ? BZ_END_FLAG : 0));
        }
    }
}

struct Twin {
    const uint8_t *p = nullptr;
    uint64_t n = 0;
    uint32_t bs = 0;
    std::vector<uint8_t> L, out;
    std::vector<uint32_t> cnt, tt;
    Env env;
    uint32_t crc_tab[256];
    Twin() { bz_crc_table(crc_tab, 0, 1); }
    bool load(const uint8_t *d, uint64_t len) { p = d; n = len; return true; }
    bool find(std::vector<uint64_t> &cand) { find_all(p, n, cand); return true; }
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
        for (uint32_t a = 0; a < m; ++a) {
            uint8_t *Lc = L.data() + (size_t)l[a].slot * bs;
            tt.resize(l[a].n);
            bz_scatter(Lc, l[a].n, &cnt[(size_t)l[a].slot * 256], tt.data());
            if (!bz_walk(tt.data(), l[a].n, l[a].orig, Lc)) return false;
            const uint64_t len = bz_rle_len(Lc, l[a].n);
            l[a].out_off = total; l[a].run_open = (len & BZ_RUN_OPEN) != 0;
            total += len & ~BZ_RUN_OPEN;
        }
        out.resize(total + 4);
        for (uint32_t a = 0; a < m; ++a) crc[a] = bz_rle_write(L.data() + (size_t)l[a].slot * bs, l[a].n, crc_tab, out.data() + l[a].out_off);
        *out_bytes = total; *bytes = out.data();
        return true;
    }
};

std::vector<uint8_t> g_out;
}  // namespace

extern "C" {

// the whole algorithm with `round_blocks` candidates per round (0: as many as the driver allows).  cand / n_cand: a candidate
// list instead of the finder's (n_cand < 0: the finder).  0: the bytes are ready (bz_twin_result); > 0: the BZ_E_* status,
// *bad_off its byte offset.  stats[5]: blocks, candidates, rejected candidates, rounds, bytes out.
int bz_twin_inflate(const uint8_t *d, uint64_t n, uint64_t round_blocks, const uint64_t *cand, int64_t n_cand, uint64_t *stats, uint64_t *bad_off) {
    Twin t;
    g_out.clear();
    BzStats st;
    std::vector<uint64_t> given;
    if (n_cand >= 0) given.assign(cand, cand + n_cand);
    const int rc = bz_run(t, d, n, round_blocks, [&](const uint8_t *b, uint64_t k) { g_out.insert(g_out.end(), b, b + k); return true; }, st, bad_off,
                          n_cand >= 0 ? &given : nullptr);
    if (stats) { stats[0] = st.blocks; stats[1] = st.candidates; stats[2] = st.rejected; stats[3] = st.rounds; stats[4] = st.bytes_out; }
    return rc;
}

uint64_t bz_twin_result(uint8_t *dst) { if (dst && !g_out.empty()) memcpy(dst, g_out.data(), g_out.size()); return g_out.size(); }

// the finder: every candidate of d[0, n) (BZ_END_FLAG: the end-of-stream magic), at most cap of them written; returns the count
uint64_t bz_twin_find(const uint8_t *d, uint64_t n, uint64_t *cand, uint64_t cap) {
    std::vector<uint64_t> c;
    find_all(d, n, c);
    for (uint64_t i = 0; i < c.size() && i < cap; ++i) cand[i] = c[i];
    return c.size();
}

}  // extern "C"
