// bz_twin.cpp -- the host twin of the block-parallel bzip2 decode (g++): bz_round.h's rounds and chain over the sequential backend
// of bz_twin.h, which runs the finder, the block decode, the scatter, the walk and the run-length layer of bz_core.h the way the kernels of
// k_bzip2.h do, so the CPU suite checks the whole algorithm against libbz2 with no GPU (tests/test_bzip2_twin.py).
// TEST INFRASTRUCTURE, not part of the product library.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "bz_twin.h"

namespace {
std::vector<uint8_t> g_out;
}  // namespace

extern "C" {

// the whole algorithm with `round_blocks` candidates per round (0: as many as the driver allows).  cand / n_cand: a candidate
// list instead of the finder's (n_cand < 0: the finder).  0: the bytes are ready (bz_twin_result); > 0: the BZ_E_* status,
// *bad_off its byte offset.  stats[5]: blocks, candidates, rejected candidates, rounds, bytes out.
int bz_twin_inflate(const uint8_t *d, uint64_t n, uint64_t round_blocks, const uint64_t *cand, int64_t n_cand, uint64_t *stats, uint64_t *bad_off) {
    BzTwin t;
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
    bz_twin_find_all(d, n, c);
    for (uint64_t i = 0; i < c.size() && i < cap; ++i) cand[i] = c[i];
    return c.size();
}

}  // extern "C"
