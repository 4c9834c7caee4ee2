// gzip_twin.cpp -- the host twin of the speculative gzip decode (g++): gzip_round.h's rounds and chain walk over a sequential
// backend that runs the finder, the marker decodes (gzip_core.h), the window propagation, the resolve and the lane-stripe
// segment CRCs the way the kernels of k_gzip.h do, so the CPU suite checks the whole algorithm against zlib with no GPU
// (tests/test_gzip_twin.py).  TEST INFRASTRUCTURE, not part of the product library.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "gz_twin.h"

namespace {
std::vector<uint8_t> g_out;
}  // namespace

extern "C" {

// the whole algorithm with chunk / round / slot-ratio parameters.  0: the bytes are ready (gzip_twin_result); -1: too many
// symbols for the slots (the library's TOO_MANY); > 0: the INF_E_* / GZ_E_* status, *bad_off the chunk's file offset.
// stats[7]: members, chunks, speculative, rejected, redecoded, overflow retries, bytes out.
int gzip_twin_inflate(const uint8_t *d, uint64_t n, uint64_t chunk, uint64_t round, uint64_t ratio, uint64_t *stats, uint64_t *bad_off) {
    GzTwin t;
    g_out.clear();
    GzStats st;
    const int rc = gz_run(t, d, n, GzCfg{chunk, round, ratio}, [&](const uint8_t *b, uint64_t k) { g_out.insert(g_out.end(), b, b + k); return true; }, st, bad_off);
    if (stats) { stats[0] = st.members; stats[1] = st.chunks; stats[2] = st.speculative; stats[3] = st.rejected; stats[4] = st.redecoded; stats[5] = st.overflow_retries; stats[6] = st.bytes_out; }
    return rc == GZ_RUN_TOO_MANY ? -1 : rc;
}

// the same call with the recorder of a seek map beside it (gzip_round.h GzSeekRec at `spacing`): the bytes and the statistics must be
// what they are without one.  Returns as gzip_twin_inflate; *entries: how many entries the recorder kept
int gzip_twin_inflate_rec(const uint8_t *d, uint64_t n, uint64_t chunk, uint64_t round, uint64_t ratio, uint64_t spacing, uint64_t *stats, uint64_t *bad_off, uint64_t *entries) {
    GzTwin t;
    t.keep_wins = true;
    g_out.clear();
    GzStats st;
    FxSeekMap m;
    GzSeekRec<GzTwin> rec = {&m, spacing ? spacing : 1};
    const int rc = gz_run(t, d, n, GzCfg{chunk, round, ratio}, [&](const uint8_t *b, uint64_t k) { g_out.insert(g_out.end(), b, b + k); return true; }, st, bad_off, &rec);
    if (stats) { stats[0] = st.members; stats[1] = st.chunks; stats[2] = st.speculative; stats[3] = st.rejected; stats[4] = st.redecoded; stats[5] = st.overflow_retries; stats[6] = st.bytes_out; }
    if (entries) *entries = m.ent.size();
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
        GzTwinEnv e;
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
