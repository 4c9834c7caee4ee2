// xz_twin.cpp -- the host twin of the block-parallel xz decode (g++): xz_round.h's walk, rounds and launches over a sequential
// backend that runs the chunk decode and the checks of xz_core.h the way the kernels of k_xz.h do -- with all 64 lanes of a step,
// so the staging, the ring, the 64-byte copy steps and the state slots are the device's -- and the CPU suite checks the whole
// algorithm against liblzma with no GPU (tests/test_xz_twin.py).
// TEST INFRASTRUCTURE, not part of the product library.
#include <stdint.h>
#include <string.h>

#include <memory>
#include <vector>

#include "xz_core.h"
#include "xz_round.h"

namespace {
struct Env {
    uint16_t probs[XZ_PROBS_MAX];
    uint8_t stage[XZ_STAGE], ring[XZ_RING];
    uint64_t tab[256], part[XZ_NL];
    uint32_t lane0() const { return 0; }
    uint32_t lane1() const { return XZ_NL; }
    void sync() {}
};

struct Twin {
    const uint8_t *p = nullptr;
    const XzChunk *chunks = nullptr;
    uint64_t budget = ~(uint64_t)0, base = 0;
    bool too_big = false;
    std::unique_ptr<uint8_t[]> text, slots;        // heap blocks of the exact size, so a sanitizer sees a step outside them (tools/xz_check.cpp)
    uint64_t text_size = 0;
    Env env;
    bool load(const uint8_t *d, uint64_t, const XzChunk *c, uint64_t) { p = d; chunks = c; return true; }
    uint32_t default_round(uint64_t) { return XZ_ROUND_MAX; }
    bool over() const { return too_big; }
    bool reserve(uint64_t bytes, uint32_t k) {
        if (base + bytes > budget) { too_big = true; return false; }
        std::unique_ptr<uint8_t[]> grown(new uint8_t[base + bytes]);
        if (base) memcpy(grown.get(), text.get(), base);
        if (bytes) memset(grown.get() + base, 0x5A, bytes);
        text = std::move(grown); text_size = base + bytes;
        slots.reset(new uint8_t[(size_t)k * XZ_SLOT_BYTES]());
        return true;
    }
    bool decode(const XzTask *t, uint32_t m, uint32_t *status, uint32_t *bad_chunk) {
        for (uint32_t a = 0; a < m; ++a) {
            memset(env.probs, 0xA5, sizeof env.probs);          // (LDS keeps nothing from launch to launch)
            memset(env.ring, 0xA5, sizeof env.ring);
            status[a] = xz_decode(env, p, chunks, t[a], text.get() + base, slots.get(), &bad_chunk[a]);
        }
        return true;
    }
    bool check(const XzSpan *s, uint32_t m, uint64_t *crc) {
        for (uint32_t a = 0; a < m; ++a) crc[a] = xz_check(env, text.get() + base + s[a].at, s[a].len, s[a].wide != 0);
        return true;
    }
    const uint8_t *commit(uint64_t bytes) { const uint8_t *r = text.get() + base; base += bytes; return r; }
};

std::vector<uint8_t> g_out;
}  // namespace

extern "C" {

// the whole algorithm with `round_blocks` blocks per round (0: as many as the driver allows), `launch_bytes` of text per block and
// launch (0: the default), the checks checked or not, at least `min_blocks` blocks, at most `budget` bytes of text (0: no limit).
// 0: the bytes are ready (xz_twin_result); > 0: the XZ_E_* status, *bad_off its byte offset.  stats[8]: streams, blocks, chunks,
// raw_chunks, checks_checked, rounds, launches, bytes_out, as lrge_hip_xz_stats
int xz_twin_inflate(const uint8_t *d, uint64_t n, uint64_t round_blocks, uint64_t launch_bytes, int check, uint64_t min_blocks, uint64_t budget, uint64_t *stats,
                    uint64_t *bad_off) {
    Twin t;
    if (budget) t.budget = budget;
    g_out.clear();
    XzStats st;
    const XzCfg cfg{round_blocks, launch_bytes, min_blocks, check != 0};
    const int rc = xz_run(t, d, n, cfg, [&](const uint8_t *b, uint64_t k) { g_out.insert(g_out.end(), b, b + k); return true; }, st, bad_off);
    if (stats) {
        const uint64_t v[8] = {st.streams, st.blocks, st.chunks, st.raw_chunks, st.checks_checked, st.rounds, st.launches, st.bytes_out};
        memcpy(stats, v, sizeof v);
    }
    return rc;
}

uint64_t xz_twin_result(uint8_t *dst) { if (dst && !g_out.empty()) memcpy(dst, g_out.data(), g_out.size()); return g_out.size(); }

// the CRC64 (wide) or CRC32 of d[0, n) by the lane stripes of xz_check
uint64_t xz_twin_crc(const uint8_t *d, uint64_t n, int wide) {
    static Env env;
    return xz_check(env, d, n, wide != 0);
}

}  // extern "C"
