// inflate_twin.cpp -- the host twin of k_inflate (g++): the same decoder (inflate_core.h) and block scan (bgzf_scan.h)
// with a sequential environment, and the block CRC over 64 emulated lane stripes, so the CPU suite checks the decoding
// logic against zlib with no GPU (tests/test_bgzf_twin.py).  TEST INFRASTRUCTURE, not part of the product library.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "bgzf_scan.h"
#include "twin_env.h"

namespace {
struct TwinEnv : TwinTabs {
    static constexpr int full = INF_E_OUTPUT;
    uint8_t *out;
    uint32_t pos = 0, cap;
    uint32_t reach() const { return pos; }
    void lit(uint8_t b) { out[pos++] = b; }
    void copy(uint32_t dist, uint32_t len) { for (uint32_t j = 0; j < len; ++j, ++pos) out[pos] = out[pos - dist]; }
    void stored(const uint8_t *src, uint32_t n) { memcpy(out + pos, src, n); pos += n; }
};

// the block's CRC as the kernel forms it: 64 stripes, each shifted past the bytes after it, XOR-combined
uint32_t crc_striped(const uint8_t *d, uint32_t n) {
    static const CrcTab tab;
    uint32_t c = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) c ^= inf_crc_stripe(tab.t, d, n, lane, 64);
    return c;
}
}  // namespace

extern "C" {

// raw deflate of exactly `cap` output bytes: INF_* status
int inflate_twin_raw(const uint8_t *comp, uint32_t len, uint8_t *out, uint32_t cap) {
    TwinEnv e;
    e.out = out; e.cap = cap;
    return inf_raw(e, comp, 0, len);
}

uint32_t inflate_twin_crc(const uint8_t *d, uint32_t n) { return crc_striped(d, n); }

// 0: BGZF, *n_blocks / *out_len set; -2: not BGZF
int inflate_twin_scan(const uint8_t *d, uint64_t n, uint64_t *n_blocks, uint64_t *out_len) {
    std::vector<BgzfBlock> t;
    if (!bgzf_scan_blocks(d, n, &t, out_len)) return -2;
    *n_blocks = t.size();
    return 0;
}

// the block table of the whole buffer, for comparison: 0 and the first min(cap, *n_blocks) records copied to tab (7 words a block:
// c_off, o_off, d_off, d_len, c_len, isize, crc); -2: not BGZF
static void twin_table_out(const std::vector<BgzfBlock> &t, uint64_t *tab, uint64_t cap) {
    for (size_t i = 0; i < t.size() && i < cap; ++i) {
        const BgzfBlock &b = t[i];
        const uint64_t w[7] = {b.c_off, b.o_off, b.d_off, b.d_len, b.c_len, b.isize, b.crc};
        memcpy(tab + 7 * i, w, sizeof w);
    }
}
int inflate_twin_scan_table(const uint8_t *d, uint64_t n, uint64_t *tab, uint64_t cap, uint64_t *n_blocks, uint64_t *out_len) {
    std::vector<BgzfBlock> t;
    if (!bgzf_scan_blocks(d, n, &t, out_len)) return -2;
    *n_blocks = t.size();
    twin_table_out(t, tab, cap);
    return 0;
}

// the incremental walk (BgzfWalk) over the same buffer cut into pieces of `piece` bytes: 0 and the table as above; -2: refused,
// *bad_off the file offset the walk names
int inflate_twin_walk_pieces(const uint8_t *d, uint64_t n, uint64_t piece, uint64_t *tab, uint64_t cap, uint64_t *n_blocks, uint64_t *out_len, uint64_t *bad_off) {
    std::vector<BgzfBlock> t;
    BgzfWalk w;
    bool ok = piece != 0;
    for (uint64_t at = 0; ok && at < n; at += piece) ok = w.feed(d + at, piece < n - at ? piece : n - at, &t);
    if (!ok || !w.end()) { *bad_off = w.bad_off; return -2; }
    *n_blocks = t.size(); *out_len = w.o;
    twin_table_out(t, tab, cap);
    return 0;
}

// the whole file: 0 and out_len bytes in `out` (out_cap >= the scan's out_len); -2: not BGZF; > 0: the INF_* status of
// the first bad block, whose file offset goes to *bad_off
int inflate_twin_bgzf(const uint8_t *d, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *bad_off) {
    std::vector<BgzfBlock> t;
    uint64_t total = 0;
    if (!bgzf_scan_blocks(d, n, &t, &total) || total > out_cap) return -2;
    TwinEnv e;
    for (const BgzfBlock &b : t) {
        e.out = out + b.o_off; e.pos = 0; e.cap = b.isize;
        int rc = inf_raw(e, d + b.c_off, b.d_off, b.d_off + b.d_len);
        if (!rc && crc_striped(out + b.o_off, b.isize) != b.crc) rc = INF_E_CRC;
        if (rc) { if (bad_off) *bad_off = b.c_off; return rc; }
    }
    return 0;
}

}  // extern "C"
