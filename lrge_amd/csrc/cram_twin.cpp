// cram_twin.cpp -- the host twin of the CRAM device ingest (g++): cram_round.h's walk, stream heads and rounds over a sequential
// backend that runs the block decode of rans_core.h the way k_rans_decode does -- all 64 lanes of a step, phase by phase, so the
// ballots, the lane-ordered renormalisation, the LDS / global choice of the model and the expansions are the device's -- and the
// CPU suite checks the whole algorithm against the host reader with no GPU (tests/test_cram_twin.py); and the sampled ingest of
// DESIGN section 27 -- cram_sampled over a backend of the device's shape, whose scratch is a heap block of exactly the round's raw
// size and whose store one of exactly the chosen bases (tests/test_cram_select_twin.py).
// TEST INFRASTRUCTURE, not part of the product library.
#include <stdint.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "cram_round.h"

namespace {
struct Env {
    static constexpr uint32_t NV = 64;
    uint32_t lane0() const { return 0; }
    uint32_t lane1() const { return 64; }
    void sync() {}
    uint64_t ballot(const bool *f) const { uint64_t m = 0; for (int l = 0; l < 64; ++l) m |= (uint64_t)f[l] << l; return m; }
    uint64_t excl_scan(const uint64_t *v, uint64_t *at) const { uint64_t x = 0; for (int l = 0; l < 64; ++l) { at[l] = x; x += v[l]; } return x; }
};

struct Twin {
    uint8_t *out = nullptr;
    // every buffer of a round is a heap block of its exact size, so a sanitizer sees a step outside it (tools/cram_check.cpp)
    bool round(const uint8_t *in, size_t in_bytes, const RansBlk *blk, uint32_t m, const RansTables &t, uint64_t tmp_bytes, uint32_t *status) {
        std::unique_ptr<uint8_t[]> in_x(new uint8_t[in_bytes ? in_bytes : 1]), tmp(new uint8_t[tmp_bytes ? tmp_bytes : 1]), aux(new uint8_t[t.aux.size() ? t.aux.size() : 1]);
        std::unique_ptr<uint16_t[]> tabs(new uint16_t[t.tabs.size() ? t.tabs.size() : 1]), lds(new uint16_t[RANS_LDS_U16]);
        std::unique_ptr<uint32_t[]> runs(new uint32_t[t.runs.size() ? t.runs.size() : 1]);
        if (in_bytes) memcpy(in_x.get(), in, in_bytes);
        if (!t.aux.empty()) memcpy(aux.get(), t.aux.data(), t.aux.size());
        if (!t.tabs.empty()) memcpy(tabs.get(), t.tabs.data(), t.tabs.size() * 2);
        if (!t.runs.empty()) memcpy(runs.get(), t.runs.data(), t.runs.size() * 4);
        Env env;
        for (uint32_t a = 0; a < m; ++a) {
            memset(lds.get(), 0xA5, RANS_LDS_U16 * 2);              // (LDS keeps nothing from block to block)
            status[a] = rans_block(env, in_x.get(), blk[a], tabs.get(), aux.get(), runs.get(), lds.get(), RANS_LDS_U16, tmp.get(), out);
        }
        return true;
    }
};

// the sink of the sampled ingest, as CramKeepDev (host_cram.inl): a round is decoded into a scratch of its raw size by the backend
// above on rebased descriptors, then the chosen reads' ranges are copied to the store.  Every copy is checked against both blocks
struct KeepTwin {
    const CramWalk *cw = nullptr;
    const CramKeepPlan *plan = nullptr;
    const uint32_t *sel = nullptr;
    std::unique_ptr<uint8_t[]> store;
    uint64_t store_bytes = 0, at = 0, scratch_max = 0, copies = 0;
    bool begin(const CramWalk &w, const CramKeepPlan &p, const uint32_t *s, uint64_t) {
        cw = &w; plan = &p; sel = s; at = 0;
        store_bytes = p.dst.back();
        store.reset(new uint8_t[store_bytes ? store_bytes : 1]());
        return true;
    }
    bool round(const uint8_t *in, size_t in_bytes, const RansBlk *blk, uint32_t m, const RansTables &t, uint64_t tmp_bytes, uint32_t *status) {
        std::vector<RansBlk> b(blk, blk + m);
        std::vector<uint64_t> scr(m);
        const uint64_t raw = cram_rebase(b.data(), m, scr.data());
        std::unique_ptr<uint8_t[]> scratch(new uint8_t[raw ? raw : 1]);      // (exactly the round's raw size: a sanitizer sees a block that writes past its place)
        scratch_max = std::max(scratch_max, raw);
        Twin tw; tw.out = scratch.get();
        tw.round(in, in_bytes, b.data(), m, t, tmp_bytes, status);
        bool good = true;
        for (uint32_t a = 0; a < m; ++a) good = good && status[a] == RANS_OK;
        std::vector<CramCopy> c;
        if (good) cram_round_copies(*cw, *plan, sel, at, m, scr.data(), c);
        for (const CramCopy &x : c) {
            if (x.src + x.len > raw || x.dst + x.len > store_bytes) return false;
            memcpy(store.get() + x.dst, scratch.get() + x.src, x.len);
        }
        copies += c.size();
        at += m;
        return true;
    }
};

std::string g_why;
CramSampled g_s;
KeepTwin g_keep;
FxSeekMap g_map;
CramWalk g_walk;
std::unique_ptr<uint8_t[]> g_bases;
uint64_t g_n_bases = 0;
}  // namespace

extern "C" {

// the layout of lrge_hip_rans_stream
struct cram_twin_stream { uint64_t offset; uint32_t length, raw_size, method, status; };

const char *cram_twin_why() { return g_why.c_str(); }

// lrge_hip_rans_decode on the host: stream i of comp decoded to out at the sum of the raw sizes before it; stats: CRAM_STAT_WORDS
// words.  0, or -1: a stream outside comp or an output above out_cap
int cram_twin_rans_decode(const uint8_t *comp, uint64_t comp_len, cram_twin_stream *s, uint32_t n, uint8_t *out, uint64_t out_cap, uint64_t round_bytes, uint64_t *stats) {
    g_why.clear();
    std::vector<RansStream> v;
    uint64_t o = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (s[i].offset > comp_len || s[i].length > comp_len - s[i].offset || (s[i].raw_size >> 31)) return -1;
        v.push_back(RansStream{comp + s[i].offset, s[i].length, (int)s[i].method, (int64_t)s[i].raw_size, o});
        o += s[i].raw_size;
    }
    if (o > out_cap) return -1;
    // the output as a heap block of its exact size
    std::unique_ptr<uint8_t[]> dense(new uint8_t[o ? o : 1]());
    Twin t; t.out = dense.get();
    CramStats st;
    std::vector<uint32_t> status(n, 0);
    cram_run(t, v, round_bytes ? round_bytes : ~(uint64_t)0, false, st, status.data(), g_why);
    for (uint32_t i = 0; i < n; ++i) s[i].status = status[i];
    if (o) memcpy(out, dense.get(), o);
    if (stats) cram_stats_words(st, stats);
    return 0;
}

// lrge_hip_reads_open | LRGE_GPU_INGEST_CRAM on the host.  0: the handle's tables are ready (cram_twin_count, cram_twin_table);
// 1: not proven (cram_twin_why)
int cram_twin_open(const uint8_t *d, uint64_t n, uint64_t round_bytes, uint64_t min_blocks, uint64_t *stats) {
    g_why.clear(); g_walk = CramWalk(); g_bases.reset(); g_n_bases = 0;
    CramStats st;
    const uint64_t t0 = cram_now_us();
    if (!cram_walk(d, n, g_walk, g_why)) return 1;
    st.walk_us = cram_now_us() - t0;
    st.containers = g_walk.w.containers; st.slices = g_walk.w.ba.size(); st.records = g_walk.w.recs.size();
    const std::vector<RansStream> s = cram_streams(g_walk);
    if (s.size() < min_blocks) { g_why = "fewer BA blocks than CRAM_MIN_BLOCKS"; return 1; }
    g_n_bases = g_walk.ba_out.back();
    g_bases.reset(new uint8_t[g_n_bases ? g_n_bases : 1]());
    Twin t; t.out = g_bases.get();
    if (cram_run(t, s, round_bytes ? round_bytes : ~(uint64_t)0, true, st, nullptr, g_why) != 0) return 1;
    if (stats) cram_stats_words(st, stats);
    return 0;
}

uint64_t cram_twin_count() { return g_walk.w.recs.size(); }
uint64_t cram_twin_name_bytes() { return g_walk.names.size(); }
uint64_t cram_twin_base_bytes() { return g_n_bases; }
// seq_len[n], name_off[n + 1], names, base_off[n] (where a record's bases start in the dense store), bases
void cram_twin_table(uint32_t *seq_len, uint64_t *name_off, char *names, uint64_t *base_off, uint8_t *bases) {
    const auto &r = g_walk.w.recs;
    for (size_t i = 0; i < r.size(); ++i) { seq_len[i] = r[i].len; base_off[i] = g_walk.ba_out[r[i].slice] + r[i].off; }
    memcpy(name_off, g_walk.name_off.data(), g_walk.name_off.size() * 8);
    if (!g_walk.names.empty()) memcpy(names, g_walk.names.data(), g_walk.names.size());
    if (g_n_bases) memcpy(bases, g_bases.get(), g_n_bases);
}

// ---- the sampled ingest ----
// what: 0 the census (sel ignored), 1 the selected open, 2 the census that leaves the map, 3 the mapped open on the last map.
// 0: done; 1: not proven (cram_twin_why); 2: an ordinal at or above the records; 3: the map is of another input; 4: the map does not
// fit the input; 5: over `cap` (0: no cap); -1: the backend failed; -2: the ordinals are not strictly ascending
int cram_twin_sampled(int what, const uint8_t *d, uint64_t n, const uint32_t *sel, uint64_t k, uint64_t round_bytes, uint64_t min_blocks, uint64_t cap, uint64_t out[4]) {
    g_why.clear(); g_s = CramSampled(); g_keep = KeepTwin();
    out[0] = out[1] = out[2] = out[3] = 0;
    if (what == 0 || what == 2) k = 0;
    if ((k && !sel) || !fx_sel_ascending(sel, k)) return -2;
    if (what == 2) g_map = FxSeekMap();
    const int rc = cram_sampled(g_keep, d, n, sel, k, what == 3, what >= 2 ? &g_map : nullptr, min_blocks, round_bytes ? round_bytes : (uint64_t)256 << 20, cap ? cap : ~(uint64_t)0, g_s, g_why);
    if (rc) { g_keep = KeepTwin(); g_s.cw = CramWalk(); return rc == CRAM_S_BACKEND ? -1 : rc; }
    out[0] = g_s.cw.w.recs.size(); out[1] = out[2] = g_s.cw.ba_out.back(); out[3] = 0;
    return 0;
}

// of the last cram_twin_sampled: the kept reads, the store bytes, the largest scratch, the rounds' copies; stats: CRAM_STAT_WORDS words;
// seek: runs, raw bytes decoded, compressed bytes uploaded, blocks decoded (a mapped open); round: the round size the pass ran at
uint64_t cram_twin_kept() { return g_s.cw.name_off.empty() ? 0 : g_s.cw.name_off.size() - 1; }      // (a refused call keeps nothing)
uint64_t cram_twin_kept_name_bytes() { return g_s.cw.names.size(); }
void cram_twin_sampled_stats(uint64_t *stats, uint64_t seek[4], uint64_t mem[4]) {
    cram_stats_words(g_s.st, stats);
    memcpy(seek, g_s.seek, sizeof g_s.seek);
    mem[0] = g_keep.store_bytes; mem[1] = g_keep.scratch_max; mem[2] = g_keep.copies; mem[3] = g_s.round_bytes;
}
// seq_len[kept], name_off[kept + 1], names, base_off[kept] (in the store), the store
void cram_twin_kept_table(const uint32_t *sel, uint32_t *seq_len, uint64_t *name_off, char *names, uint64_t *base_off, uint8_t *store) {
    const uint64_t k = cram_twin_kept();
    for (uint64_t j = 0; j < k; ++j) { seq_len[j] = g_s.cw.w.recs[sel[j]].len; base_off[j] = g_s.plan.dst[j]; }
    memcpy(name_off, g_s.cw.name_off.data(), g_s.cw.name_off.size() * 8);
    if (!g_s.cw.names.empty()) memcpy(names, g_s.cw.names.data(), g_s.cw.names.size());
    if (g_keep.store_bytes) memcpy(store, g_keep.store.get(), g_keep.store_bytes);
}
// the last map: out = {records, points, slices, bases, file length}; the points (ordinal, base offset, file offset of the BA block, slice)
void cram_twin_map(uint64_t out[5]) { out[0] = g_map.records; out[1] = g_map.pts.size(); out[2] = g_map.n_blocks; out[3] = g_map.bases; out[4] = g_map.file_len; }
uint64_t cram_twin_map_points(uint64_t *ord, uint64_t *off, uint64_t *c_off, uint64_t *slice, uint64_t cap) {
    for (uint64_t i = 0; i < g_map.pts.size() && i < cap; ++i) { ord[i] = g_map.pts[i].ord; off[i] = g_map.pts[i].off; c_off[i] = g_map.pts[i].c_off; slice[i] = g_map.pts[i].blk; }
    return g_map.pts.size();
}
// the walk's (slice, offset, length) of every record of the last call and the BA block of every slice (compressed size, raw size):
// what a test counts the mapped statistics from
uint64_t cram_twin_walk_recs(uint32_t *slice, uint32_t *len, uint64_t cap) {
    const auto &r = g_s.cw.w.recs;
    for (uint64_t i = 0; i < r.size() && i < cap; ++i) { slice[i] = r[i].slice; len[i] = r[i].len; }
    return r.size();
}
uint64_t cram_twin_walk_slices(uint64_t *comp, uint64_t *raw, uint64_t cap) {
    const auto &b = g_s.cw.w.ba;
    for (uint64_t i = 0; i < b.size() && i < cap; ++i) { comp[i] = b[i].data || b[i].raw_size ? b[i].size : ~(uint64_t)0; raw[i] = (uint64_t)b[i].raw_size; }
    return b.size();
}

}  // extern "C"
