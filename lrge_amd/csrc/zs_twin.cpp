// zs_twin.cpp -- the host twin of the block-parallel Zstandard decode (g++): zs_round.h's walk, rounds and scan over a sequential
// backend that runs the heads, the literals, the sequences, the execution, the resolve and XXH64 of zs_core.h the way the kernels
// of k_zstd.h do -- with all 64 lanes of a step, so the 64-byte copy steps are the device's -- and the CPU suite checks the whole
// algorithm against libzstd with no GPU (tests/test_zstd_twin.py).
// TEST INFRASTRUCTURE, not part of the product library.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "zs_core.h"
#include "zs_round.h"

namespace {
struct Env {
    ZsTabs tabs;
    ZsTabs *t = &tabs;
    uint8_t tb[ZS_NL];
    uint32_t to[ZS_NL];
    uint32_t lane0() const { return 0; }
    uint32_t lane1() const { return ZS_NL; }
    uint32_t slot(uint32_t l) const { return l; }
    void sync() {}
};

struct Twin {
    const uint8_t *p = nullptr;
    uint64_t n = 0, budget = ~(uint64_t)0;
    bool too_big = false;
    std::vector<uint8_t> text, lit;
    std::vector<ZsSeq> seq;
    std::vector<uint32_t> org;
    Env env;
    // the sliding mode (zs_round.h): every round's work text [history | round] is a heap block of its own of exactly that many
    // bytes, so a read in front of the history or behind the round is a heap overflow under a sanitizer, not a silent hit
    bool sliding = false;
    uint8_t *work = nullptr;
    uint64_t work_len = 0, hist = 0, keep = 0;
    ZsXxh xs[2] = {};
    ~Twin() { delete[] work; }
    bool slides() const { return sliding; }
    bool plan(uint64_t) { return true; }
    bool slide(uint64_t history, uint64_t bytes) {
        if (history != keep || keep > work_len) return false;
        uint8_t *w = new uint8_t[history + bytes];
        if (history) memcpy(w, work + (work_len - history), history);
        delete[] work;
        work = w; work_len = history + bytes; hist = history;
        return true;
    }
    bool retire(uint64_t keep_bytes) { keep = keep_bytes; return keep_bytes <= work_len; }
    bool xxh64_part(const ZsXxhJob *job, uint32_t m, uint64_t *h) {
        for (uint32_t i = 0; i < m; ++i) {
            if (job[i].at + job[i].len > work_len) return false;
            h[i] = zs_xxh64_part(env, xs[job[i].slot & 1], work + job[i].at, job[i].len, (job[i].flags & 1) != 0, (job[i].flags & 2) != 0);
        }
        return true;
    }
    bool load(const uint8_t *d, uint64_t len) { p = d; n = len; return true; }
    uint32_t default_round() { return ZS_ROUND_MAX; }
    bool over() const { return too_big; }
    bool heads(ZsBlock *b, uint32_t k) {
        for (uint32_t j = 0; j < k; ++j) if (b[j].type == 2) zs_block_head(p + b[j].src, b[j].size, b[j].bmax, b[j].h);
        return true;
    }
    bool entropy(const ZsBlock *b, uint32_t k, uint64_t lit_bytes, uint64_t n_seq, uint32_t *lit_status, ZsSeqRes *res) {
        lit.assign(lit_bytes + 1, 0); seq.assign(n_seq + 1, ZsSeq{0, 0, 0});
        for (uint32_t j = 0; j < k; ++j) {
            if (b[j].type != 2) continue;
            lit_status[j] = zs_literals(env, p, n, b[j], lit.data() + b[j].lit_off);
            zs_sequences(env, p, n, b[j], seq.data() + b[j].seq_off, res[j]);
        }
        return true;
    }
    bool reserve(uint64_t bytes) {
        if (sliding) return true;
        if (text.size() + bytes > budget) { too_big = true; return false; }
        return true;
    }
    bool execute(const ZsBlock *b, uint32_t k, const uint32_t *group, uint32_t n_groups, uint64_t bytes, uint32_t *status) {
        const uint64_t base = sliding ? hist : text.size();
        if (!sliding) text.resize(base + bytes);
        uint8_t *const txt = sliding ? work : text.data();
        org.assign(bytes + 1, 0);
        bool good = true;
        for (uint32_t j = 0; j < k; ++j) {
            status[j] = zs_execute(env, p, b[j], lit.data() + b[j].lit_off, seq.data() + b[j].seq_off, txt, org.data() + (b[j].out - base));
            good = good && !status[j];
        }
        if (!good) return true;
        for (uint32_t g = 0; g < n_groups; ++g)
            for (uint32_t j = group[g]; j < group[g + 1]; ++j) zs_resolve_block(txt, org.data() + (b[j].out - base), b[j].out, b[j].out_size, 0, 1, 1);
        return true;
    }
    bool xxh64(const uint64_t *at, const uint64_t *len, uint32_t m, uint64_t *h) {
        for (uint32_t i = 0; i < m; ++i) h[i] = zs_xxh64(env, (sliding ? work : text.data()) + at[i], len[i]);
        return true;
    }
    const uint8_t *bytes(uint64_t at, uint64_t) { return (sliding ? work : text.data()) + at; }
};

std::vector<uint8_t> g_out;
}  // namespace

extern "C" {

// the whole algorithm with `round_blocks` blocks per round (0: as many as the driver allows), the checksums checked or not, at
// most `budget` bytes of text (0: no limit).  0: the bytes are ready (zs_twin_result); > 0: the ZS_E_* status, *bad_off its byte
// offset.  stats[9]: as lrge_hip_zstd_stats.
int zs_twin_inflate(const uint8_t *d, uint64_t n, uint64_t round_blocks, int checksum, uint64_t budget, uint64_t *stats, uint64_t *bad_off) {
    Twin t;
    if (budget) t.budget = budget;
    g_out.clear();
    ZsStats st;
    const int rc = zs_run(t, d, n, round_blocks, checksum != 0, [&](const uint8_t *b, uint64_t k) { g_out.insert(g_out.end(), b, b + k); return true; }, st, bad_off);
    if (stats) {
        const uint64_t v[9] = {st.frames, st.skippable, st.blocks, st.raw_blocks, st.rle_blocks, st.sequences, st.checksums_checked, st.rounds, st.bytes_out};
        memcpy(stats, v, sizeof v);
    }
    return rc;
}

// the same with the sliding backend: a work text [history | round] per round instead of the whole text.  slide_stats[4]: rounds,
// the largest history carried, the largest work text, the bytes of all histories (lrge_hip_reads_zstd_stats)
int zs_twin_inflate_sliding(const uint8_t *d, uint64_t n, uint64_t round_blocks, int checksum, uint64_t *stats, uint64_t *bad_off, uint64_t *slide_stats) {
    Twin t;
    t.sliding = true;
    g_out.clear();
    ZsStats st;
    ZsSlide sl;
    const int rc = zs_run(t, d, n, round_blocks, checksum != 0, [&](const uint8_t *b, uint64_t k) { g_out.insert(g_out.end(), b, b + k); return true; }, st, bad_off, &sl);
    if (stats) {
        const uint64_t v[9] = {st.frames, st.skippable, st.blocks, st.raw_blocks, st.rle_blocks, st.sequences, st.checksums_checked, st.rounds, st.bytes_out};
        memcpy(stats, v, sizeof v);
    }
    if (slide_stats) { const uint64_t v[4] = {sl.rounds, sl.max_history, sl.max_work, sl.moved}; memcpy(slide_stats, v, sizeof v); }
    return rc;
}

// XXH64 of p[0, n) taken in parts at the ascending cuts cut[0, k) (each <= n) through zs_xxh64_part: a part takes its whole
// stripes, the next starts where the state stands, the last finishes
uint64_t zs_twin_xxh64_parts(const uint8_t *p, uint64_t n, const uint64_t *cut, uint64_t k) {
    Env env;
    ZsXxh S = {};
    for (uint64_t i = 0; i < k; ++i) {
        const uint64_t from = i ? S.hashed : 0;
        (void)zs_xxh64_part(env, S, p + from, cut[i] - from, i == 0, false);
    }
    const uint64_t from = k ? S.hashed : 0;
    return zs_xxh64_part(env, S, p + from, n - from, k == 0, true);
}

uint64_t zs_twin_result(uint8_t *dst) { if (dst && !g_out.empty()) memcpy(dst, g_out.data(), g_out.size()); return g_out.size(); }

// the repeat offsets behind n sequences (ofv, ll) from `in`: by the transfer function (composed over pieces of `piece` sequences)
// into by_fn, by the plain walk into by_walk.  Bit 0 of the result: the function refused; bit 1: the walk met an offset of 0
int zs_twin_rep(const uint32_t *ofv, const uint32_t *ll, uint64_t n, uint64_t piece, const uint32_t *in, uint32_t *by_fn, uint32_t *by_walk) {
    int out = 0;
    uint32_t cur[3] = {in[0], in[1], in[2]};
    for (uint64_t i = 0; i < n && !(out & 1);) {
        ZsRepEl f[3];
        zs_rep_identity(f);
        const uint64_t e = piece ? (i + piece < n ? i + piece : n) : n;
        for (; i < e; ++i) if (!zs_rep_step(f, ofv[i], ll[i])) { out |= 1; break; }
        uint32_t next[3];
        if (!(out & 1) && !zs_rep_apply(f, cur, next)) out |= 1;
        if (!(out & 1)) memcpy(cur, next, sizeof cur);
    }
    memcpy(by_fn, cur, sizeof cur);
    uint32_t r[3] = {in[0], in[1], in[2]};
    for (uint64_t i = 0; i < n; ++i) if (!zs_rep_resolve(r, ofv[i], ll[i])) { out |= 2; break; }
    memcpy(by_walk, r, sizeof r);
    return out;
}

}  // extern "C"
