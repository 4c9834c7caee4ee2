// names_twin.cpp -- the identifier ranking by radix refinement as loops on the CPU (g++), in the passes a
// device form would run, over the core of name_core.h -- a key per active entry from aligned 8-byte words, a stable sort by the key
// bits in use, the head positions max-scanned tile by tile, then rank, verdict and compaction per sorted entry -- so the CPU
// suite checks the symbol, key and split rules against engine.name_ranks (tests/test_names_twin.py).
// TEST INFRASTRUCTURE, not part of the product library.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "name_core.h"

namespace {
const uint64_t TILE = 256;       // entries per tile of the head max-scan: one 256-lane workgroup

struct Rec { uint64_t off; uint32_t len; };
}  // namespace

extern "C" {

// blob[name_off[i], name_off[i + 1]): identifier i of n_names; idx[0..n): the selected identifiers (any order, repeats allowed; NULL: all of them, n = n_names), rank_out[n];
// stats: {rounds, sorted_entries, tied_entries}.  0, -9 (an entry out of range, idx == NULL with n neither 0 nor n_names), -3 (n >= 2^32),
// -100: a key with bits above nr_key_bits (a broken rule, never expected)
int names_twin_ranks(const uint8_t *blob, const uint64_t *name_off, uint64_t n_names, const uint32_t *idx, uint64_t n, uint32_t *rank_out, uint64_t stats[3]) {
    if (stats) stats[0] = stats[1] = stats[2] = 0;
    if (n >> 32) return -3;
    if (n == 0) return 0;
    if (!idx && n != n_names) return -9;
    if (!rank_out) return -9;
    const uint64_t n_text = name_off[n_names];
    std::vector<uint64_t> text(n_text / 8 + 2, 0);                  // the text in aligned words, with slack behind it as on the device
    if (n_text) memcpy(text.data(), blob, (size_t)n_text);
    std::vector<Rec> recs(n_names);
    for (uint64_t i = 0; i < n_names; ++i) recs[i] = Rec{name_off[i], (uint32_t)(name_off[i + 1] - name_off[i])};
    uint32_t max_len = 0;
    for (uint64_t j = 0; j < n; ++j) {
        const uint64_t i = idx ? idx[j] : j;
        if (i >= n_names) return -9;
        max_len = std::max(max_len, recs[i].len);
    }
    const uint32_t round_cap = nr_max_rounds(max_len);
    std::vector<std::pair<uint64_t, uint64_t>> act(n), next;     // (key, entry)
    std::vector<uint32_t> rank(n, 0), keep, dst, tsub, tgrp;
    for (uint64_t e = 0; e < n; ++e) {
        const Rec &rc = recs[idx ? idx[e] : e];
        act[e] = {nr_key(text.data(), n_text, rc.off, rc.len, 0, 0), e};
    }
    uint32_t round = 0;
    uint64_t sorted_total = 0, tied = 0;
    while (!act.empty()) {
        if (round >= round_cap) return -5;
        const uint64_t n_act = act.size();
        const uint32_t bits = nr_key_bits(round, n);
        for (const auto &kv : act) if (bits < 64 && (kv.first >> bits)) return -100;
        std::stable_sort(act.begin(), act.end(), [](const std::pair<uint64_t, uint64_t> &a, const std::pair<uint64_t, uint64_t> &b) { return a.first < b.first; });
        sorted_total += n_act;
        // per tile: the last sub-group head and the last group head (position + 1, 0: none), then their exclusive max-scan
        const uint64_t n_tiles = (n_act + TILE - 1) / TILE;
        tsub.assign(n_tiles, 0); tgrp.assign(n_tiles, 0);
        for (uint64_t p = 0; p < n_act; ++p) {
            const uint32_t h = nr_heads(act[p].first, p ? act[p - 1].first : 0, p == 0, round);
            if (h & 1) tsub[p / TILE] = (uint32_t)p + 1;
            if (h & 2) tgrp[p / TILE] = (uint32_t)p + 1;
        }
        uint32_t cs = 0, cg = 0;
        for (uint64_t t = 0; t < n_tiles; ++t) {
            const uint32_t s = tsub[t], g = tgrp[t];
            tsub[t] = cs; tgrp[t] = cg;
            cs = std::max(cs, s); cg = std::max(cg, g);
        }
        keep.assign(n_act, 0); dst.assign(n_act, 0);
        for (uint64_t t = 0; t < n_tiles; ++t) {
            uint32_t s = tsub[t], g = tgrp[t];
            for (uint64_t p = t * TILE; p < std::min(n_act, (t + 1) * TILE); ++p) {
                const uint64_t key = act[p].first;
                const uint32_t h = nr_heads(key, p ? act[p - 1].first : 0, p == 0, round);
                if (h & 1) s = (uint32_t)p + 1;
                if (h & 2) g = (uint32_t)p + 1;
                const bool next_starts = p + 1 >= n_act || act[p + 1].first != key;
                const uint32_t v = nr_verdict(key, (h & 1) != 0, next_starts);
                rank[act[p].second] = nr_new_rank(key, round, s - 1, g - 1);
                keep[p] = v == NR_GOES_ON;
                tied += v == NR_TIED;
            }
        }
        uint32_t total = 0;
        for (uint64_t p = 0; p < n_act; ++p) { dst[p] = total; total += keep[p]; }
        ++round;
        next.assign(total, {0, 0});
        for (uint64_t p = 0; p < n_act; ++p) {
            if (!keep[p]) continue;
            const uint64_t e = act[p].second;
            const Rec &rc = recs[idx ? idx[e] : e];
            next[dst[p]] = {nr_key(text.data(), n_text, rc.off, rc.len, round, rank[e]), e};
        }
        act.swap(next);
    }
    memcpy(rank_out, rank.data(), (size_t)n * 4);
    if (stats) { stats[0] = round; stats[1] = sorted_total; stats[2] = tied; }
    return 0;
}

uint32_t names_twin_max_rounds(uint32_t len) { return nr_max_rounds(len); }

}  // extern "C"
