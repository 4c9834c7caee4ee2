// names_lsd_twin.cpp -- the identifier ranking by fixed LSD passes as loops on the CPU (g++): the backend of
// name_lsd_round.h that runs the steps of the device backend (host_names.inl, k_names.h) over the rules of name_lsd.h, with
// std::stable_sort on the u64 key as the sort, so the CPU suite checks the key, equality and rank rules, the gather, the limits
// and the pass loop -- the result side of a ping-pong sort included -- against engine.name_ranks (tests/test_names_lsd_twin.py,
// tools/name_lsd_check.cpp).  TEST INFRASTRUCTURE, not part of the product library.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <numeric>
#include <utility>
#include <vector>

#include "name_lsd_round.h"

namespace {
struct NlTwin {
    const NlBlob *B = nullptr;
    uint64_t n = 0;
    std::vector<uint64_t> kb[2], vb[2];
    std::vector<uint32_t> flag, excl, start, rank;
    uint32_t distinct = 0, status = 0;

    int upload(const NlBlob &b, uint64_t n_) {
        B = &b; n = n_;
        for (int s = 0; s < 2; ++s) { kb[s].assign((size_t)n, ~0ULL); vb[s].assign((size_t)n, ~0ULL); }
        flag.assign((size_t)n, 0); excl.assign((size_t)n, 0); start.assign((size_t)n, ~0u); rank.assign((size_t)n, ~0u);
        return NL_OK;
    }
    uint64_t *key_buf(int s) { return kb[s].data(); }
    uint64_t *val_buf(int s) { return vb[s].data(); }
    // as the kernels: an entry that does not lie inside the blob is cut there
    void entry(uint64_t e, uint64_t &o, uint32_t &l) const {
        o = B->off[(size_t)e]; l = B->len[(size_t)e];
        if (o > B->bytes) { o = B->bytes; l = 0; }
        if ((uint64_t)l > B->bytes - o) l = (uint32_t)(B->bytes - o);
    }
    int keys(uint32_t pass, uint32_t W, bool first, uint64_t *val, uint64_t *key) {
        for (uint64_t p = 0; p < n; ++p) {
            const uint64_t e = first ? p : val[p];
            if (e >= n) { status |= NL_BAD_VAL; key[p] = 0; continue; }
            if (first) val[p] = p;
            uint64_t o; uint32_t l;
            entry(e, o, l);
            key[p] = nl_pass_key(B->words.data(), o, l, pass, W);
        }
        return NL_OK;
    }
    // the call shape of radix_sort_pairs: one pass per key byte, each from one pair into the other, so the result lies in
    // (k0, v0) after an even number of passes and in (k1, v1) after an odd one; the side it does not lie in is overwritten
    int sort(uint64_t *k0, uint64_t *v0, uint64_t *k1, uint64_t *v1, uint64_t n_, int nbits, uint64_t **rk, uint64_t **rv) {
        *rk = k0; *rv = v0;
        if (n_ <= 1 || nbits <= 0) return NL_OK;
        const int passes = (nbits + 7) / 8;
        const uint64_t mask = passes >= 8 ? ~0ULL : (1ULL << (8 * passes)) - 1;
        std::vector<std::pair<uint64_t, uint64_t>> a((size_t)n_);
        for (uint64_t p = 0; p < n_; ++p) a[(size_t)p] = {k0[p], v0[p]};
        std::stable_sort(a.begin(), a.end(), [mask](const std::pair<uint64_t, uint64_t> &x, const std::pair<uint64_t, uint64_t> &y) { return (x.first & mask) < (y.first & mask); });
        uint64_t *dk = passes & 1 ? k1 : k0, *dv = passes & 1 ? v1 : v0, *ok = passes & 1 ? k0 : k1, *ov = passes & 1 ? v0 : v1;
        for (uint64_t p = 0; p < n_; ++p) { dk[p] = a[(size_t)p].first; dv[p] = a[(size_t)p].second; ok[p] = ~0ULL; ov[p] = ~0ULL; }
        *rk = dk; *rv = dv;
        return NL_OK;
    }
    int heads(const uint64_t *val, uint32_t W) {
        for (uint64_t p = 0; p < n; ++p) {
            if (p == 0) { flag[0] = 1; continue; }
            const uint64_t a = val[p - 1], b = val[p];
            if (a >= n || b >= n) { status |= NL_BAD_VAL; flag[(size_t)p] = 1; continue; }
            uint64_t oa, ob; uint32_t la, lb;
            entry(a, oa, la); entry(b, ob, lb);
            flag[(size_t)p] = nl_equal(B->words.data(), oa, la, ob, lb, W) ? 0u : 1u;
        }
        return NL_OK;
    }
    int ranks(const uint64_t *val) {
        uint32_t run = 0;
        for (uint64_t p = 0; p < n; ++p) { excl[(size_t)p] = run; run += flag[(size_t)p]; }
        distinct = run;
        for (uint64_t p = 0; p < n; ++p) {
            if (!flag[(size_t)p]) continue;
            if (excl[(size_t)p] >= n) { status |= NL_BAD_RUN; continue; }
            start[excl[(size_t)p]] = (uint32_t)p;
        }
        for (uint64_t p = 0; p < n; ++p) {
            const uint32_t r = nl_run_of(excl[(size_t)p], flag[(size_t)p]);
            const uint64_t e = val[p];
            if (r >= n) { status |= NL_BAD_RUN; continue; }
            if (e >= n) { status |= NL_BAD_VAL; continue; }
            rank[(size_t)e] = start[r];
        }
        return NL_OK;
    }
    int finish(uint32_t *rank_out, uint64_t *word) {
        memcpy(rank_out, rank.data(), (size_t)n * 4);
        *word = (uint64_t)status << 32 | distinct;
        return NL_OK;
    }
};
}  // namespace

extern "C" {

// names[name_off[i], name_off[i + 1]): identifier i of n_names; idx[0..n): the selected identifiers (any order, repeats allowed;
// NULL: all of them, n = n_names), rank_out[n]; stats (may be NULL): {sorts run, W, distinct identifiers, microseconds};
// max_bytes: the cap on the longest identifier (0: NL_MAX_BYTES_DEFAULT).  The verdicts of lrge_hip_name_ranks: 0, -3, -9, -10.
int names_lsd_twin_ranks(const char *names, const uint64_t *name_off, uint64_t n_names, const uint32_t *idx, uint64_t n, uint32_t *rank_out, uint64_t stats[4],
                         uint64_t max_bytes) {
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    NlBlob B;
    const char *why = "";
    int rc = nl_gather(names, name_off, n_names, idx, n, max_bytes ? max_bytes : NL_MAX_BYTES_DEFAULT, B, &why);
    if (rc) return rc;
    NlTwin dev;
    NlStats st;
    rc = nl_run(dev, B, n, rank_out, st, &why);
    if (stats) {
        stats[0] = st.sorts; stats[1] = st.words; stats[2] = st.distinct;
        stats[3] = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    }
    return rc;
}

// the key of word w of the identifier name[0, len) placed at byte `shift` (0..7) of an aligned buffer (tests of nl_word_key)
uint64_t names_lsd_word_key(const char *name, uint32_t len, uint32_t shift, uint32_t w) {
    std::vector<uint64_t> buf((size_t)(((uint64_t)shift + len) / 8 + 3), 0);
    if (len) memcpy((char *)buf.data() + shift, name, len);
    return nl_word_key(buf.data(), shift, len, w);
}

// The host sort the callers run today, for tools/names_bench.py: the std::sort form of detail::name_ranks (include/lrge_hip.hpp)
// over the same arguments.  0, -3, -9.
int names_lsd_host_sort_ranks(const char *names, const uint64_t *name_off, uint64_t n_names, const uint32_t *idx, uint64_t n, uint32_t *rank_out) {
    if (n >> 32) return -3;
    if (!idx && n != n_names) return -9;
    struct Ent { const char *p; uint32_t len; uint32_t e; };
    std::vector<Ent> all((size_t)n);
    for (uint64_t e = 0; e < n; ++e) {
        const uint64_t i = idx ? idx[e] : e;
        if (i >= n_names) return -9;
        all[(size_t)e] = Ent{names + name_off[i], (uint32_t)(name_off[i + 1] - name_off[i]), (uint32_t)e};
    }
    const auto cmp = [](const Ent &a, const Ent &b) -> int {
        const uint32_t m = a.len < b.len ? a.len : b.len;
        const int c = m ? memcmp(a.p, b.p, m) : 0;
        return c ? c : (a.len < b.len ? -1 : a.len > b.len ? 1 : 0);
    };
    std::sort(all.begin(), all.end(), [&](const Ent &a, const Ent &b) { return cmp(a, b) < 0; });
    uint32_t r = 0;
    for (uint64_t j = 0; j < n; ++j) {
        if (j && cmp(all[(size_t)j], all[(size_t)j - 1]) != 0) r = (uint32_t)j;
        rank_out[all[(size_t)j].e] = r;
    }
    return 0;
}

}  // extern "C"
