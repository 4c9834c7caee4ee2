// name_lsd_round.h -- host side of the identifier ranking by fixed LSD passes: the gather of the selected
// identifiers into one padded blob with its checks, the limits and verdicts, and the pass loop.  One template drives both the
// device (host_names.inl: kernels of k_names.h, radix_sort_pairs, scan_exclusive_u32) and the host twin (names_lsd_twin.cpp: the
// same steps as loops over name_lsd.h), so the CPU suite tests this logic as the library runs it.
//
// The control flow does not depend on the data: the number and the shape of all steps follow from n and Lmax alone, both known
// on the host before the first step; nothing comes back before finish().
#pragma once
#include <stdint.h>
#include <string.h>

#include <utility>
#include <vector>

#include "name_lsd.h"

// the verdicts (the values of LRGE_OK, LRGE_ERR_TOO_MANY, _DEVICE, _INVALID, _UNPROVEN in include/lrge_hip.h)
enum { NL_OK = 0, NL_E_TOO_MANY = -3, NL_E_DEVICE = -5, NL_E_INVALID = -9, NL_E_UNPROVEN = -10 };

// the selected identifiers back to back: entry e is bytes [off[e], off[e] + len[e]) of `words`
struct NlBlob {
    std::vector<uint64_t> words;        // 8-byte aligned, at least NL_PAD zero bytes behind `bytes`
    uint64_t bytes = 0;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    uint32_t lmax = 0;
    uint64_t padded() const { return words.size() * 8; }
};
struct NlStats { uint64_t sorts, words, distinct; };

// Checks the call and gathers identifiers idx[0..n) (NULL: all n_names of them, in order) of names / name_off[n_names + 1], one
// memcpy each.  NL_E_TOO_MANY: n >= 2^32.  n == 0 is NL_OK whatever idx is.  NL_E_INVALID: idx == NULL with n != n_names, an
// entry out of range, offsets that are not monotone or leave the names, an identifier of 2^32 bytes or more.  NL_E_UNPROVEN:
// an identifier longer than max_bytes.  *why: a constant string for the message.
static inline int nl_gather(const char *names, const uint64_t *name_off, uint64_t n_names, const uint32_t *idx, uint64_t n, uint64_t max_bytes, NlBlob &B,
                            const char **why) {
    B = NlBlob();
    *why = "";
    if (n >> 32) { *why = "2^32 entries or more"; return NL_E_TOO_MANY; }
    if (n == 0) return NL_OK;                                     // an empty selection, whatever idx is
    if (!idx && n != n_names) { *why = "no index list: n must equal n_names"; return NL_E_INVALID; }
    if (!name_off || n_names == 0) { *why = "no identifiers"; return NL_E_INVALID; }
    const uint64_t end = name_off[n_names];
    if (end && !names) { *why = "no identifier bytes"; return NL_E_INVALID; }
    B.off.resize((size_t)n); B.len.resize((size_t)n);
    uint64_t total = 0;
    for (uint64_t e = 0; e < n; ++e) {
        const uint64_t i = idx ? idx[e] : e;
        if (i >= n_names) { *why = "an index out of range"; return NL_E_INVALID; }
        const uint64_t a = name_off[i], b = name_off[i + 1];
        if (a > b || b > end) { *why = "identifier offsets that are not monotone or leave the names"; return NL_E_INVALID; }
        if ((b - a) >> 32) { *why = "an identifier of 2^32 bytes or more"; return NL_E_INVALID; }
        B.off[(size_t)e] = total; B.len[(size_t)e] = (uint32_t)(b - a);
        if (B.len[(size_t)e] > B.lmax) B.lmax = B.len[(size_t)e];
        total += b - a;
    }
    if (B.lmax > max_bytes) { *why = "an identifier above NAME_RANK_MAX_BYTES: take the host sort"; return NL_E_UNPROVEN; }
    B.bytes = total;
    B.words.assign((size_t)(total / 8 + 3), 0);                   // 17..24 zero bytes behind the last identifier
    char *dst = (char *)B.words.data();
    for (uint64_t e = 0; e < n; ++e)
        if (B.len[(size_t)e]) memcpy(dst + B.off[(size_t)e], names + name_off[idx ? idx[e] : e], B.len[(size_t)e]);
    return NL_OK;
}

// D (the backend; every step returns NL_OK or a verdict):
//   int upload(const NlBlob &B, uint64_t n)      the blob, off and len; takes ALL the memory of the call, before any other step
//   uint64_t *key_buf(int s), *val_buf(int s)    the two (key, value) pairs the sort ping-pongs between, n entries each
//   int keys(uint32_t pass, uint32_t W, bool first, uint64_t *val, uint64_t *key)
//                                                key[p] = nl_pass_key of entry val[p]; first: entry p itself, and val[p] = p is written
//   int sort(uint64_t *k0, uint64_t *v0, uint64_t *k1, uint64_t *v1, uint64_t n, int nbits, uint64_t **rk, uint64_t **rv)
//                                                a stable sort by key bits [0, nbits), rounded up to whole bytes; the result lies in
//                                                (*rk, *rv), one of the two pairs
//   int heads(const uint64_t *val, uint32_t W)   head flag per sorted position
//   int ranks(const uint64_t *val)               exclusive scan of the flags, start[run], rank_out[val[p]] = start[run(p)]
//   int finish(uint32_t *rank_out, uint64_t *word)   the only read-back: the ranks and one word, distinct identifiers (low half) and
//                                                status bits (high half: NL_BAD_*), then the synchronisation
template <class D>
static int nl_run(D &dev, const NlBlob &B, uint64_t n, uint32_t *rank_out, NlStats &st, const char **why) {
    const uint32_t W = nl_words(B.lmax);
    st = NlStats{0, W, 0};
    *why = "";
    if (n >> 32) { *why = "2^32 entries or more"; return NL_E_TOO_MANY; }
    if (n == 0) return NL_OK;                                   // n == 0 and n == 1: no step runs
    if (!rank_out) { *why = "no rank_out"; return NL_E_INVALID; }
    if (n == 1) { rank_out[0] = 0; st.distinct = 1; return NL_OK; }
    int rc;
    if ((rc = dev.upload(B, n))) return rc;
    uint64_t *k = dev.key_buf(0), *v = dev.val_buf(0), *k2 = dev.key_buf(1), *v2 = dev.val_buf(1);
    for (uint32_t i = 0; i <= W; ++i) {
        const uint32_t pass = W - i;                            // W: the length pass, then the words W-1 .. 0
        if ((rc = dev.keys(pass, W, i == 0, v, k))) return rc;
        uint64_t *rk = nullptr, *rv = nullptr;
        if ((rc = dev.sort(k, v, k2, v2, n, pass == W ? (int)nl_len_bits(B.lmax) : 64, &rk, &rv))) return rc;
        ++st.sorts;
        // the sort ping-pongs: its result side depends on the pass count; the other pair is the next call's scratch side
        if (rk == k2 && rv == v2) { std::swap(k, k2); std::swap(v, v2); }
        else if (rk != k || rv != v) { *why = "the sort returned a pair that is neither of its two"; return NL_E_DEVICE; }
    }
    if ((rc = dev.heads(v, W))) return rc;
    if ((rc = dev.ranks(v))) return rc;
    uint64_t word = 0;
    if ((rc = dev.finish(rank_out, &word))) return rc;
    st.distinct = (uint32_t)word;
    if (word >> 32) { *why = "a sorted value or a run number out of range"; return NL_E_DEVICE; }
    return NL_OK;
}
