// name_lsd.h -- the rules of the identifier ranking by a fixed number of LSD sort passes, written to compile
// for the device (hipcc: k_names.h) as well as for the host twin (names_lsd_twin.cpp; g++): how an identifier becomes 64-bit
// word keys and a length key, when two neighbours of the sorted order are equal, and how head flags become competition ranks.
// The result must equal engine.name_ranks / detail::name_ranks: rank = the number of selected entries whose identifier is
// strictly smaller, byte-wise on unsigned bytes, a proper prefix being smaller.
//
// The selected identifiers lie back to back in one blob (8-byte aligned, NL_PAD zero bytes behind its end); entry e is
// blob[off[e], off[e] + len[e]).  W = ceil(Lmax / 8).  The key of word w is bytes [8w, 8w + 8) of the identifier, 0 for every
// byte at or past len, read as a big-endian u64; the length key is len.  One stable sort by the length key, then one stable
// 64-bit sort per word W-1 .. 0, leave the entries in byte-wise order with a proper prefix first: the zero padding ties `ab`
// with `ab\0`, and the length pass -- the least significant one -- has put `ab` in front.
#pragma once
#include <stdint.h>

#include "name_core.h"

#define NL_PAD 16u                 // zero bytes behind the blob at least
#define NL_MAX_BYTES_DEFAULT 256u  // option NAME_RANK_MAX_BYTES: the longest identifier the fixed-pass form takes

// status bits a kernel (or the twin's loop) raises when an invariant the host has checked does not hold after all
#define NL_BAD_VAL 1u              // a sorted value is no selection position
#define NL_BAD_RUN 2u              // a run number outside [0, n)

NR_HD uint32_t nl_words(uint32_t lmax) { return (lmax + 7u) / 8u; }
// the key bits of the length pass: the bits of Lmax (the sort rounds them up to whole bytes)
NR_HD uint32_t nl_len_bits(uint32_t lmax) { uint32_t b = 0; while (b < 32 && (lmax >> b)) ++b; return b; }

NR_HD uint64_t nl_bswap64(uint64_t v) {
    v = ((v & 0x00FF00FF00FF00FFULL) << 8) | ((v >> 8) & 0x00FF00FF00FF00FFULL);
    v = ((v & 0x0000FFFF0000FFFFULL) << 16) | ((v >> 16) & 0x0000FFFF0000FFFFULL);
    return (v << 32) | (v >> 32);
}

// the key of word w of identifier blob[off, off + len); w8: the blob as aligned words.  A word wholly past the end is 0
// without any load; otherwise only words that hold one of the identifier's bytes are loaded
NR_HD uint64_t nl_word_key(const uint64_t *w8, uint64_t off, uint32_t len, uint32_t w) {
    const uint64_t d = (uint64_t)w * 8;
    if (d >= len) return 0;
    const uint32_t left = len - (uint32_t)d, cnt = left < 8 ? left : 8;
    uint64_t b = nr_load_bytes(w8, off + d, cnt);          // little-endian: the first byte lowest
    if (cnt < 8) b &= (1ULL << (8 * cnt)) - 1;
    return nl_bswap64(b);
}

// pass W is the length pass, pass w < W the pass of word w
NR_HD uint64_t nl_pass_key(const uint64_t *w8, uint64_t off, uint32_t len, uint32_t pass, uint32_t W) {
    return pass >= W ? (uint64_t)len : nl_word_key(w8, off, len, pass);
}

// equal identifiers: the same length and the same W word keys, leaving at the first word that differs
NR_HD bool nl_equal(const uint64_t *w8, uint64_t off_a, uint32_t len_a, uint64_t off_b, uint32_t len_b, uint32_t W) {
    if (len_a != len_b) return false;
    for (uint32_t w = 0; w < W; ++w)
        if (nl_word_key(w8, off_a, len_a, w) != nl_word_key(w8, off_b, len_b, w)) return false;
    return true;
}

// Competition rank from the head flags (1: the sorted position starts a run of equal identifiers; position 0 always does) and
// their exclusive scan: a position lies in run `excl + flag - 1`, a head writes start[run] = position, and every position p
// writes rank_out[val[p]] = start[run(p)].
NR_HD uint32_t nl_run_of(uint32_t excl, uint32_t flag) { return excl + flag - 1u; }
