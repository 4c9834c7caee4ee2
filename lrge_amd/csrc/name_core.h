// name_core.h -- the rules of the identifier ranking by radix refinement, written to compile for the device
// (hipcc) as well as for the host twin (names_twin.cpp; g++), which is their only user so far: how an identifier becomes symbols,
// how symbols and the current rank become a sort key, and what one entry of a sorted round does next.
// The result must equal engine.name_ranks / detail::name_ranks: rank = the number of selected entries whose identifier is strictly smaller, byte-wise on unsigned bytes, a proper prefix
// being smaller.
//
// An identifier is read as 9-bit symbols: byte + 1, and 0 at every position past its end.  So the end of an identifier sorts
// in front of every byte, 0x00 included, and bytes of 0x80 and above need no special case.  Round 0 sorts every entry by its
// first NR_FIRST_SYMS symbols; round k > 0 sorts the entries that are still tied by (current rank, the next NR_NEXT_SYMS
// symbols).  An entry leaves when its key is unique in the round, or when the LAST symbol of its key is 0: then every entry
// that shares the key has ended too, so their identifiers are equal (tied entries).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NR_HD __host__ __device__ __forceinline__
#else
#define NR_HD static inline
#endif

#define NR_SYM_BITS 9u
#define NR_FIRST_SYMS 7u       // 63 key bits in round 0
#define NR_NEXT_SYMS 3u        // 27 key bits below the rank in the later rounds
#define NR_RANK_SHIFT (NR_NEXT_SYMS * NR_SYM_BITS)
#define NR_SYM_MASK ((1u << NR_SYM_BITS) - 1)

// what nr_verdict returns
#define NR_GOES_ON 0u
#define NR_ALONE 1u            // the key is unique: the rank is final
#define NR_TIED 2u             // the key is shared and ends with symbol 0: equal identifiers, the rank is final

NR_HD uint32_t nr_round_syms(uint32_t round) { return round ? NR_NEXT_SYMS : NR_FIRST_SYMS; }
// the byte at which round `round` starts reading
NR_HD uint32_t nr_round_depth(uint32_t round) { return round ? NR_FIRST_SYMS + (round - 1) * NR_NEXT_SYMS : 0; }
// the rounds an identifier of `len` bytes can stay tied for: its len + 1 symbols (the end included) must have been read
NR_HD uint32_t nr_max_rounds(uint32_t len) { return len + 1 <= NR_FIRST_SYMS ? 1 : 1 + (len + 1 - NR_FIRST_SYMS + NR_NEXT_SYMS - 1) / NR_NEXT_SYMS; }
// the key bits a round sorts by, n entries in the call
NR_HD uint32_t nr_key_bits(uint32_t round, uint64_t n) {
    if (!round) return NR_FIRST_SYMS * NR_SYM_BITS;
    uint32_t b = 0;
    while (b < 32 && (1ULL << b) < n) ++b;
    return NR_RANK_SHIFT + b;
}

// `cnt` <= 8 text bytes from byte address a (relative to the 8-byte aligned base w8) as a little-endian word: aligned 8-byte
// loads and a funnel shift; only words that hold one of the bytes are loaded, the bytes above cnt are undefined
NR_HD uint64_t nr_load_bytes(const uint64_t *w8, uint64_t a, uint32_t cnt) {
    const uint32_t sh = (uint32_t)(a & 7) * 8;
    const uint64_t lo = w8[a >> 3];
    if (!sh) return lo;
    const uint64_t hi = (uint32_t)(a & 7) + cnt > 8 ? w8[(a >> 3) + 1] : 0;
    return (lo >> sh) | (hi << (64 - sh));
}

// the first nsym symbols of the `cnt` bytes in `bytes` (first byte lowest), most significant symbol first
NR_HD uint64_t nr_pack_syms(uint64_t bytes, uint32_t cnt, uint32_t nsym) {
    uint64_t k = 0;
    for (uint32_t i = 0; i < nsym; ++i) {
        const uint64_t s = i < cnt ? ((bytes >> (8 * i)) & 0xFF) + 1 : 0;
        k = (k << NR_SYM_BITS) | s;
    }
    return k;
}

// the sort key of an entry in round `round`: identifier text[off, off + len), current rank `rank` (0 in round 0).  n_text:
// the bytes of the text; an identifier that does not lie inside it is cut there, so no load leaves the text's last word
NR_HD uint64_t nr_key(const uint64_t *w8, uint64_t n_text, uint64_t off, uint32_t len, uint32_t round, uint32_t rank) {
    if (off > n_text) { off = n_text; len = 0; }
    if ((uint64_t)len > n_text - off) len = (uint32_t)(n_text - off);
    const uint32_t d = nr_round_depth(round), nsym = nr_round_syms(round);
    uint32_t cnt = len > d ? len - d : 0;
    if (cnt > nsym) cnt = nsym;
    const uint64_t syms = cnt ? nr_pack_syms(nr_load_bytes(w8, off + d, cnt), cnt, nsym) : 0;
    return round ? ((uint64_t)rank << NR_RANK_SHIFT) | syms : syms;
}

// entry p of a sorted round, from its key and its neighbours': bit 0: p starts a sub-group (a run of equal keys), bit 1: p
// starts a group (a run of equal ranks; round 0 has one group)
NR_HD uint32_t nr_heads(uint64_t key, uint64_t prev_key, bool first, uint32_t round) {
    if (first) return 3u;
    return (uint32_t)(key != prev_key) | ((uint32_t)(round && (key >> NR_RANK_SHIFT) != (prev_key >> NR_RANK_SHIFT)) << 1);
}
// starts: p starts a sub-group; next_starts: p + 1 does, or p is the last entry
NR_HD uint32_t nr_verdict(uint64_t key, bool starts, bool next_starts) {
    if (starts && next_starts) return NR_ALONE;
    return (key & NR_SYM_MASK) == 0 ? NR_TIED : NR_GOES_ON;
}
// the new rank: sub_head / group_head are the sorted positions at which the entry's sub-group and group start
NR_HD uint32_t nr_new_rank(uint64_t key, uint32_t round, uint32_t sub_head, uint32_t group_head) {
    return (round ? (uint32_t)(key >> NR_RANK_SHIFT) : 0u) + (sub_head - group_head);
}
