// sam_core.h -- the record scan of unaligned SAM text, shared by the device (k_sam.h, host_sam.inl; hipcc) and the host twin
// (sam_twin.cpp; g++): the sniff, the per-line predicate, the tab mask of a 16-byte group and the per-record rule.  The result
// must equal lrge::io::detail::parse_sam (include/lrge_io.hpp) record for record; whatever these rules cannot prove is the
// verdict FX_UNPROVEN, and the caller takes the host parser.
//
// Lines are those of fx_line (fastx_core.h): cut at line feeds, one trailing CR stripped.  An empty line and a line whose first
// byte is '@' are skipped wherever they stand; every other line is a record line and needs ten tabs.  A record line is read in
// steps of SAM_STEP bytes -- 64 lanes, one aligned 16-byte group each -- up to its tenth tab and no further.
#pragma once
#include <stdint.h>

#include "fastx_core.h"

#define FX_FMT_SAM 4
#define SAM_STEP 1024u         // text bytes per step of a record line: 64 lanes x one 16-byte load
#define SAM_N_TABS 4u          // the tabs the rule needs: ranks 1, 2, 9 and 10 of the line

// the host's sniff (lrge_io.hpp: sniff): "@HD", "@SQ" or "@RG" at offset 0; h: the first three bytes of a text of n bytes
FX_HD bool sam_sniff(const uint8_t *h, uint64_t n) {
    return n >= 3 && h[0] == '@' && ((h[1] == 'H' && h[2] == 'D') || (h[1] == 'S' && h[2] == 'Q') || (h[1] == 'R' && h[2] == 'G'));
}

// the rank (1-based, counted from the start of the line) of the tab that slot s of a SamTabs holds
FX_HD uint32_t sam_tab_rank(uint32_t s) { return s == 0 ? 1u : s == 1 ? 2u : s == 2 ? 9u : 10u; }

// line [a, e) carries a record
FX_HD bool sam_is_record_line(const uint8_t *t, uint64_t a, uint64_t e) { return e > a && t[a] != '@'; }

// the tabs of one little-endian word, bit i for byte i.  x has a zero byte where w has a tab; (x & 0x7F..) + 0x7F.. carries into
// bit 7 of every byte with a low bit set and never across bytes, so z has 0x80 exactly in the zero bytes; the multiplication
// moves bits 0, 8, 16, 24 of z >> 7 to bits 28..31 (sixteen distinct partial products: no carries)
FX_HD uint32_t sam_word_tabs(uint32_t w) {
    const uint32_t x = w ^ 0x09090909u;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
    return ((z >> 7) * 0x10204080u) >> 28;
}

// the tabs of the group of 16 bytes at p (a multiple of 16; p < e) that lie inside the line [a, e): bit i is byte p + i
FX_HD uint32_t sam_tab_mask(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint64_t p, uint64_t a, uint64_t e) {
    uint32_t m = sam_word_tabs(w0) | sam_word_tabs(w1) << 4 | sam_word_tabs(w2) << 8 | sam_word_tabs(w3) << 12;
    if (p < a) m &= ~((1u << (uint32_t)(a - p)) - 1);
    if (e - p < 16) m &= (1u << (uint32_t)(e - p)) - 1;
    return m;
}

// the index of set bit number r (0-based from the low end) of m, which has more than r bits set
FX_HD uint32_t sam_nth_bit(uint32_t m, uint32_t r) {
    for (; r; --r) m &= m - 1;
    return (uint32_t)__builtin_ctz(m);
}

// The record of the line that starts at a, with its tabs 1, 2, 9 and 10 at t1, t2, t9 and t10: name [a, t1), flag (t1, t2),
// sequence (t9, t10).  The flag is 1 to 9 ASCII digits and nothing else, with bit 2 set: strtoul on the host also takes blanks,
// signs, an embedded NUL and values up to 2^64, none of which is restated here.  A name or sequence that is the single byte
// '*' is empty.  Verdict bits; *rec is complete only when they are 0.
FX_HD uint32_t sam_record(const uint8_t *t, uint64_t a, uint64_t t1, uint64_t t2, uint64_t t9, uint64_t t10, FxRec *rec) {
    const uint64_t fl = t2 - t1 - 1;
    if (fl < 1 || fl > 9) return FX_UNPROVEN;
    uint32_t flag = 0;
    for (uint64_t i = t1 + 1; i < t2; ++i) {
        const uint32_t c = t[i];
        if (c < '0' || c > '9') return FX_UNPROVEN;
        flag = flag * 10 + (c - '0');
    }
    if (!(flag & 4)) return FX_UNPROVEN;                            // a mapped record: the host has the message for it
    uint64_t nl = t1 - a, sl = t10 - t9 - 1;
    if (nl == 1 && t[a] == '*') nl = 0;
    if (sl == 1 && t[t9 + 1] == '*') sl = 0;
    rec->name_off = a; rec->seq_off = t9 + 1; rec->seq_span = sl;  // (seq_span == seq_len: the gather copies words)
    if (nl >> 32) return FX_UNPROVEN;
    if (sl >> 32) return FX_TOO_MANY;
    rec->name_len = (uint32_t)nl; rec->seq_len = (uint32_t)sl;
    return 0;
}
