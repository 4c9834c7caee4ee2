// bam_core.h -- the record scan of uncompressed unaligned BAM, shared by the device (k_bam.h, host_bam.inl; hipcc) and the host
// twin (bam_twin.cpp; g++): the per-record rule, the header walk, the candidate predicate of the speculative starts, the
// nibble decode of the gather.  The host-side logic between the rounds is bam_round.h.  The result must equal
// lrge::io::detail::parse_bam (include/lrge_io.hpp) record for record; whatever these rules cannot prove is the verdict
// BAM_UNPROVEN, and the caller takes the host parser.
//
// BAM records form a length-prefixed chain: where record i + 1 starts is known only from the block size of record i.  The
// records area [hdr_end, n) is cut into segments of S bytes; a record belongs to the segment its first byte lies in.  Every
// segment is walked from a start of its own -- segment 0 from hdr_end, the others from a candidate (bam_plausible) -- and
// bam_chain_plan (bam_round.h) ties the walks together: a start counts only once it is the landing of the segment in front of it.
#pragma once
#include <stdint.h>

#include "fastx_core.h"

#define FX_FMT_BAM 3
#define BAM_UNPROVEN FX_UNPROVEN
#define BAM_NONE (~(uint64_t)0)            // no candidate in a segment; the landing of a walk that met a record it refuses
// A window of the windowed ingest (fx_window.h) ends somewhere inside a record.  There the walks run in tail
// mode: a record start that is only *incomplete* -- fewer than 4 bytes are left, or a block size of 32 or more reaches past the
// end -- ends the walk with the landing BAM_TAIL | start.  Everything else bam_record refuses stays refused (a block size below
// 32 is judged as soon as its four bytes are there).  Offsets are below 2^63, and BAM_NONE is never taken for a tail landing.
#define BAM_TAIL ((uint64_t)1 << 63)
#define BAM_SHORT 4u                       // beside BAM_UNPROVEN in a header's verdict: it failed only for lack of bytes

// one segment: where its walk started (BAM_NONE: no walk), the records that start in it, and the first record start at or
// behind its end that the walk reached (n at the exact end of the text)
struct BamSeg { uint64_t start, count, landing; };

struct BamStats { uint64_t segments, empty_segments, speculative_starts, rejected_starts, repair_rounds, rewalked_segments; };
// the counts of a run of windows: every field sums (a new field is added here as well)
inline void bam_stats_add(BamStats &sum, const BamStats &w) {
    sum.segments += w.segments; sum.empty_segments += w.empty_segments; sum.speculative_starts += w.speculative_starts;
    sum.rejected_starts += w.rejected_starts; sum.repair_rounds += w.repair_rounds; sum.rewalked_segments += w.rewalked_segments;
}

// multi-byte fields lie at any byte offset: assembled from bytes
FX_HD uint32_t bam_u16(const uint8_t *t, uint64_t o) { return (uint32_t)t[o] | (uint32_t)t[o + 1] << 8; }
FX_HD uint32_t bam_u32(const uint8_t *t, uint64_t o) { return bam_u16(t, o) | bam_u16(t, o + 2) << 16; }

// The record at `off`, by the host's rule: 0 with *rec filled and *next the offset behind it, or BAM_UNPROVEN (which covers a
// mapped record: the host answers that one with its own message).  Reads no byte at or past n.
FX_HD uint32_t bam_record(const uint8_t *t, uint64_t n, uint64_t off, FxRec *rec, uint64_t *next) {
    if (off > n || n - off < 4) return BAM_UNPROVEN;
    const int32_t block = (int32_t)bam_u32(t, off);
    if (block < 32 || n - off - 4 < (uint64_t)block) return BAM_UNPROVEN;
    const uint32_t l_read_name = t[off + 12], n_cigar = bam_u16(t, off + 16), flag = bam_u16(t, off + 18);
    const int32_t l_seq = (int32_t)bam_u32(t, off + 20);
    if (l_seq < 0) return BAM_UNPROVEN;
    const uint64_t span = ((uint64_t)l_seq + 1) / 2;
    if (32 + (uint64_t)l_read_name + 4 * (uint64_t)n_cigar + span > (uint64_t)block) return BAM_UNPROVEN;
    if (!(flag & 4)) return BAM_UNPROVEN;
    rec->name_off = off + 36;
    rec->name_len = l_read_name ? l_read_name - 1 : 0;                       // the bytes as they are: no cut at whitespace, NULs kept
    if (rec->name_len == 1 && t[off + 36] == '*') rec->name_len = 0;
    rec->seq_off = off + 36 + l_read_name + 4 * (uint64_t)n_cigar;
    rec->seq_len = (uint32_t)l_seq;
    rec->seq_span = span;
    *next = off + 4 + (uint64_t)block;
    return 0;
}

// the record start at `off` <= n is incomplete: more bytes may still make it a record (or show that it is none)
FX_HD bool bam_incomplete(const uint8_t *t, uint64_t n, uint64_t off) {
    if (n - off < 4) return true;
    const int32_t block = (int32_t)bam_u32(t, off);
    return block >= 32 && n - off - 4 < (uint64_t)block;
}

// the header: magic, l_text, text, n_ref, then l_name, name, l_ref of every reference, with the host's bounds (a negative n_ref
// is no reference, as there).  0 with *hdr_end the offset of the first record, or BAM_UNPROVEN; BAM_UNPROVEN | BAM_SHORT when
// every field that is there passes and the text ends inside the header (a window's caller waits for more; any other has
// BAM_UNPROVEN in it and needs no second look).
FX_HD uint32_t bam_header(const uint8_t *t, uint64_t n, uint64_t *hdr_end) {
    const uint8_t magic[4] = {'B', 'A', 'M', 1};
    for (uint64_t i = 0; i < 4 && i < n; ++i)
        if (t[i] != magic[i]) return BAM_UNPROVEN;
    if (n < 8) return BAM_UNPROVEN | BAM_SHORT;
    const int32_t l_text = (int32_t)bam_u32(t, 4);
    uint64_t off = 8;
    if (l_text < 0) return BAM_UNPROVEN;
    if (n - off < (uint64_t)l_text) return BAM_UNPROVEN | BAM_SHORT;
    off += (uint64_t)l_text;
    if (n - off < 4) return BAM_UNPROVEN | BAM_SHORT;
    const int32_t n_ref = (int32_t)bam_u32(t, off);
    off += 4;
    for (int32_t r = 0; r < n_ref; ++r) {
        if (n - off < 4) return BAM_UNPROVEN | BAM_SHORT;
        const int32_t l_name = (int32_t)bam_u32(t, off);
        off += 4;
        if (l_name < 0) return BAM_UNPROVEN;
        if (n - off < (uint64_t)l_name + 4) return BAM_UNPROVEN | BAM_SHORT;
        off += (uint64_t)l_name + 4;
    }
    *hdr_end = off;
    return 0;
}

// A candidate for a speculative start: a record by bam_record that carries what every writer of unaligned BAM puts into the
// four position fields (refID, pos, next_refID, next_pos = -1), followed by another such record or by the end of the text.
// Correctness never rests on this: a candidate counts only once the chain from the header has reached it.  In a window n is
// the block's end, taken as the end of the text: a candidate whose own record or whose successor the block cuts off is rejected.
FX_HD bool bam_candidate_one(const uint8_t *t, uint64_t n, uint64_t off, uint64_t *next) {
    FxRec r;
    if (bam_record(t, n, off, &r, next)) return false;
    return (bam_u32(t, off + 4) & bam_u32(t, off + 8) & bam_u32(t, off + 24) & bam_u32(t, off + 28)) == 0xFFFFFFFFu;
}
FX_HD bool bam_plausible(const uint8_t *t, uint64_t n, uint64_t off) {
    uint64_t next, after;
    if (!bam_candidate_one(t, n, off, &next)) return false;
    return next == n || bam_candidate_one(t, n, next, &after);
}

FX_HD uint64_t bam_seg_begin(uint64_t hdr_end, uint64_t S, uint64_t s) { return hdr_end + s * S; }
FX_HD uint64_t bam_seg_end(uint64_t hdr_end, uint64_t S, uint64_t n, uint64_t s) { return n - hdr_end - s * S <= S ? n : hdr_end + (s + 1) * S; }

// the walk of one segment from `start` (>= the segment's begin): follows the chain until it reaches the segment's end.
// tail: an incomplete record start ends the walk with a tail landing instead of none
FX_HD BamSeg bam_walk(const uint8_t *t, uint64_t n, uint64_t start, uint64_t end, bool tail = false) {
    BamSeg g = {start, 0, BAM_NONE};
    if (start == BAM_NONE) return g;
    uint64_t off = start;
    while (off < end) {
        FxRec r;
        uint64_t next;
        if (bam_record(t, n, off, &r, &next)) {
            if (tail && bam_incomplete(t, n, off)) g.landing = BAM_TAIL | off;
            return g;
        }
        ++g.count;
        off = next;
    }
    g.landing = off;
    return g;
}
// the same walk from a proven start, writing the table: `cap` records at recs / seq_len / name_len (the count of the proving
// walk).  Verdict bits; *name_bytes: the identifier bytes of the records written.
FX_HD uint32_t bam_walk_records(const uint8_t *t, uint64_t n, uint64_t start, uint64_t end, uint64_t cap, FxRec *recs, uint32_t *seq_len, uint32_t *name_len,
                                uint64_t *name_bytes) {
    uint64_t off = start, k = 0, nb = 0;
    uint32_t f = 0;
    while (off < end && k < cap) {
        FxRec r;
        uint64_t next;
        if ((f = bam_record(t, n, off, &r, &next))) break;
        recs[k] = r; seq_len[k] = r.seq_len; name_len[k] = r.name_len;
        nb += r.name_len;
        ++k;
        off = next;
    }
    *name_bytes = nb;
    return f | (k != cap || off < end ? BAM_UNPROVEN : 0);
}

// ---- the gather: 4-bit codes to ASCII ----
// code c is byte c & 7 of BAM_NT_LO (c < 8) or of BAM_NT_HI: "=ACMGRSV" and "TWYHKDBN" as little-endian words
#define BAM_NT_LO 0x565352474D43413DULL
#define BAM_NT_HI 0x4E42444B48595754ULL
FX_HD uint32_t bam_nt(uint32_t c) { return (uint32_t)(((c & 8) ? BAM_NT_HI : BAM_NT_LO) >> ((c & 7) * 8)) & 0xFF; }
// base i of the packed sequence at s: the high nibble comes first
FX_HD uint32_t bam_base(const uint8_t *s, uint64_t i) { return bam_nt((uint32_t)(s[i >> 1] >> ((~i & 1) << 2)) & 15); }
// eight bases from the 64-bit window v whose byte 0 holds the first of them, in its high nibble (odd = 0) or its low one
// (odd = 1: five bytes are used): the ASCII of bases 0-3 into out[0], 4-7 into out[1], little-endian
FX_HD void bam_decode8(uint64_t v, uint32_t odd, uint32_t out[2]) {
    out[0] = out[1] = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t m = 0; m < 8; ++m) {
        const uint32_t j = m + odd;
        const uint32_t c = (uint32_t)(v >> (8 * (j >> 1) + ((j & 1) ? 0 : 4))) & 15;
        out[m >> 2] |= bam_nt(c) << ((m & 3) * 8);
    }
}
// the window at byte address a: the aligned word a lies in and the one behind it, shifted so that a is byte 0 (five bytes are
// valid at any alignment, which is what an odd start needs; the word behind may lie in the slack behind the text)
FX_HD uint64_t bam_window(const uint8_t *a) {
    const uintptr_t p = (uintptr_t)a;
    uint32_t q[2];
#if defined(__HIPCC__)
    q[0] = ((const uint32_t *)(p & ~(uintptr_t)3))[0]; q[1] = ((const uint32_t *)(p & ~(uintptr_t)3))[1];
#else
    __builtin_memcpy(q, (const void *)(p & ~(uintptr_t)3), 8);
#endif
    return (((uint64_t)q[1] << 32) | q[0]) >> ((uint32_t)(p & 3) * 8);
}
// bases [i0, i0 + 8) of the packed sequence at s as two words of ASCII
FX_HD void bam_group8(const uint8_t *s, uint64_t i0, uint32_t out[2]) { bam_decode8(bam_window(s + (i0 >> 1)), (uint32_t)(i0 & 1), out); }
