// bam_round.h -- host side of the BAM record scan: the header's result, the segments, round 0, the repair rounds, the counts and
// the table step.  One template drives both the device (host_bam.inl: kernels of k_bam.h) and the host twin (bam_twin.cpp: the
// same steps run segment by segment on the CPU), so the CPU suite tests this logic as the library runs it.  The rules of a
// single record, walk and candidate are bam_core.h.
#pragma once
#include <stdint.h>

#include <vector>

#include "bam_core.h"

// One pass over the summaries, in segment order.  Segment s > 0 is consistent when a record of segment s - 1 reaches to its end
// or beyond (it is empty then, and inherits that landing: set here), or when its walk started at landing[s - 1].  Every other
// segment goes on the list to be walked again from landing[s - 1], unless the segment in front of it is on the list itself (its
// landing is about to change) or has no landing yet (a speculative walk that stopped at a record it refuses).  The first segment
// on the list always follows a proven prefix, so every round proves at least one more segment; an isolated false start is
// settled by the one round that walks its segment again, because the segment behind it started at the true landing.
// Returns the length of the list (list[i], from[i]); 0 means every start is proven by induction from segment 0.
// *verdict: BAM_UNPROVEN when a proven walk met a record bam_record refuses, or when the last walk does not end exactly at n.
//
// tail (a window that is not the last; the walks ran in tail mode): the chain may end at an incomplete record start instead.
// A tail landing of a *proven* segment ends the chain there: every segment behind it is out, whatever its walk found, and with
// an empty list the plan is done (*tail: the segments that count and the cut, n when the chain ends exactly there).  A tail
// landing of a segment that is not proven yet is a walk without a landing, exactly as BAM_NONE is: nothing is listed from it.
// The induction is unchanged -- the first listed segment still follows a proven prefix, so a round proves one more segment,
// or the pass meets a proven tail landing or the last segment and stops -- and so is its bound of n_seg rounds.
struct BamTail { uint64_t n_seg, cut; };
static inline uint64_t bam_chain_plan(BamSeg *seg, uint64_t n_seg, uint64_t hdr_end, uint64_t S, uint64_t n, uint32_t *list, uint64_t *from, uint32_t *verdict,
                                      BamTail *tail = nullptr) {
    *verdict = 0;
    uint64_t k = 0;
    bool proven = true, prev_listed = false;            // proven: every segment in front of s is consistent and not listed
    for (uint64_t s = 1; s < n_seg; ++s) {
        const uint64_t land = seg[s - 1].landing;
        if (prev_listed) { prev_listed = false; proven = false; continue; }
        if (land == BAM_NONE) {
            if (proven) { *verdict = BAM_UNPROVEN; return 0; }
            continue;
        }
        if (tail && (land & BAM_TAIL)) {
            if (proven) { tail->n_seg = s; tail->cut = land & ~BAM_TAIL; return 0; }
            continue;
        }
        if (land >= bam_seg_end(hdr_end, S, n, s)) { seg[s].start = BAM_NONE; seg[s].count = 0; seg[s].landing = land; continue; }
        if (seg[s].start == land) continue;
        list[k] = (uint32_t)s; from[k] = land; ++k;
        prev_listed = true; proven = false;
    }
    if (k == 0 && n_seg) {
        const uint64_t land = seg[n_seg - 1].landing;
        if (tail && land != BAM_NONE && (land & BAM_TAIL)) { tail->n_seg = n_seg; tail->cut = land & ~BAM_TAIL; }
        else if (land != n) *verdict = BAM_UNPROVEN;
        else if (tail) { tail->n_seg = n_seg; tail->cut = n; }
    }
    return k;
}

// the counts behind a proven chain (cand: what the finder gave each segment, BAM_NONE for none and for segment 0)
static inline void bam_chain_stats(const BamSeg *seg, const uint64_t *cand, uint64_t n_seg, BamStats *st) {
    st->segments = n_seg;
    for (uint64_t s = 1; s < n_seg; ++s) {
        st->empty_segments += seg[s].start == BAM_NONE;
        st->speculative_starts += cand[s] != BAM_NONE;
        st->rejected_starts += cand[s] != BAM_NONE && seg[s].start != cand[s];
    }
}

enum { BAM_RUN_DEVICE = -2 };

// B (the backend) holds the text of n bytes and does the passes over it.  Every step returns 0, or nonzero for a runtime failure
// (an int, so that the device's steps keep the library's checking macros): bam_run stops with BAM_RUN_DEVICE, the backend knows why.
// `tail` below is false for a text that is scanned whole.
//   int header(uint64_t *hdr_end, uint32_t *verdict)              bam_header
//   int round0(uint64_t hdr_end, uint64_t S, uint64_t n_seg, bool tail, uint64_t *cand, BamSeg *seg)
//                                                                  cand[s], 0 < s < n_seg: the first bam_plausible offset of
//                                                                  segment s, or BAM_NONE (cand[0]: anything); seg[s]: bam_walk
//                                                                  from there, seg[0] from hdr_end (all hold for the later steps)
//   int rewalk(const uint32_t *list, const uint64_t *from, uint64_t k, BamSeg *got)
//                                                                  got[i]: bam_walk of segment list[i] from from[i]
//   int records(const uint64_t *start, const uint64_t *base, uint64_t n_seg, uint64_t n_rec, uint64_t cut, uint32_t *flags, uint64_t *name_bytes)
//                                                                  the table of n_rec records: bam_walk_records of every segment
//                                                                  with a start (not BAM_NONE) up to its end or `cut`, whichever
//                                                                  comes first, base[s + 1] - base[s] records at base[s];
//                                                                  *flags: the verdict bits of all of them together
// S: bytes per segment, at least 64 (the callers' business: the device clamps, the twin refuses).
// Returns 0 (*n_rec records in the backend's table, *name_bytes of identifiers; no record at all behind a header that ends the
// text), BAM_RUN_DEVICE, or the verdict bits BAM_UNPROVEN / FX_TOO_MANY with *refused naming the step that gave them.
//
// The windows of fx_window.h.  first = false: the text starts on a record start, there is no header in it.
// cut != nullptr: the text is a window that is not the last -- the walks run in tail mode, and 0 comes with *cut the end of the
// proven run of complete records [0, *cut) that the table holds, or with *cut = 0 when there is none yet: the header is not
// whole, or the first record of a later window is not.  (A header that is whole is a cut of its own, so *cut = 0 is free to
// mean that.)  A block size that is truly bad but at least 32 looks incomplete first: block sizes are below 2^31, so the block
// holds such a record's claimed bytes before the window reaches the driver's 2^32 limit, and the record is judged then, unless
// the budget has refused the window before; either way the call ends unproven.
template <class B>
static int bam_run(B &be, uint64_t n, uint64_t S, BamStats *st, uint64_t *n_rec, uint64_t *name_bytes, const char **refused, bool first = true, uint64_t *cut = nullptr) {
    *st = BamStats{0, 0, 0, 0, 0, 0};
    *n_rec = *name_bytes = 0;
    *refused = nullptr;
    if (cut) *cut = 0;
    uint64_t hdr_end = 0;
    uint32_t verdict = 0;
    if (first && be.header(&hdr_end, &verdict)) return BAM_RUN_DEVICE;
    if (verdict) {
        if (cut && (verdict & BAM_SHORT)) return 0;                     // the block keeps growing
        *refused = "BAM header";
        return (int)BAM_UNPROVEN;
    }
    if (hdr_end == n) { if (cut) *cut = n; return 0; }                  // no record: an empty read set, as on the host
    const uint64_t n_seg = (n - hdr_end + S - 1) / S;
    if (n_seg >> 31) { *refused = "2^31 BAM segments or more"; return (int)BAM_UNPROVEN; }
    std::vector<uint64_t> cand(n_seg), from(n_seg + 1), start(n_seg);
    std::vector<BamSeg> seg(n_seg), got(n_seg);
    std::vector<uint32_t> list(n_seg);
    // round 0: every segment from its candidate
    if (be.round0(hdr_end, S, n_seg, cut != nullptr, cand.data(), seg.data())) return BAM_RUN_DEVICE;
    cand[0] = BAM_NONE;
    // repair rounds
    BamTail tail = {n_seg, n};
    for (;;) {
        const uint64_t k = bam_chain_plan(seg.data(), n_seg, hdr_end, S, n, list.data(), from.data(), &verdict, cut ? &tail : nullptr);
        if (verdict) { *refused = "the BAM record chain"; return (int)verdict; }
        if (!k) break;
        ++st->repair_rounds; st->rewalked_segments += k;
        if (be.rewalk(list.data(), from.data(), k, got.data())) return BAM_RUN_DEVICE;
        for (uint64_t i = 0; i < k; ++i) seg[list[i]] = got[i];
    }
    const uint64_t n_use = tail.n_seg;                                  // (a window: the segments up to the one the chain ends in)
    bam_chain_stats(seg.data(), cand.data(), n_use, st);
    // the table: every segment again from its proven start, at the exclusive scan of the counts
    uint64_t total = 0;
    for (uint64_t s = 0; s < n_use; ++s) { from[s] = total; total += seg[s].count; start[s] = seg[s].start; }
    from[n_use] = total;
    if (total >> 32) { *refused = "records"; return (int)FX_TOO_MANY; }
    if (cut) {
        *cut = tail.cut;
        if (!total) return 0;                                           // the header alone, or nothing yet
    }
    uint32_t flags = 0;
    if (be.records(start.data(), from.data(), n_use, total, tail.cut, &flags, name_bytes)) return BAM_RUN_DEVICE;
    if (flags) { *refused = "a BAM record changed between the walks"; return (int)flags; }
    *n_rec = total;
    return 0;
}
