// bam_twin.cpp -- the host twin of the device BAM record scan (k_bam.h, host_bam.inl; g++): the same passes over the same core
// (bam_core.h) run segment by segment on the CPU -- header, candidate search, walks, the repair rounds of bam_chain_plan, the
// table, the nibble gather -- with the segment size a parameter, so the CPU suite checks the algorithm and its counts against
// the host parser with records straddling segment edges (tests/test_bam_twin.py).  TEST INFRASTRUCTURE, not part of the
// product library.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "bam_core.h"

namespace {
struct Parsed {
    std::vector<uint8_t> text;          // a copy with slack behind it, as the device buffer has (the gather's word loads)
    std::vector<FxRec> recs;
    BamStats st = {0, 0, 0, 0, 0, 0};
};
Parsed g;
const uint64_t PAD = 64;
}  // namespace

extern "C" {

// 0: proven (bam_twin_count records), FX_UNPROVEN, FX_TOO_MANY.  `S`: bytes per segment, at least 64.
int bam_twin_parse(const uint8_t *text, uint64_t n, uint64_t S) {
    g = Parsed();
    if (S < 64) return -1;
    g.text.assign(n + PAD, 0);
    if (n) memcpy(g.text.data(), text, n);
    const uint8_t *t = g.text.data();
    uint64_t hdr_end = 0;
    if (bam_header(t, n, &hdr_end)) return (int)BAM_UNPROVEN;
    if (hdr_end == n) return 0;
    const uint64_t n_seg = (n - hdr_end + S - 1) / S;
    if (n_seg >> 31) return (int)BAM_UNPROVEN;
    // the finder: the first plausible offset of every segment behind the first
    std::vector<uint64_t> cand(n_seg, BAM_NONE), from(n_seg + 1);
    for (uint64_t s = 1; s < n_seg; ++s) {
        const uint64_t end = bam_seg_end(hdr_end, S, n, s);
        for (uint64_t off = bam_seg_begin(hdr_end, S, s); off < end; ++off)
            if (bam_plausible(t, n, off)) { cand[s] = off; break; }
    }
    // round 0, then the repair rounds
    std::vector<BamSeg> seg(n_seg);
    std::vector<uint32_t> list(n_seg);
    for (uint64_t s = 0; s < n_seg; ++s) seg[s] = bam_walk(t, n, s ? cand[s] : hdr_end, bam_seg_end(hdr_end, S, n, s));
    for (;;) {
        uint32_t verdict = 0;
        const uint64_t k = bam_chain_plan(seg.data(), n_seg, hdr_end, S, n, list.data(), from.data(), &verdict);
        if (verdict) return (int)verdict;
        if (!k) break;
        ++g.st.repair_rounds; g.st.rewalked_segments += k;
        for (uint64_t i = 0; i < k; ++i) seg[list[i]] = bam_walk(t, n, from[i], bam_seg_end(hdr_end, S, n, list[i]));
    }
    bam_chain_stats(seg.data(), cand.data(), n_seg, &g.st);
    // the table
    uint64_t n_rec = 0;
    for (uint64_t s = 0; s < n_seg; ++s) { from[s] = n_rec; n_rec += seg[s].count; }
    from[n_seg] = n_rec;
    if (n_rec >> 32) return (int)FX_TOO_MANY;
    g.recs.resize(n_rec);
    std::vector<uint32_t> seq_len(n_rec), name_len(n_rec);
    uint32_t flags = 0;
    for (uint64_t s = 0; s < n_seg; ++s) {
        if (seg[s].start == BAM_NONE) continue;
        uint64_t nb = 0;
        flags |= bam_walk_records(t, n, seg[s].start, bam_seg_end(hdr_end, S, n, s), from[s + 1] - from[s], g.recs.data() + from[s], seq_len.data() + from[s],
                                  name_len.data() + from[s], &nb);
    }
    if (flags) { g.recs.clear(); return (int)BAM_UNPROVEN; }
    return 0;
}

uint64_t bam_twin_count(void) { return g.recs.size(); }
void bam_twin_table(FxRec *out) { if (!g.recs.empty()) memcpy(out, g.recs.data(), g.recs.size() * sizeof(FxRec)); }
void bam_twin_stats(BamStats *out) { *out = g.st; }

// the bases of record i into out[0, seq_len), as the device gather forms them for a destination that is `misalign` bytes
// behind a word boundary: single bases up to the boundary, groups of eight through bam_group8, single bases behind the last
// whole group; returns how many bytes were written
uint64_t bam_twin_seq(uint64_t i, uint32_t misalign, uint8_t *out) {
    const FxRec &r = g.recs[i];
    const uint8_t *s = g.text.data() + r.seq_off;
    const uint64_t len = r.seq_len;
    const uint64_t head = std::min<uint64_t>((4 - (misalign & 3)) & 3, len);
    uint64_t w = 0;
    for (; w < head; ++w) out[w] = (uint8_t)bam_base(s, w);
    for (uint64_t k = 0; k < (len - head) >> 3; ++k, w += 8) {
        uint32_t q[2];
        bam_group8(s, head + 8 * k, q);
        memcpy(out + w, q, 8);
    }
    for (; w < len; ++w) out[w] = (uint8_t)bam_base(s, w);
    return w;
}

}  // extern "C"
