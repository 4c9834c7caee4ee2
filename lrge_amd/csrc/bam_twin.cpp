// bam_twin.cpp -- the host twin of the device BAM record scan (k_bam.h, host_bam.inl; g++): the library's own driver (bam_run,
// bam_round.h) over a backend that runs the same passes over the same core (bam_core.h) segment by segment on the CPU --
// header, candidate search, walks, the table -- and the nibble gather, with the segment size a parameter, so the CPU suite
// checks the algorithm, the repair rounds and their counts against the host parser with records straddling segment edges
// (tests/test_bam_twin.py).  TEST INFRASTRUCTURE, not part of the product library.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "bam_round.h"

namespace {
struct Parsed {
    std::vector<uint8_t> text;          // a copy with slack behind it, as the device buffer has (the gather's word loads)
    std::vector<FxRec> recs;
    BamStats st = {0, 0, 0, 0, 0, 0};
};
Parsed g;
const uint64_t PAD = 64;

// the backend of bam_run: every pass a loop over the segments
struct Twin {
    const uint8_t *t; uint64_t n, hdr_end, S;
    uint64_t end(uint64_t s) const { return bam_seg_end(hdr_end, S, n, s); }
    int header(uint64_t *he, uint32_t *verdict) { *verdict = bam_header(t, n, he); return 0; }
    int round0(uint64_t he, uint64_t seg_bytes, uint64_t n_seg, uint64_t *cand, BamSeg *seg) {
        hdr_end = he; S = seg_bytes;
        cand[0] = hdr_end;
        for (uint64_t s = 1; s < n_seg; ++s) {
            cand[s] = BAM_NONE;
            for (uint64_t off = bam_seg_begin(hdr_end, S, s); off < end(s); ++off)
                if (bam_plausible(t, n, off)) { cand[s] = off; break; }
        }
        for (uint64_t s = 0; s < n_seg; ++s) seg[s] = bam_walk(t, n, cand[s], end(s));
        return 0;
    }
    int rewalk(const uint32_t *list, const uint64_t *from, uint64_t k, BamSeg *got) {
        for (uint64_t i = 0; i < k; ++i) got[i] = bam_walk(t, n, from[i], end(list[i]));
        return 0;
    }
    int records(const uint64_t *start, const uint64_t *base, uint64_t n_seg, uint64_t n_rec, uint32_t *flags, uint64_t *name_bytes) {
        g.recs.resize(n_rec);
        std::vector<uint32_t> seq_len(n_rec), name_len(n_rec);
        for (uint64_t s = 0; s < n_seg; ++s) {
            if (start[s] == BAM_NONE) continue;
            uint64_t nb = 0;
            *flags |= bam_walk_records(t, n, start[s], end(s), base[s + 1] - base[s], g.recs.data() + base[s], seq_len.data() + base[s], name_len.data() + base[s], &nb);
            *name_bytes += nb;
        }
        return 0;
    }
};
}  // namespace

extern "C" {

// 0: proven (bam_twin_count records), FX_UNPROVEN, FX_TOO_MANY.  `S`: bytes per segment, at least 64.
int bam_twin_parse(const uint8_t *text, uint64_t n, uint64_t S) {
    g = Parsed();
    if (S < 64) return -1;
    g.text.assign(n + PAD, 0);
    if (n) memcpy(g.text.data(), text, n);
    Twin be = {g.text.data(), n, 0, 0};
    uint64_t n_rec = 0, name_bytes = 0;
    const char *refused = nullptr;
    const int rc = bam_run(be, n, S, &g.st, &n_rec, &name_bytes, &refused);
    if (rc) g.recs.clear();
    return rc > 0 && rc != (int)FX_TOO_MANY ? (int)BAM_UNPROVEN : rc;       // (any bits of the table step are unproven, as before)
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
