// bam_twin.cpp -- the host twin of the device BAM record scan (k_bam.h, host_bam.inl; g++): the library's own driver (bam_run,
// bam_round.h) over a backend that runs the same passes over the same core (bam_core.h) segment by segment on the CPU --
// header, candidate search, walks, the table -- and the nibble gather, with the segment size a parameter, so the CPU suite
// checks the algorithm, the repair rounds and their counts against the host parser with records straddling segment edges
// (tests/test_bam_twin.py); and the windowed ingest of fx_window.h over the same passes, with the window and the appended
// piece as parameters (tests/test_bam_window_twin.py).  TEST INFRASTRUCTURE, not part of the product library.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "bam_round.h"
#include "win_twin.h"

namespace bam_twin {             // (a name of its own: tools/window_twin_check.cpp holds the three twins in one translation unit)
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
    bool tail = false;
    uint64_t end(uint64_t s) const { return bam_seg_end(hdr_end, S, n, s); }
    int header(uint64_t *he, uint32_t *verdict) { *verdict = bam_header(t, n, he); return 0; }
    int round0(uint64_t he, uint64_t seg_bytes, uint64_t n_seg, bool tail_mode, uint64_t *cand, BamSeg *seg) {
        hdr_end = he; S = seg_bytes; tail = tail_mode;
        cand[0] = hdr_end;
        for (uint64_t s = 1; s < n_seg; ++s) {
            cand[s] = BAM_NONE;
            for (uint64_t off = bam_seg_begin(hdr_end, S, s); off < end(s); ++off)
                if (bam_plausible(t, n, off)) { cand[s] = off; break; }
        }
        for (uint64_t s = 0; s < n_seg; ++s) seg[s] = bam_walk(t, n, cand[s], end(s), tail);
        return 0;
    }
    int rewalk(const uint32_t *list, const uint64_t *from, uint64_t k, BamSeg *got) {
        for (uint64_t i = 0; i < k; ++i) got[i] = bam_walk(t, n, from[i], end(list[i]), tail);
        return 0;
    }
    int records(const uint64_t *start, const uint64_t *base, uint64_t n_seg, uint64_t n_rec, uint64_t cut, uint32_t *flags, uint64_t *name_bytes) {
        g.recs.resize(n_rec);
        std::vector<uint32_t> seq_len(n_rec), name_len(n_rec);
        for (uint64_t s = 0; s < n_seg; ++s) {
            if (start[s] == BAM_NONE) continue;
            uint64_t nb = 0;
            *flags |= bam_walk_records(t, n, start[s], std::min(end(s), cut), base[s + 1] - base[s], g.recs.data() + base[s], seq_len.data() + base[s], name_len.data() + base[s], &nb);
            *name_bytes += nb;
        }
        return 0;
    }
};

// bam_run over a copy of the text into `g`: 0, BAM_UNPROVEN (any bits of the table step included), FX_TOO_MANY
int run(const uint8_t *text, uint64_t n, uint64_t S, bool first = true, uint64_t *cut = nullptr) {
    g = Parsed();
    g.text.assign(n + PAD, 0);
    if (n) memcpy(g.text.data(), text, n);
    Twin be = {g.text.data(), n, 0, 0};
    uint64_t n_rec = 0, name_bytes = 0;
    const char *refused = nullptr;
    const int rc = bam_run(be, n, S, &g.st, &n_rec, &name_bytes, &refused, first, cut);
    return rc > 0 && rc != (int)FX_TOO_MANY ? (int)BAM_UNPROVEN : rc;
}

// ---- the windowed ingest: win_twin.h over the passes above ----
// (the store holds the packed bytes of every record, as k_bam_store leaves them, with PAD of slack behind; seq_span = (seq_len + 1) / 2)
WinTwinOut gw;
BamStats gw_bam = {0, 0, 0, 0, 0, 0};   // summed over the windows
uint64_t gw_scans = 0, gw_store_bytes = 0;       // record scans run, with or without a cut; the store without its slack

struct Scan {
    uint64_t S;
    int scan(const std::vector<uint8_t> &blk, bool first, bool end, uint64_t *cut, int *fmt) {
        uint64_t c = 0;
        ++gw_scans;
        const int rc = run(blk.data(), blk.size(), S, first, end ? nullptr : &c);
        if (rc) return rc;
        *cut = end ? blk.size() : c;
        *fmt = FX_FMT_BAM;
        if (!*cut) return 0;
        uint64_t *sum = &gw_bam.segments;
        const uint64_t *add = &g.st.segments;
        for (int i = 0; i < 6; ++i) sum[i] += add[i];
        return 0;
    }
    const std::vector<FxRec> &recs() const { return g.recs; }
    void append(const std::vector<uint8_t> &, uint64_t, const FxRec &r, std::vector<uint8_t> &store) const {
        store.insert(store.end(), g.text.data() + r.seq_off, g.text.data() + r.seq_off + r.seq_span);
    }
};

// the gather of bam_twin_seq over text s
uint64_t gather(const uint8_t *s, uint64_t len, uint32_t misalign, uint8_t *out) {
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
}  // namespace

extern "C" {

// 0: proven (bam_twin_count records), FX_UNPROVEN, FX_TOO_MANY.  `S`: bytes per segment, at least 64.
int bam_twin_parse(const uint8_t *text, uint64_t n, uint64_t S) {
    g = Parsed();
    if (S < 64) return -1;
    const int rc = run(text, n, S);
    if (rc) g.recs.clear();
    return rc;
}

uint64_t bam_twin_count(void) { return g.recs.size(); }
void bam_twin_table(FxRec *out) { if (!g.recs.empty()) memcpy(out, g.recs.data(), g.recs.size() * sizeof(FxRec)); }
void bam_twin_stats(BamStats *out) { *out = g.st; }

// the bases of record i into out[0, seq_len), as the device gather forms them for a destination that is `misalign` bytes
// behind a word boundary: single bases up to the boundary, groups of eight through bam_group8, single bases behind the last
// whole group; returns how many bytes were written
uint64_t bam_twin_seq(uint64_t i, uint32_t misalign, uint8_t *out) {
    const FxRec &r = g.recs[i];
    return gather(g.text.data() + r.seq_off, r.seq_len, misalign, out);
}

// The text through the windows of fx_window.h (win_twin_run).  0: proven, BAM_UNPROVEN, FX_TOO_MANY; the records by
// bam_twin_windowed_count / _table / _seq (the same gather, applied to the store), the store by _store, the counts by _stats
// (windows flushed first: 0 means the text ended before its first flush and was scanned whole, as without windows, with no store
// as on the device; out[4]: record scans run, kept across a refused run) and _bam_stats (summed over the windows).
int bam_twin_windowed(const uint8_t *text, uint64_t n, uint64_t S, uint64_t window, uint64_t piece) {
    gw = WinTwinOut(); gw_bam = BamStats{0, 0, 0, 0, 0, 0}; gw_scans = gw_store_bytes = 0;
    if (S < 64 || !piece) return -1;
    Scan sc = {S};
    const int rc = win_twin_run(sc, text, n, window, piece, false, gw);
    if (rc) { gw_bam = BamStats{0, 0, 0, 0, 0, 0}; return rc; }
    gw_store_bytes = gw.store.size();
    gw.store.resize(gw_store_bytes + PAD, 0);
    return 0;
}

uint64_t bam_twin_windowed_count(void) { return gw.recs.size(); }
void bam_twin_windowed_table(FxRec *out) { gw.table(out); }
void bam_twin_windowed_stats(uint64_t out[5]) { gw.stats(out); out[4] = gw_scans; }
void bam_twin_windowed_bam_stats(BamStats *out) { *out = gw_bam; }
uint64_t bam_twin_windowed_store(uint8_t *out) { return gw.store_to(out, gw_store_bytes); }
uint64_t bam_twin_windowed_seq(uint64_t i, uint32_t misalign, uint8_t *out) {
    const FxRec &r = gw.recs[i];
    return gather(gw.store.data() + r.seq_off, r.seq_len, misalign, out);
}

}  // extern "C"
}  // namespace bam_twin
