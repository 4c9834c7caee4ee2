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
#include "fx_window.h"

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

// ---- the windowed ingest: fx_window.h over the passes above ----
struct WinOut {
    std::vector<FxRec> recs;            // name_off: in the whole text; seq_off: in `store`; seq_span = (seq_len + 1) / 2
    std::vector<uint8_t> store;         // the packed bytes of every record, dense, as k_bam_store leaves them (PAD of slack behind)
    FxWinStats st = {0, 0, 0, 0};
    BamStats bam = {0, 0, 0, 0, 0, 0};
    uint64_t scans = 0;                 // record scans run, with or without a cut
    uint64_t store_bytes = 0;
};
WinOut gw;

struct WinTwin {
    std::vector<uint8_t> blk;
    uint64_t S, base = 0;               // base: where the block starts in the whole text
    uint64_t len() const { return blk.size(); }
    int resident_format(bool *yes) const { *yes = false; return 0; }
    void resident_again() const {}
    int unproven(const char *) const { return (int)BAM_UNPROVEN; }
    int flush(bool first, bool end, uint64_t *cut, int *fmt) {
        const uint64_t n = blk.size();
        g = Parsed();
        g.text.assign(n + PAD, 0);
        if (n) memcpy(g.text.data(), blk.data(), n);
        Twin be = {g.text.data(), n, 0, 0};
        uint64_t n_rec = 0, name_bytes = 0, c = 0;
        const char *refused = nullptr;
        ++gw.scans;
        const int rc = bam_run(be, n, S, &g.st, &n_rec, &name_bytes, &refused, first, end ? nullptr : &c);
        if (rc) return rc > 0 && rc != (int)FX_TOO_MANY ? (int)BAM_UNPROVEN : rc;
        *cut = end ? n : c;
        *fmt = FX_FMT_BAM;
        if (!*cut) return 0;
        uint64_t *sum = &gw.bam.segments;
        const uint64_t *add = &g.st.segments;
        for (int i = 0; i < 6; ++i) sum[i] += add[i];
        for (uint64_t i = 0; i < n_rec; ++i) {
            const FxRec &r = g.recs[i];
            gw.recs.push_back(FxRec{base + r.name_off, gw.store.size(), r.seq_span, r.name_len, r.seq_len});
            gw.store.insert(gw.store.end(), g.text.data() + r.seq_off, g.text.data() + r.seq_off + r.seq_span);
        }
        return 0;
    }
    int carry(uint64_t cut) {
        blk.erase(blk.begin(), blk.begin() + (long)cut);
        base += cut;
        return 0;
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
    return gather(g.text.data() + r.seq_off, r.seq_len, misalign, out);
}

// The text through the windows of fx_window.h: `piece` bytes appended per step, a flush once the block holds `window` bytes.
// 0: proven, BAM_UNPROVEN, FX_TOO_MANY; the records by bam_twin_windowed_count / _table / _seq (the same gather, applied to the
// store), the store by _store, the counts by _stats (windows flushed first: 0 means the text ended before its first flush and
// was scanned whole, as without windows; out[4]: record scans run) and _bam_stats (summed over the windows).
int bam_twin_windowed(const uint8_t *text, uint64_t n, uint64_t S, uint64_t window, uint64_t piece) {
    gw = WinOut();
    if (S < 64 || !piece) return -1;
    WinTwin b;
    b.S = S;
    FxWindow<WinTwin> win(b, window);
    int rc = 0;
    for (uint64_t p = 0; p < n && !rc; p += piece) {
        b.blk.insert(b.blk.end(), text + p, text + (n - p < piece ? n : p + piece));
        rc = win.step(false);
    }
    uint64_t all = 0;
    if (!rc) rc = win.st.windows ? win.step(true) : b.flush(true, true, &all, &win.fmt);         // (or the resident scan)
    const uint64_t scans = gw.scans;
    if (rc) { gw = WinOut(); gw.scans = scans; return rc; }
    gw.store_bytes = gw.store.size();
    gw.st = win.st; gw.st.bases = win.st.windows ? gw.store_bytes : 0;      // (resident: no store, as on the device)
    gw.store.resize(gw.store_bytes + PAD, 0);
    return 0;
}

uint64_t bam_twin_windowed_count(void) { return gw.recs.size(); }
void bam_twin_windowed_table(FxRec *out) { if (!gw.recs.empty()) memcpy(out, gw.recs.data(), gw.recs.size() * sizeof(FxRec)); }
void bam_twin_windowed_stats(uint64_t out[5]) { out[0] = gw.st.windows; out[1] = gw.st.bases; out[2] = gw.st.max_window; out[3] = gw.st.carried; out[4] = gw.scans; }
void bam_twin_windowed_bam_stats(BamStats *out) { *out = gw.bam; }
uint64_t bam_twin_windowed_store(uint8_t *out) { if (out && gw.store_bytes) memcpy(out, gw.store.data(), gw.store_bytes); return gw.store_bytes; }
uint64_t bam_twin_windowed_seq(uint64_t i, uint32_t misalign, uint8_t *out) {
    const FxRec &r = gw.recs[i];
    return gather(gw.store.data() + r.seq_off, r.seq_len, misalign, out);
}

}  // extern "C"
