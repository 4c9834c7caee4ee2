// bam_twin.cpp -- the host twin of the device BAM record scan (k_bam.h, host_bam.inl; g++): the library's own driver (bam_run,
// bam_round.h) over a backend that runs the same passes over the same core (bam_core.h) segment by segment on the CPU --
// header, candidate search, walks, the table -- and the nibble gather, with the segment size a parameter, so the CPU suite
// checks the algorithm, the repair rounds and their counts against the host parser with records straddling segment edges
// (tests/test_bam_twin.py); and the windowed ingest of fx_window.h over the same passes, with the window and the appended
// piece as parameters (tests/test_bam_window_twin.py); and the sampled ingest of DESIGN section 25 over the same windows -- the
// census, the selection, the seek map and the mapped pass (tests/test_bam_select_twin.py, tests/test_bam_seek_twin.py).
// TEST INFRASTRUCTURE, not part of the product library.
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
    bool header = true;                 // false: the sub-text of a mapped run, whole records of a proven text -- no window of it has a header
    int scan(const std::vector<uint8_t> &blk, bool first, bool end, uint64_t *cut, int *fmt) {
        uint64_t c = 0;
        ++gw_scans;
        const int rc = run(blk.data(), blk.size(), S, first && header, end ? nullptr : &c);
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

FxSeekMap gm;                           // the map of the last bam_twin_census_map
FxSeekPlan gp;                          // the plan of the last bam_twin_seek_plan / bam_twin_mapped

// one run through the windows in a keep mode: the globals reset, the store given its slack
int windowed_run(const uint8_t *text, uint64_t n, uint64_t S, uint64_t window, uint64_t piece, bool header, FxKeepMode mode, const uint32_t *sel, uint64_t k, FxSeekMap *map) {
    gw = WinTwinOut(); gw_bam = BamStats{0, 0, 0, 0, 0, 0}; gw_scans = gw_store_bytes = 0;
    if (S < 64 || !piece) return -1;
    Scan sc = {S, header};
    const int rc = win_twin_run(sc, text, n, window, piece, false, gw, mode, sel, k, map, FX_LEAD_BAM);
    if (rc) { gw_bam = BamStats{0, 0, 0, 0, 0, 0}; return rc; }
    gw_store_bytes = gw.store.size();
    gw.store.resize(gw_store_bytes + PAD, 0);
    return 0;
}

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
    return windowed_run(text, n, S, window, piece, true, FX_KEEP_ALL, nullptr, 0, nullptr);
}

// The same text in the two passes of the sampled ingest, as fastx_twin_census / _selected.  bam_twin_census keeps
// nothing: out = {records, sequence bases, text bytes, windows flushed}.  bam_twin_selected keeps records sel[0, k) (strictly
// ascending ordinals): the accessors above read its result as they read bam_twin_windowed's (the store holds the chosen records'
// packed bytes), bam_twin_windowed_select_stats what the run saw and kept, in bases.  0, BAM_UNPROVEN, FX_TOO_MANY, or
// WIN_TWIN_INVALID for a selection that is not ascending or reaches past the records
int bam_twin_census(const uint8_t *text, uint64_t n, uint64_t S, uint64_t window, uint64_t piece, uint64_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    const int rc = windowed_run(text, n, S, window, piece, true, FX_KEEP_NONE, nullptr, 0, nullptr);
    if (!rc) { out[0] = gw.sel.seen; out[1] = gw.sel.bases_seen; out[2] = n; out[3] = gw.st.windows; }
    return rc;
}

int bam_twin_selected(const uint8_t *text, uint64_t n, uint64_t S, uint64_t window, uint64_t piece, const uint32_t *sel, uint64_t k) {
    return windowed_run(text, n, S, window, piece, true, FX_KEEP_SEL, sel, k, nullptr);
}

// The seek map and the mapped second pass (fx_seek.h), as fastx_twin_census_map / _seek_plan / _mapped: a record starts at its
// block_size field (fx_rec_start with FX_LEAD_BAM), so the first point is record 0 at hdr_end; the planner is fx_seek_plan
int bam_twin_census_map(const uint8_t *text, uint64_t n, uint64_t S, uint64_t window, uint64_t piece, uint64_t stride, uint64_t out[4]) {
    gm = FxSeekMap();
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!stride) return -1;
    FxSeekMap m;
    m.stride = stride;
    const int rc = windowed_run(text, n, S, window, piece, true, FX_KEEP_NONE, nullptr, 0, &m);
    if (rc) return rc;
    out[0] = gw.sel.seen; out[1] = gw.sel.bases_seen; out[2] = n; out[3] = gw.st.windows;
    m.records = gw.sel.seen; m.bases = gw.sel.bases_seen; m.text_bytes = m.file_len = n; m.windows = gw.st.windows; m.fmt = gw.fmt;
    gm = m;
    return 0;
}

uint64_t bam_twin_map_points(uint64_t *ord, uint64_t *off, uint64_t cap) {
    for (uint64_t i = 0; i < gm.pts.size() && i < cap; ++i) { ord[i] = gm.pts[i].ord; off[i] = gm.pts[i].off; }
    return gm.pts.size();
}

int bam_twin_seek_plan(const uint32_t *c_len, const uint32_t *isize, uint64_t n_blk, uint64_t file_len, const uint32_t *sel, uint64_t k, uint64_t out[4]) {
    return win_twin_seek_plan(gm, c_len, isize, n_blk, file_len, sel, k, &gp, out);
}
uint64_t bam_twin_plan_runs(uint64_t *out, uint64_t cap) { return win_twin_plan_runs(gp, out, cap); }
void bam_twin_plan_sel(uint32_t *out) { if (!gp.sel.empty()) memcpy(out, gp.sel.data(), gp.sel.size() * 4); }

// The mapped second pass over text `text`, which must be the text of the last map (WIN_TWIN_INVALID: another size): the runs of the
// plan, concatenated, are a record stream without a header, scanned from its first window on as later windows are.  BAM_UNPROVEN
// also when the sub-text does not hold the plan's records.  bam_twin_windowed_bam_stats: summed over the windows of the sub-text
int bam_twin_mapped(const uint8_t *text, uint64_t n, uint64_t S, uint64_t window, uint64_t piece, const uint32_t *sel, uint64_t k) {
    gw = WinTwinOut(); gp = FxSeekPlan(); gw_store_bytes = 0;
    if (S < 64 || !piece) return -1;
    if (n != gm.text_bytes || gm.kind != FX_SEEK_PLAIN || win_twin_sel_fits(gm, sel, k)) return WIN_TWIN_INVALID;
    fx_seek_plan(gm, sel, k, &gp);
    const std::vector<uint8_t> sub = win_twin_sub_text(gp, text);
    int rc = windowed_run(sub.data(), sub.size(), S, window, piece, false, FX_KEEP_SEL, gp.sel.data(), k, nullptr);
    if (rc == WIN_TWIN_INVALID || (!rc && gw.sel.seen != gp.records)) rc = (int)BAM_UNPROVEN;       // the map does not fit the input
    if (rc) { gw = WinTwinOut(); gw_bam = BamStats{0, 0, 0, 0, 0, 0}; gw_store_bytes = 0; return rc; }
    win_twin_mapped_back(gw, gp, gm);
    if (gw.fmt == FX_FMT_EMPTY) gw.fmt = gm.fmt;
    return 0;
}

void bam_twin_windowed_select_stats(uint64_t out[4]) { gw.select_stats(out); }
// the records of every window of the last run, in order (at most `cap` are written); returns how many windows took records or a cut
uint64_t bam_twin_windowed_cuts(uint64_t *out, uint64_t cap) { return gw.cuts(out, cap); }

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
