// sam_twin.cpp -- the host twin of the device SAM record scan (k_sam.h, host_sam.inl; g++): the same passes over the same core
// (sam_core.h, fastx_core.h) as loops on the CPU -- line starts from 16-byte groups, a mark and a rank per line, then every
// record line in steps of SAM_STEP bytes, 64 "lanes" of one 16-byte group each, the tabs ranked by an inclusive scan of the
// lanes' popcounts -- so the CPU suite checks the stepping against the host parser (tests/test_sam_twin.py); and the windowed
// ingest of fx_window.h over the same passes, with the window and the appended piece as parameters
// (tests/test_sam_window_twin.py); and the sampled ingest of DESIGN section 27 over the same windows -- the census, the selection,
// the seek map and the mapped pass (tests/test_sam_select_twin.py, tests/test_sam_seek_twin.py).
// TEST INFRASTRUCTURE, not part of the product library.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "sam_core.h"
#include "win_twin.h"

namespace sam_twin {             // (a name of its own: tools/window_twin_check.cpp holds the three twins in one translation unit)
namespace {
std::vector<FxRec> g_recs;

// the words of the group at p (a multiple of 16), as a lane loads them: bytes past the text read as zero
void group_words(const uint8_t *t, uint64_t n, uint64_t p, uint32_t w[4]) {
    uint8_t b[16] = {0};
    memcpy(b, t + p, (size_t)(n - p < 16 ? n - p : 16));
    memcpy(w, b, 16);
}

// what one wavefront of k_sam_records does with the record line [a, e): verdict bits, *rec complete when they are 0
uint32_t record_line(const uint8_t *t, uint64_t n, uint64_t a, uint64_t e, FxRec *rec) {
    uint64_t tab[SAM_N_TABS] = {0, 0, 0, 0};
    uint32_t seen = 0;
    for (uint64_t p0 = a & ~(uint64_t)15; p0 < e && seen < 10; p0 += SAM_STEP) {
        uint32_t m[64], inc[64], any = 0, run = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint64_t p = p0 + (uint64_t)lane * 16;
            m[lane] = 0;
            if (p < e) {
                uint32_t w[4];
                group_words(t, n, p, w);
                m[lane] = sam_tab_mask(w[0], w[1], w[2], w[3], p, a, e);
            }
            any |= m[lane];
        }
        if (!any) continue;
        for (uint32_t lane = 0; lane < 64; ++lane) inc[lane] = run += (uint32_t)__builtin_popcount(m[lane]);
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t cnt = (uint32_t)__builtin_popcount(m[lane]), excl = seen + inc[lane] - cnt;
            for (uint32_t s = 0; s < SAM_N_TABS; ++s) {
                const uint32_t k = sam_tab_rank(s);
                if (excl < k && k <= excl + cnt) tab[s] = p0 + (uint64_t)lane * 16 + sam_nth_bit(m[lane], k - excl - 1);
            }
        }
        seen += inc[63];
    }
    return seen < 10 ? FX_UNPROVEN : sam_record(t, a, tab[0], tab[1], tab[2], tab[3], rec);
}

// the passes over t[0, n), which the caller has found to be SAM, into g_recs.  cut != nullptr: the text is a window that is not
// the last -- the prefix directly behind its last line feed (*cut; 0: it has none yet) is scanned as a complete text of that
// size, with the window's own line table
int parse(const uint8_t *t, uint64_t n, uint64_t *cut) {
    g_recs.clear();
    if (cut) *cut = 0;
    // the line starts, group by group as k_fx_census / k_fx_scatter find them
    std::vector<uint64_t> ls(1, 0);
    for (uint64_t p = 0; p < n; p += 16) {
        uint32_t w[4];
        group_words(t, n, p, w);
        const uint32_t nvalid = (uint32_t)(n - p < 16 ? n - p : 16);
        const uint32_t lf = fx_group_masks(w[0], w[1], w[2], w[3], p ? t[p - 1] : '\n', p + 16 < n ? t[p + 16] : FX_EOT, nvalid).lf;
        for (uint32_t b = lf; b; b &= b - 1) ls.push_back(p + (uint64_t)__builtin_ctz(b) + 1);
    }
    FxCensus c;
    memset(&c, 0, sizeof c);
    c.n_lf = ls.size() - 1;
    uint32_t verdict = fx_limits(FX_FMT_FASTQ, c);
    if (!verdict && (c.n_lf + 1) >> 32) verdict = FX_UNPROVEN;
    if (verdict) return (int)verdict;
    const uint64_t n_lines = c.n_lf + 1;
    if (cut) {
        if (!c.n_lf) return 0;
        *cut = n = ls[c.n_lf];
    }
    // marks, and their exclusive scan
    std::vector<uint32_t> mark(n_lines), rank(n_lines);
    uint32_t n_rec = 0;
    for (uint64_t j = 0; j < n_lines; ++j) {
        uint64_t a, e;
        fx_line(t, n, ls.data(), c.n_lf, j, &a, &e);
        mark[j] = (uint32_t)sam_is_record_line(t, a, e);
        rank[j] = n_rec; n_rec += mark[j];
    }
    g_recs.resize(n_rec);
    uint32_t flags = 0;
    uint64_t name_bytes = 0;
    for (uint64_t j = 0; j < n_lines; ++j) {
        if (!mark[j]) continue;
        uint64_t a, e;
        fx_line(t, n, ls.data(), c.n_lf, j, &a, &e);
        FxRec rec = {0, 0, 0, 0, 0};
        const uint32_t v = record_line(t, n, a, e, &rec);
        if (v) { rec.name_len = 0; rec.seq_len = 0; rec.seq_span = 0; }
        g_recs[rank[j]] = rec;
        flags |= v; name_bytes += rec.name_len;
    }
    if (!flags && name_bytes >> 32) flags = FX_UNPROVEN;
    if (flags) { g_recs.clear(); if (cut) *cut = 0; return flags & FX_UNPROVEN ? (int)FX_UNPROVEN : (int)FX_TOO_MANY; }
    return 0;
}

// ---- the windowed ingest: win_twin.h over the passes above ----
struct Scan {
    bool header = true;                 // false: the sub-text of a mapped run, whole lines of a proven text -- it starts with a record line and is never sniffed
    int scan(const std::vector<uint8_t> &blk, bool first, bool end, uint64_t *cut, int *fmt) {
        if (first && header && !sam_sniff(blk.data(), blk.size())) return (int)FX_UNPROVEN;     // (later windows are SAM by the run, not by their first bytes)
        uint64_t c = 0;
        const int rc = parse(blk.data(), blk.size(), end ? nullptr : &c);
        *cut = end ? blk.size() : c;
        *fmt = FX_FMT_SAM;
        return rc;
    }
    const std::vector<FxRec> &recs() const { return g_recs; }
    void append(const std::vector<uint8_t> &blk, uint64_t, const FxRec &r, std::vector<uint8_t> &store) const {
        store.insert(store.end(), blk.data() + r.seq_off, blk.data() + r.seq_off + r.seq_len);
    }
};
WinTwinOut gw;
FxSeekMap gm;                           // the map of the last sam_twin_census_map
FxSeekPlan gp;                          // the plan of the last sam_twin_seek_plan / sam_twin_mapped

// one run through the windows in a keep mode
int windowed_run(const uint8_t *t, uint64_t n, uint64_t window, uint64_t piece, bool header, FxKeepMode mode, const uint32_t *sel, uint64_t k, FxSeekMap *map) {
    gw = WinTwinOut();
    if (!piece) return -1;
    Scan sc;
    sc.header = header;
    return win_twin_run(sc, t, n, window, piece, false, gw, mode, sel, k, map, FX_LEAD_SAM);
}
}  // namespace

extern "C" {

// 0: proven (sam_twin_count records), FX_UNPROVEN (text without the SAM magic included), FX_TOO_MANY
int sam_twin_parse(const uint8_t *t, uint64_t n) {
    g_recs.clear();
    if (!sam_sniff(t, n)) return FX_UNPROVEN;
    return parse(t, n, nullptr);
}

// The text through the windows of fx_window.h (win_twin_run; the driver waits for the four bytes of the sniff).  0: proven,
// FX_UNPROVEN, FX_TOO_MANY; the records by sam_twin_windowed_count / _table / _seq, the counts by _stats (windows flushed first: 0
// means the text ended before its first flush and was scanned whole, as without windows, and no store was kept)
int sam_twin_windowed(const uint8_t *t, uint64_t n, uint64_t window, uint64_t piece) {
    return windowed_run(t, n, window, piece, true, FX_KEEP_ALL, nullptr, 0, nullptr);
}

// The same text in the two passes of the sampled ingest, as bam_twin_census / _selected.  sam_twin_census keeps
// nothing: out = {records, sequence bases, text bytes, windows flushed}.  sam_twin_selected keeps records sel[0, k) (strictly
// ascending ordinals): the accessors below read its result as they read sam_twin_windowed's (the store holds the chosen records'
// bases), sam_twin_windowed_select_stats what the run saw and kept.  0, FX_UNPROVEN, FX_TOO_MANY, or WIN_TWIN_INVALID for a
// selection that is not ascending or reaches past the records
int sam_twin_census(const uint8_t *t, uint64_t n, uint64_t window, uint64_t piece, uint64_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    const int rc = windowed_run(t, n, window, piece, true, FX_KEEP_NONE, nullptr, 0, nullptr);
    if (!rc) { out[0] = gw.sel.seen; out[1] = gw.sel.bases_seen; out[2] = n; out[3] = gw.st.windows; }
    return rc;
}

int sam_twin_selected(const uint8_t *t, uint64_t n, uint64_t window, uint64_t piece, const uint32_t *sel, uint64_t k) {
    return windowed_run(t, n, window, piece, true, FX_KEEP_SEL, sel, k, nullptr);
}

// The seek map and the mapped second pass (fx_seek.h), as bam_twin_census_map / _seek_plan / _mapped: a record starts at the first
// byte of its line (fx_rec_start with FX_LEAD_SAM), so header, @CO and empty lines lie in front of whichever point follows them;
// the planner is fx_seek_plan
int sam_twin_census_map(const uint8_t *t, uint64_t n, uint64_t window, uint64_t piece, uint64_t stride, uint64_t out[4]) {
    gm = FxSeekMap();
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!stride) return -1;
    FxSeekMap m;
    m.stride = stride;
    const int rc = windowed_run(t, n, window, piece, true, FX_KEEP_NONE, nullptr, 0, &m);
    if (rc) return rc;
    out[0] = gw.sel.seen; out[1] = gw.sel.bases_seen; out[2] = n; out[3] = gw.st.windows;
    m.records = gw.sel.seen; m.bases = gw.sel.bases_seen; m.text_bytes = m.file_len = n; m.windows = gw.st.windows; m.fmt = gw.fmt;
    gm = m;
    return 0;
}

uint64_t sam_twin_map_points(uint64_t *ord, uint64_t *off, uint64_t cap) {
    for (uint64_t i = 0; i < gm.pts.size() && i < cap; ++i) { ord[i] = gm.pts[i].ord; off[i] = gm.pts[i].off; }
    return gm.pts.size();
}

int sam_twin_seek_plan(const uint32_t *c_len, const uint32_t *isize, uint64_t n_blk, uint64_t file_len, const uint32_t *sel, uint64_t k, uint64_t out[4]) {
    return win_twin_seek_plan(gm, c_len, isize, n_blk, file_len, sel, k, &gp, out);
}
uint64_t sam_twin_plan_runs(uint64_t *out, uint64_t cap) { return win_twin_plan_runs(gp, out, cap); }
void sam_twin_plan_sel(uint32_t *out) { if (!gp.sel.empty()) memcpy(out, gp.sel.data(), gp.sel.size() * 4); }

// The mapped second pass over text t, which must be the text of the last map (WIN_TWIN_INVALID: another size): the runs of the
// plan, concatenated, are whole lines -- a SAM text without a header, scanned from its first window on without the sniff.
// FX_UNPROVEN also when the sub-text does not hold the plan's records
int sam_twin_mapped(const uint8_t *t, uint64_t n, uint64_t window, uint64_t piece, const uint32_t *sel, uint64_t k) {
    gw = WinTwinOut(); gp = FxSeekPlan();
    if (!piece) return -1;
    if (n != gm.text_bytes || gm.kind != FX_SEEK_PLAIN || win_twin_sel_fits(gm, sel, k)) return WIN_TWIN_INVALID;
    fx_seek_plan(gm, sel, k, &gp);
    const std::vector<uint8_t> sub = win_twin_sub_text(gp, t);
    int rc = windowed_run(sub.data(), sub.size(), window, piece, false, FX_KEEP_SEL, gp.sel.data(), k, nullptr);
    if (rc == WIN_TWIN_INVALID || (!rc && gw.sel.seen != gp.records)) rc = (int)FX_UNPROVEN;        // the map does not fit the input
    if (rc) { gw = WinTwinOut(); return rc; }
    win_twin_mapped_back(gw, gp, gm);
    if (gw.fmt == FX_FMT_EMPTY) gw.fmt = gm.fmt;
    return 0;
}

void sam_twin_windowed_select_stats(uint64_t out[4]) { gw.select_stats(out); }
// the records of every window of the last run, in order (at most `cap` are written); returns how many windows took records or a cut
uint64_t sam_twin_windowed_cuts(uint64_t *out, uint64_t cap) { return gw.cuts(out, cap); }

uint64_t sam_twin_windowed_count(void) { return gw.recs.size(); }
void sam_twin_windowed_table(FxRec *out) { gw.table(out); }
void sam_twin_windowed_stats(uint64_t out[4]) { gw.stats(out); }
uint64_t sam_twin_windowed_store(uint8_t *out) { return gw.store_to(out, gw.store.size()); }
uint64_t sam_twin_windowed_seq(uint64_t i, uint8_t *out) { return gw.seq(i, out); }

uint64_t sam_twin_count(void) { return g_recs.size(); }
void sam_twin_table(FxRec *out) { if (!g_recs.empty()) memcpy(out, g_recs.data(), g_recs.size() * sizeof(FxRec)); }

}  // extern "C"
}  // namespace sam_twin
