// win_twin.h -- the windowed backend of the host twins (fastx_twin.cpp, bam_twin.cpp, sam_twin.cpp; g++), once for the three: the
// block, the carry, the records and the store of the bases, the loop over the pieces and the counts, under the driver of
// fx_window.h.  A twin supplies its record scan:
//   int scan(blk, bool first, bool end, uint64_t *cut, int *fmt)   the block as the first / the last window: 0 with *cut (end: the
//       block's size; else 0 when there is no cut yet), the format and the records of [0, *cut) behind recs(), or its verdict
//   void append(blk, cut, const FxRec &r, store)                   the bases of record r of the prefix, as the device stores them
// TEST INFRASTRUCTURE, not part of the product library.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "fx_window.h"
#include "fx_seek.h"

// what a windowed run leaves, behind the <twin>_windowed_* accessors
struct WinTwinOut {
    std::vector<FxRec> recs;            // name_off: in the whole text; seq_off: in `store`; seq_span: the record's bytes there
    std::vector<uint8_t> store;         // the bases of every record, dense, in file order
    FxWinStats st = {0, 0, 0, 0};
    FxSelStats sel = {0, 0, 0, 0};      // a run that does not keep all (fx_window.h FxKeepMode): what it saw and what it kept
    std::vector<uint64_t> win_recs;     // the records of every flush that took a prefix, in order: where the run's cuts fell
    int fmt = FX_FMT_EMPTY;
    uint64_t cuts(uint64_t *o, uint64_t cap) const { for (uint64_t i = 0; i < win_recs.size() && i < cap; ++i) o[i] = win_recs[i]; return win_recs.size(); }
    void table(FxRec *out) const { if (!recs.empty()) memcpy(out, recs.data(), recs.size() * sizeof(FxRec)); }
    void select_stats(uint64_t o[4]) const { o[0] = sel.seen; o[1] = sel.kept; o[2] = sel.bases_seen; o[3] = sel.bases_kept; }
    void stats(uint64_t out[4]) const { out[0] = st.windows; out[1] = st.bases; out[2] = st.max_window; out[3] = st.carried; }
    uint64_t store_to(uint8_t *out, uint64_t bytes) const { if (out && bytes) memcpy(out, store.data(), bytes); return bytes; }
    uint64_t seq(uint64_t i, uint8_t *out) const {           // (a store of plain bases)
        const FxRec &r = recs[i];
        if (r.seq_len) memcpy(out, store.data() + r.seq_off, r.seq_len);
        return r.seq_len;
    }
};

// the backend of FxWindow over a twin's scan
template <class Scan> struct WinTwin {
    Scan &scan;
    WinTwinOut &out;
    std::vector<uint8_t> blk;
    uint64_t base = 0;                  // where the block starts in the whole text
    FxKeepMode mode = FX_KEEP_ALL;      // FX_KEEP_SEL: sel[0, k), strictly ascending; sel[0, at) lay in the windows flushed so far
    const uint32_t *sel = nullptr;
    uint64_t k = 0, at = 0;
    FxSeekMap *map = nullptr;           // a census that leaves a seek map (fx_seek.h): every window's records go through the point rule
    uint32_t lead = FX_LEAD_TEXT;       // where a record starts in front of its identifier (fx_rec_start): FX_LEAD_BAM for a BAM twin, FX_LEAD_SAM for a SAM twin
    WinTwin(Scan &s, WinTwinOut &o) : scan(s), out(o) {}
    void keep(const FxRec &r, uint64_t cut) {
        const uint64_t a = out.store.size();
        scan.append(blk, cut, r, out.store);
        out.recs.push_back(FxRec{base + r.name_off, a, out.store.size() - a, r.name_len, r.seq_len});
    }
    uint64_t len() const { return blk.size(); }
    int resident_format(bool *yes) const { *yes = false; return 0; }        // (a twin scans one format, and windows it)
    int unproven(const char *) const { return (int)FX_UNPROVEN; }
    int flush(bool first, bool end, uint64_t *cut, int *fmt) {
        const int rc = scan.scan(blk, first, end, cut, fmt);
        if (rc || !*cut) return rc;
        const std::vector<FxRec> &recs = scan.recs();
        out.win_recs.push_back(recs.size());
        if (mode == FX_KEEP_ALL) {
            for (const FxRec &r : recs) keep(r, *cut);
            return 0;
        }
        // the census and the selection: every record is counted, the window's slice of the selection is kept
        const uint64_t r0 = out.sel.seen, n_rec = recs.size();
        if ((r0 + n_rec) >> 32) return (int)FX_UNPROVEN;
        const uint64_t b = mode == FX_KEEP_SEL ? fx_sel_slice(sel, k, at, r0, n_rec) : at;
        if (map) for (uint64_t i = 0; i < n_rec; ++i) fx_seek_add(*map, r0 + i, base + fx_rec_start(recs[i].name_off, lead));
        for (const FxRec &r : recs) out.sel.bases_seen += r.seq_len;
        for (; at < b; ++at) {
            const FxRec &r = recs[sel[at] - r0];
            keep(r, *cut);
            ++out.sel.kept; out.sel.bases_kept += r.seq_len;
        }
        out.sel.seen += n_rec;
        return 0;
    }
    int carry(uint64_t cut) {
        blk.erase(blk.begin(), blk.begin() + (long)cut);
        base += cut;
        return 0;
    }
};

// The text through the windows of fx_window.h: `piece` bytes appended per step, a flush once the block holds `window` bytes;
// a text that ends before its first flush is scanned whole, as without windows (resident_bases: its bases count in the stats all
// the same).  0 with `out` filled, or the verdict with `out` empty
// mode, sel, k: what the run keeps (fx_window.h FxKeepMode); WIN_TWIN_INVALID: sel is not strictly ascending, or holds an ordinal
// at or above the records the run saw.  map: a census (FX_KEEP_NONE) fills the points of a seek map (fx_seek.h; stride set by the caller),
// a record starting `lead` bytes in front of its identifier
#define WIN_TWIN_INVALID (-2)
template <class Scan> int win_twin_run(Scan &scan, const uint8_t *t, uint64_t n, uint64_t window, uint64_t piece, bool resident_bases, WinTwinOut &out,
                                       FxKeepMode mode = FX_KEEP_ALL, const uint32_t *sel = nullptr, uint64_t k = 0, FxSeekMap *map = nullptr, uint32_t lead = FX_LEAD_TEXT) {
    out = WinTwinOut();
    if (mode == FX_KEEP_SEL && ((k && !sel) || !fx_sel_ascending(sel, k))) return WIN_TWIN_INVALID;
    WinTwin<Scan> b(scan, out);
    b.mode = mode; b.sel = sel; b.k = k; b.map = map; b.lead = lead;
    FxWindow<WinTwin<Scan>> win(b, window);
    int rc = 0;
    for (uint64_t p = 0; p < n && !rc; p += piece) {
        b.blk.insert(b.blk.end(), t + p, t + (n - p < piece ? n : p + piece));
        rc = win.step(false);
    }
    uint64_t all = 0;
    // (or the resident scan; `first` is the driver's word: the scan of a mapped sub-text clears it itself, as in every window)
    if (!rc) rc = win.st.windows ? win.step(true) : b.flush(true, true, &all, &win.fmt);
    if (!rc && mode == FX_KEEP_SEL && b.at < k) rc = WIN_TWIN_INVALID;
    if (rc) { out = WinTwinOut(); return rc; }
    out.st = win.st; out.st.bases = win.st.windows || resident_bases ? out.store.size() : 0;
    out.fmt = win.fmt;
    return 0;
}

// ---- the seek map of a twin (fx_seek.h), once for the twins that have one (fastx_twin.cpp, bam_twin.cpp, sam_twin.cpp) ----
// the selection against map m: 0, or WIN_TWIN_INVALID for one that is not ascending or reaches the map's records
static inline int win_twin_sel_fits(const FxSeekMap &m, const uint32_t *sel, uint64_t k) {
    if ((k && !sel) || !fx_sel_ascending(sel, k)) return WIN_TWIN_INVALID;
    for (uint64_t j = 0; j < k; ++j) if (sel[j] >= m.records) return WIN_TWIN_INVALID;
    return 0;
}

// The plan of selection sel[0, k) on map gm.  n_blk == 0: for the plain text.  Else for the same text in BGZF blocks of member
// lengths c_len and text sizes isize (a file of file_len bytes): the block fields are attached as the device attaches them.
// out = {runs, text bytes brought, file bytes read, blocks decoded}
static inline int win_twin_seek_plan(const FxSeekMap &gm, const uint32_t *c_len, const uint32_t *isize, uint64_t n_blk, uint64_t file_len, const uint32_t *sel, uint64_t k,
                                     FxSeekPlan *gp, uint64_t out[4]) {
    *gp = FxSeekPlan();
    out[0] = out[1] = out[2] = out[3] = 0;
    if (win_twin_sel_fits(gm, sel, k)) return WIN_TWIN_INVALID;
    FxSeekMap m = gm;
    if (n_blk) {
        std::vector<BgzfBlock> t(n_blk);
        uint64_t c = 0, o = 0;
        for (uint64_t i = 0; i < n_blk; ++i) { t[i] = BgzfBlock{c, o, 0, 0, c_len[i], isize[i], 0}; c += c_len[i]; o += isize[i]; }
        if (o != m.text_bytes || c != file_len) return WIN_TWIN_INVALID;
        m.kind = FX_SEEK_BGZF; m.n_blocks = n_blk; m.file_len = file_len;
        fx_seek_attach(m, t.data(), n_blk);
    }
    fx_seek_plan(m, sel, k, gp);
    out[0] = gp->runs.size(); out[1] = gp->text_bytes; out[2] = gp->file_bytes; out[3] = gp->blocks;
    return 0;
}

static inline uint64_t win_twin_plan_runs(const FxSeekPlan &gp, uint64_t *out, uint64_t cap) {
    for (uint64_t i = 0; i < gp.runs.size() && i < cap; ++i) { out[4 * i] = gp.runs[i].ord0; out[4 * i + 1] = gp.runs[i].n_rec; out[4 * i + 2] = gp.runs[i].t0; out[4 * i + 3] = gp.runs[i].t1; }
    return gp.runs.size();
}

// the sub-text of plan gp over text t, and -- behind the selecting run over it -- the records' name_off translated back into the
// whole text, the select stats' seen / bases_seen the map's
static inline std::vector<uint8_t> win_twin_sub_text(const FxSeekPlan &gp, const uint8_t *t) {
    std::vector<uint8_t> sub;
    for (const FxSeekRun &r : gp.runs) sub.insert(sub.end(), t + r.t0, t + r.t1);
    return sub;
}
static inline void win_twin_mapped_back(WinTwinOut &gw, const FxSeekPlan &gp, const FxSeekMap &gm) {
    size_t ri = 0;
    uint64_t before = 0;                // sub-text bytes in front of run ri
    for (FxRec &r : gw.recs) {
        while (r.name_off >= before + (gp.runs[ri].t1 - gp.runs[ri].t0)) { before += gp.runs[ri].t1 - gp.runs[ri].t0; ++ri; }
        r.name_off = r.name_off - before + gp.runs[ri].t0;
    }
    gw.sel.seen = gm.records; gw.sel.bases_seen = gm.bases;
}
