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
        if (map) for (uint64_t i = 0; i < n_rec; ++i) fx_seek_add(*map, r0 + i, base + recs[i].name_off - 1);
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
// at or above the records the run saw.  map: a census (FX_KEEP_NONE) fills the points of a seek map (fx_seek.h; stride set by the caller)
#define WIN_TWIN_INVALID (-2)
template <class Scan> int win_twin_run(Scan &scan, const uint8_t *t, uint64_t n, uint64_t window, uint64_t piece, bool resident_bases, WinTwinOut &out,
                                       FxKeepMode mode = FX_KEEP_ALL, const uint32_t *sel = nullptr, uint64_t k = 0, FxSeekMap *map = nullptr) {
    out = WinTwinOut();
    if (mode == FX_KEEP_SEL && ((k && !sel) || !fx_sel_ascending(sel, k))) return WIN_TWIN_INVALID;
    WinTwin<Scan> b(scan, out);
    b.mode = mode; b.sel = sel; b.k = k; b.map = map;
    FxWindow<WinTwin<Scan>> win(b, window);
    int rc = 0;
    for (uint64_t p = 0; p < n && !rc; p += piece) {
        b.blk.insert(b.blk.end(), t + p, t + (n - p < piece ? n : p + piece));
        rc = win.step(false);
    }
    uint64_t all = 0;
    if (!rc) rc = win.st.windows ? win.step(true) : b.flush(true, true, &all, &win.fmt);         // (or the resident scan)
    if (!rc && mode == FX_KEEP_SEL && b.at < k) rc = WIN_TWIN_INVALID;
    if (rc) { out = WinTwinOut(); return rc; }
    out.st = win.st; out.st.bases = win.st.windows || resident_bases ? out.store.size() : 0;
    out.fmt = win.fmt;
    return 0;
}
