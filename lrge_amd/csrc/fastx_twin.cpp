// fastx_twin.cpp -- the host twin of the device record scan (k_fastx.h, host_fastx.inl; g++): the same passes over the same
// core (fastx_core.h) run tile by tile on the CPU -- census, exclusive scans, table scatter, per-record rules, sequence gather --
// with the tile size a parameter, so the CPU suite checks the algorithm against the host parser with records and lines
// straddling tile edges (tests/test_fastx_twin.py); and the windowed ingest of fx_window.h over the same passes, with the window
// and the appended piece as parameters (tests/test_fastx_window_twin.py).  TEST INFRASTRUCTURE, not part of the product library.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "fastx_core.h"
#include "win_twin.h"
#include "gz_twin.h"
#include "bz_twin.h"

namespace fastx_twin {           // (a name of its own: tools/window_twin_check.cpp holds the three twins in one translation unit)
namespace {
struct Parsed {
    int fmt = FX_FMT_EMPTY;
    std::vector<FxRec> recs;
};
Parsed g;
// a window's request (fx_window.h): null for a text that is scanned whole
struct Win { bool first, end; uint64_t cut; };

// the masks of the 16-byte group at p (a multiple of 16), as a lane of the device passes forms them
FxMasks group_at(const uint8_t *t, uint64_t n, uint64_t p) {
    uint8_t b[16] = {0};
    const uint32_t nvalid = (uint32_t)(n - p < 16 ? n - p : 16);
    memcpy(b, t + p, nvalid);
    uint32_t w[4];
    memcpy(w, b, 16);
    return fx_group_masks(w[0], w[1], w[2], w[3], p ? t[p - 1] : '\n', p + 16 < n ? t[p + 16] : FX_EOT, nvalid);
}
uint32_t valid_mask(uint64_t n, uint64_t p) { return n - p < 16 ? (1u << (n - p)) - 1 : 0xFFFFu; }

void scan_exclusive(std::vector<uint32_t> &v) {            // (wraps modulo 2^32, as the device scan does)
    uint32_t s = 0;
    for (uint32_t &x : v) { const uint32_t c = x; x = s; s += c; }
}

// the bases of record r of text t[0, n) appended to `out`, as the device copy forms them: the span in 16-byte groups, removed
// bytes dropped
void append_seq(const uint8_t *t, uint64_t n, const FxRec &r, std::vector<uint8_t> &out) {
    const uint64_t a = r.seq_off, b = r.seq_off + r.seq_span;
    for (uint64_t p = a & ~(uint64_t)15; p < b; p += 16) {
        uint32_t keep = ~group_at(t, n, p).rem & valid_mask(n, p);
        if (p < a) keep &= ~((1u << (a - p)) - 1);
        if (b - p < 16) keep &= (1u << (b - p)) - 1;
        for (; keep; keep &= keep - 1) out.push_back(t[p + (uint64_t)__builtin_ctz(keep)]);
    }
}

// the passes over t[0, n) into `g`.  w: the scan of a window -- up to its cut (w->cut; 0: none yet, g stays empty) unless w->end
int parse(const uint8_t *t, uint64_t n, uint64_t tile, Win *w) {
    g = Parsed();
    if (w) w->cut = 0;
    const uint64_t n_tiles = (n + tile - 1) / tile;
    // pass 1: the census of every tile
    std::vector<uint32_t> c_lf(n_tiles), c_rem(n_tiles), c_hdr(n_tiles);
    for (uint64_t k = 0; k < n_tiles; ++k)
        for (uint64_t p = k * tile; p < n && p < (k + 1) * tile; p += 16) {
            const FxMasks m = group_at(t, n, p);
            c_lf[k] += (uint32_t)__builtin_popcount(m.lf); c_rem[k] += (uint32_t)__builtin_popcount(m.rem); c_hdr[k] += (uint32_t)__builtin_popcount(m.hdr);
        }
    // the summary: totals, the first and last tile with a byte that stays, the exact positions inside them
    FxCensus c;
    memset(&c, 0, sizeof c);
    c.first = c.last = n;
    uint64_t t_first = n_tiles, t_last = n_tiles;
    for (uint64_t k = 0; k < n_tiles; ++k) {
        c.n_lf += c_lf[k]; c.n_rem += c_rem[k]; c.n_hdr += c_hdr[k];
        const uint64_t bytes = n - k * tile < tile ? n - k * tile : tile;
        if (c_rem[k] < bytes) { if (t_first == n_tiles) t_first = k; t_last = k; }
    }
    for (int side = 0; side < 2 && t_first < n_tiles; ++side) {
        const uint64_t k = side ? t_last : t_first;
        for (uint64_t p = k * tile; p < n && p < (k + 1) * tile; p += 16) {
            const uint32_t keep = ~group_at(t, n, p).rem & valid_mask(n, p);
            if (!keep) continue;
            if (!side) { if (c.first == n) c.first = p + (uint64_t)__builtin_ctz(keep); }
            else c.last = p + 31 - (uint64_t)__builtin_clz(keep);
        }
    }
    for (int i = 0; i < 4; ++i) c.head[i] = (uint64_t)i < n ? t[i] : 0;
    c.at_first = c.first < n ? t[c.first] : 0;
    c.tail = n ? t[n - 1] : 0;
    if (w) fx_win_census(c, w->first);
    uint32_t verdict;
    const int fmt = fx_format(n, c, &verdict);
    if (verdict) return (int)verdict;
    g.fmt = fmt;
    if (fmt == FX_FMT_EMPTY) return 0;
    if ((verdict = fx_limits(fmt, c))) return (int)verdict;
    // the censuses become offsets
    scan_exclusive(c_lf); scan_exclusive(c_rem); scan_exclusive(c_hdr);
    uint32_t flags = 0;
    if (fmt == FX_FMT_FASTQ) {
        // pass 2: the line starts; the ranks of the first and last non-empty line come out of the same pass
        std::vector<uint64_t> ls(c.n_lf + 1);
        ls[0] = 0;
        uint64_t l0 = 0, l_last = 0;
        for (uint64_t k = 0; k < n_tiles; ++k) {
            uint64_t r = c_lf[k];
            for (uint64_t p = k * tile; p < n && p < (k + 1) * tile; p += 16) {
                const uint32_t lf = group_at(t, n, p).lf;
                if (c.first >= p && c.first < p + 16) l0 = r + (uint64_t)__builtin_popcount(lf & ((1u << (c.first - p)) - 1));
                if (c.last >= p && c.last < p + 16) l_last = r + (uint64_t)__builtin_popcount(lf & ((1u << (c.last - p)) - 1));
                for (uint32_t m = lf; m; m &= m - 1) ls[++r] = p + (uint64_t)__builtin_ctz(m) + 1;
            }
        }
        uint64_t n_lines, n_rec, n_use = n, n_lf = c.n_lf;
        fx_fastq_shape(n, c, l0, l_last, &n_lines, &n_rec);
        if (w && !w->end) {                                 // the prefix of whole groups, scanned as a text of its own
            n_rec = fx_win_fastq_groups(c.n_lf, l0, l_last);
            if (!n_rec) { g.fmt = FX_FMT_EMPTY; return 0; }
            n_lf = n_lines = l0 + 4 * n_rec;
            n_use = ls[n_lf];
        }
        if (n_rec >> 32) return FX_TOO_MANY;
        g.recs.resize(n_rec);
        for (uint64_t r = 0; r < n_rec; ++r) flags |= fx_fastq_record(t, n_use, ls.data(), n_lf, n_lines, l0, r, &g.recs[r]);
        if (w) w->cut = n_use;
    } else {
        // pass 2: where every header is and how many removed bytes lie in front of it
        std::vector<uint64_t> hpos(c.n_hdr);
        std::vector<uint32_t> hrem(c.n_hdr);
        for (uint64_t k = 0; k < n_tiles; ++k) {
            uint64_t r = c_hdr[k];
            uint32_t rem = c_rem[k];
            for (uint64_t p = k * tile; p < n && p < (k + 1) * tile; p += 16) {
                const FxMasks m = group_at(t, n, p);
                for (uint32_t h = m.hdr; h; h &= h - 1) {
                    const uint32_t i = (uint32_t)__builtin_ctz(h);
                    hpos[r] = p + i; hrem[r] = rem + (uint32_t)__builtin_popcount(m.rem & ((1u << i) - 1)); ++r;
                }
                rem += (uint32_t)__builtin_popcount(m.rem);
            }
        }
        uint64_t n_rec = c.n_hdr, n_use = n, n_rem = c.n_rem;
        if (w && !w->end) {                                 // the prefix in front of the last header, scanned as a text of its own
            n_rec = c.n_hdr - 1;
            n_use = hpos[n_rec]; n_rem = hrem[n_rec];
            if (!n_use) { g.fmt = FX_FMT_EMPTY; return 0; }
            if (!n_rec) g.fmt = FX_FMT_EMPTY;               // (the empty lines in front of the first header)
        }
        g.recs.resize(n_rec);
        for (uint64_t i = 0; i < n_rec; ++i) flags |= fx_fasta_record(t, n_use, hpos.data(), hrem.data(), n_rec, n_rem, i, &g.recs[i]);
        if (w) w->cut = n_use;
    }
    if (flags) { g.recs.clear(); if (w) w->cut = 0; return flags & FX_UNPROVEN ? (int)FX_UNPROVEN : (int)FX_TOO_MANY; }
    return 0;
}

// ---- the windowed ingest: win_twin.h over the passes above ----
struct Scan {
    uint64_t tile;
    bool sniff = true;                  // false: the sub-text of a mapped run, whole records of a proven text (a run may start with a read named HD..)
    int scan(const std::vector<uint8_t> &blk, bool first, bool end, uint64_t *cut, int *fmt) {
        Win w = {first && sniff, end, 0};
        const int rc = parse(blk.data(), blk.size(), tile, &w);
        *cut = end ? blk.size() : w.cut;
        *fmt = g.fmt;
        return rc;
    }
    const std::vector<FxRec> &recs() const { return g.recs; }
    void append(const std::vector<uint8_t> &blk, uint64_t cut, const FxRec &r, std::vector<uint8_t> &store) const { append_seq(blk.data(), cut, r, store); }
};
WinTwinOut gw;
FxSeekMap gm;                           // the map of the last fastx_twin_census_map
FxSeekPlan gp;                          // the plan of the last fastx_twin_seek_plan / fastx_twin_mapped
std::vector<uint8_t> gz_text;           // the text of the last fastx_twin_gz_census_map / fastx_twin_bz_census_map
BzStats bz_st;                          // what bz_run counted in the last fastx_twin_bz_census_map
}  // namespace

extern "C" {

// 0: proven (fastx_twin_count records), FX_UNPROVEN, FX_TOO_MANY.  `tile`: bytes per tile, a multiple of 16.
int fastx_twin_parse(const uint8_t *t, uint64_t n, uint64_t tile) {
    g = Parsed();
    if (tile < 16 || tile % 16) return -1;
    return parse(t, n, tile, nullptr);
}

uint64_t fastx_twin_count(void) { return g.recs.size(); }
int fastx_twin_format(void) { return g.fmt; }
void fastx_twin_table(FxRec *out) { if (!g.recs.empty()) memcpy(out, g.recs.data(), g.recs.size() * sizeof(FxRec)); }

// the bases of record i into out[0, seq_len), as the device gather forms them: the span in 16-byte groups, removed bytes dropped;
// returns how many bytes were written
uint64_t fastx_twin_seq(const uint8_t *t, uint64_t n, uint64_t i, uint8_t *out) {
    std::vector<uint8_t> s;
    append_seq(t, n, g.recs[i], s);
    if (!s.empty()) memcpy(out, s.data(), s.size());
    return s.size();
}

// The text through the windows of fx_window.h (win_twin_run).  0: proven, FX_UNPROVEN, FX_TOO_MANY; the records by
// fastx_twin_windowed_count / _table / _seq, the counts by _stats (windows flushed first: 0 means the text ended before its first
// flush and was scanned whole, as without windows; the bases are counted all the same).
int fastx_twin_windowed(const uint8_t *t, uint64_t n, uint64_t tile, uint64_t window, uint64_t piece) {
    gw = WinTwinOut();
    if (tile < 16 || tile % 16 || !piece) return -1;
    Scan sc = {tile};
    return win_twin_run(sc, t, n, window, piece, true, gw);
}

// The same text in the two passes of the selected ingest.  fastx_twin_census keeps nothing: out = {records,
// sequence bases, text bytes, windows flushed}.  fastx_twin_selected keeps records sel[0, k) (strictly ascending ordinals): the
// accessors below read its result as they read fastx_twin_windowed's, fastx_twin_select_stats what the run saw and kept.
// 0, FX_UNPROVEN, FX_TOO_MANY, or WIN_TWIN_INVALID for a selection that is not ascending or reaches past the records
int fastx_twin_census(const uint8_t *t, uint64_t n, uint64_t tile, uint64_t window, uint64_t piece, uint64_t out[4]) {
    gw = WinTwinOut();
    out[0] = out[1] = out[2] = out[3] = 0;
    if (tile < 16 || tile % 16 || !piece) return -1;
    Scan sc = {tile};
    const int rc = win_twin_run(sc, t, n, window, piece, true, gw, FX_KEEP_NONE);
    if (!rc) { out[0] = gw.sel.seen; out[1] = gw.sel.bases_seen; out[2] = n; out[3] = gw.st.windows; }
    return rc;
}

int fastx_twin_selected(const uint8_t *t, uint64_t n, uint64_t tile, uint64_t window, uint64_t piece, const uint32_t *sel, uint64_t k) {
    gw = WinTwinOut();
    if (tile < 16 || tile % 16 || !piece) return -1;
    Scan sc = {tile};
    return win_twin_run(sc, t, n, window, piece, true, gw, FX_KEEP_SEL, sel, k);
}

// The seek map and the mapped second pass (fx_seek.h).  fastx_twin_census_map: fastx_twin_census that also keeps
// the map of the text (plain input: the file is the text), its points through the point rule the device uses, from the record table
// of every window; the points by fastx_twin_map_points (returns how many there are).
int fastx_twin_census_map(const uint8_t *t, uint64_t n, uint64_t tile, uint64_t window, uint64_t piece, uint64_t stride, uint64_t out[4]) {
    gw = WinTwinOut(); gm = FxSeekMap();
    out[0] = out[1] = out[2] = out[3] = 0;
    if (tile < 16 || tile % 16 || !piece || !stride) return -1;
    Scan sc = {tile};
    FxSeekMap m;
    m.stride = stride;
    const int rc = win_twin_run(sc, t, n, window, piece, true, gw, FX_KEEP_NONE, nullptr, 0, &m);
    if (rc) return rc;
    out[0] = gw.sel.seen; out[1] = gw.sel.bases_seen; out[2] = n; out[3] = gw.st.windows;
    m.records = gw.sel.seen; m.bases = gw.sel.bases_seen; m.text_bytes = m.file_len = n; m.windows = gw.st.windows; m.fmt = gw.fmt;
    gm = m;
    return 0;
}

uint64_t fastx_twin_map_points(uint64_t *ord, uint64_t *off, uint64_t cap) {
    for (uint64_t i = 0; i < gm.pts.size() && i < cap; ++i) { ord[i] = gm.pts[i].ord; off[i] = gm.pts[i].off; }
    return gm.pts.size();
}

// The plan of selection sel[0, k) on the last map (win_twin_seek_plan).
// out = {runs, text bytes brought, file bytes read, blocks decoded}; the runs by fastx_twin_plan_runs (ord0, n_rec, t0, t1 each; returns
// how many there are), the renumbered selection by fastx_twin_plan_sel
int fastx_twin_seek_plan(const uint32_t *c_len, const uint32_t *isize, uint64_t n_blk, uint64_t file_len, const uint32_t *sel, uint64_t k, uint64_t out[4]) {
    return win_twin_seek_plan(gm, c_len, isize, n_blk, file_len, sel, k, &gp, out);
}

uint64_t fastx_twin_plan_runs(uint64_t *out, uint64_t cap) { return win_twin_plan_runs(gp, out, cap); }
void fastx_twin_plan_sel(uint32_t *out) { if (!gp.sel.empty()) memcpy(out, gp.sel.data(), gp.sel.size() * 4); }

// The mapped second pass over text t, which must be the text of the last map (WIN_TWIN_INVALID: another size): the plan, the
// sub-text built from its runs, and the selecting run of fastx_twin_selected over the sub-text with the renumbered selection.
// FX_UNPROVEN also when the sub-text does not hold the plan's records.  The result reads as fastx_twin_selected's: name_off is
// translated back into the whole text, the select stats' seen / bases_seen are the map's
int fastx_twin_mapped(const uint8_t *t, uint64_t n, uint64_t tile, uint64_t window, uint64_t piece, const uint32_t *sel, uint64_t k) {
    gw = WinTwinOut(); gp = FxSeekPlan();
    if (tile < 16 || tile % 16 || !piece) return -1;
    if (n != gm.text_bytes || gm.kind != FX_SEEK_PLAIN || win_twin_sel_fits(gm, sel, k)) return WIN_TWIN_INVALID;
    fx_seek_plan(gm, sel, k, &gp);
    const std::vector<uint8_t> sub = win_twin_sub_text(gp, t);
    Scan sc = {tile, false};
    int rc = win_twin_run(sc, sub.data(), sub.size(), window, piece, true, gw, FX_KEEP_SEL, gp.sel.data(), k);
    if (rc == WIN_TWIN_INVALID || (!rc && gw.sel.seen != gp.records)) rc = (int)FX_UNPROVEN;        // the map does not fit the input
    if (rc) { gw = WinTwinOut(); return rc; }
    win_twin_mapped_back(gw, gp, gm);
    return 0;
}

// ---- the seek map of plain and multi-member gzip (fx_seek.h FX_SEEK_GZIP) ----
// The census with a map on gzip bytes: gz_run over the twin's backend with the recorder the device uses (chunk, round, ratio as
// gzip_twin_inflate; entries every `spacing` text bytes), the text through the windows with the point rule, the entries attached
// to the points.  A stream gz_run does not accept is FX_UNPROVEN, as on the device.  The text by fastx_twin_gz_text
int fastx_twin_gz_census_map(const uint8_t *d, uint64_t n, uint64_t chunk, uint64_t round, uint64_t ratio, uint64_t spacing, uint64_t tile, uint64_t window, uint64_t piece,
                             uint64_t stride, uint64_t out[4]) {
    gw = WinTwinOut(); gm = FxSeekMap(); gz_text.clear();
    out[0] = out[1] = out[2] = out[3] = 0;
    if (tile < 16 || tile % 16 || !piece || !stride || !spacing) return -1;
    FxSeekMap m;
    m.stride = stride; m.gz_spacing = spacing; m.kind = FX_SEEK_GZIP; m.file_len = n;
    GzTwin t;
    t.keep_wins = true;
    GzStats st;
    GzSeekRec<GzTwin> rec = {&m, spacing};
    if (gz_run(t, d, n, GzCfg{chunk, round, ratio}, [&](const uint8_t *b, uint64_t k) { gz_text.insert(gz_text.end(), b, b + k); return true; }, st, nullptr, &rec))
        return (int)FX_UNPROVEN;
    Scan sc = {tile};
    const int rc = win_twin_run(sc, gz_text.data(), gz_text.size(), window, piece, true, gw, FX_KEEP_NONE, nullptr, 0, &m);
    if (rc) { m.pts.clear(); m.n_blocks = m.ent.size(); gm = m; return rc; }      // (the entries and the text stay readable: they are the gzip side's alone)
    out[0] = gw.sel.seen; out[1] = gw.sel.bases_seen; out[2] = gz_text.size(); out[3] = gw.st.windows;
    m.records = gw.sel.seen; m.bases = gw.sel.bases_seen; m.text_bytes = gz_text.size(); m.windows = gw.st.windows; m.fmt = gw.fmt;
    fx_seek_attach_gzip(m);
    gm = m;
    return 0;
}

uint64_t fastx_twin_gz_text(uint8_t *dst) { if (dst && !gz_text.empty()) memcpy(dst, gz_text.data(), gz_text.size()); return gz_text.size(); }
uint32_t fastx_twin_gz_ring(void) { return GZ_RING; }
// would the device enter the last map (fx_gz_enterable)?  The twin's own passes enter every map: they test the decode
int fastx_twin_gz_enterable(void) { return fx_gz_enterable(gm) ? 1 : 0; }

// the entries of the last map, six words each: bit, text offset, text length, CRC-32, valid, in_member; returns how many there are
uint64_t fastx_twin_gz_entries(uint64_t *out, uint64_t cap) {
    for (uint64_t i = 0; i < gm.ent.size() && i < cap; ++i) {
        const FxGzEntry &e = gm.ent[i];
        uint64_t *o = out + 6 * i;
        o[0] = e.bit; o[1] = e.off; o[2] = e.len; o[3] = e.crc; o[4] = e.valid; o[5] = e.in_member;
    }
    return gm.ent.size();
}
// the window of entry i; and one byte of it overwritten (a damaged map)
void fastx_twin_gz_window(uint64_t i, uint8_t *dst) { memcpy(dst, gm.ent_win.data() + i * FX_GZ_WIN, FX_GZ_WIN); }
void fastx_twin_gz_poke_window(uint64_t i, uint32_t j, uint8_t v) { gm.ent_win[i * FX_GZ_WIN + j] = v; }
// the points' entry fields (lrge_hip_read_map_points' c_off, and the entry index)
uint64_t fastx_twin_gz_point_entries(uint64_t *c_off, uint64_t *blk, uint64_t cap) {
    for (uint64_t i = 0; i < gm.pts.size() && i < cap; ++i) { c_off[i] = gm.pts[i].c_off; blk[i] = gm.pts[i].blk; }
    return gm.pts.size();
}

// Entry i decoded alone from its seed out of file d[0, n) -- which may be a damaged copy of the census's -- as the device's
// wavefront decodes it, the text at byte `skew` of a 4-byte aligned block.  Returns the status word of gz_entry_run (0: out[0, len)
// is the entry's text), or -1 when a byte outside [skew, skew + len) of the block was written
int fastx_twin_gz_entry(const uint8_t *d, uint64_t n, uint64_t i, uint32_t skew, uint8_t *out) {
    if (i >= gm.ent.size()) return -1;
    const uint64_t len = gm.ent[i].len;
    std::vector<uint32_t> blk((size_t)((skew + len + 64) / 4 + 1), 0xA5A5A5A5u);
    uint8_t *b = (uint8_t *)blk.data();
    const uint32_t rc = gz_twin_entry(gm, i, d, n, i ? gm.ent_win.data() + i * FX_GZ_WIN : nullptr, b, skew);
    for (uint64_t j = 0; j < blk.size() * 4; ++j) if ((j < skew || j >= skew + len) && b[j] != 0xA5) return -1;
    if (!rc && len) memcpy(out, b + skew, (size_t)len);
    return (int)rc;
}

// The mapped second pass over gzip file d, which must have the length of the last map's (WIN_TWIN_INVALID): the plan, every entry the
// runs touch decoded once from its seed, the sub-text built from what the runs take of them, and the selecting run over it, as
// fastx_twin_mapped.  An entry that fails its checks is FX_UNPROVEN: the map does not fit the input
int fastx_twin_gz_mapped(const uint8_t *d, uint64_t n, uint64_t tile, uint64_t window, uint64_t piece, const uint32_t *sel, uint64_t k) {
    gw = WinTwinOut(); gp = FxSeekPlan();
    if (tile < 16 || tile % 16 || !piece) return -1;
    if (n != gm.file_len || gm.kind != FX_SEEK_GZIP || win_twin_sel_fits(gm, sel, k)) return WIN_TWIN_INVALID;
    fx_seek_plan(gm, sel, k, &gp);
    std::vector<uint8_t> sub;
    std::vector<uint8_t> txt;
    uint64_t have = ~(uint64_t)0, decoded = 0;           // the entry in txt
    for (const FxSeekRun &r : gp.runs)
        for (uint64_t b = r.b0; b < r.b1; ++b) {
            const FxGzEntry &e = gm.ent[b];
            if (have != b) {
                txt.assign((size_t)e.len + 8, 0);
                std::vector<uint32_t> al((size_t)(e.len / 4 + 4));
                if (gz_twin_entry(gm, b, d, n, b ? gm.ent_win.data() + b * FX_GZ_WIN : nullptr, (uint8_t *)al.data(), (uint32_t)(sub.size() & 3))) return (int)FX_UNPROVEN;
                memcpy(txt.data(), (uint8_t *)al.data() + (sub.size() & 3), (size_t)e.len);
                have = b; ++decoded;
            }
            const uint64_t a = std::max(r.t0, e.off), z = std::min(r.t1, e.off + e.len);
            if (a < z) sub.insert(sub.end(), txt.begin() + (long)(a - e.off), txt.begin() + (long)(z - e.off));
        }
    if (decoded != gp.blocks || sub.size() != gp.text_bytes) return (int)FX_UNPROVEN;       // (never: the planner counts what is decoded)
    Scan sc = {tile, false};
    int rc = win_twin_run(sc, sub.data(), sub.size(), window, piece, true, gw, FX_KEEP_SEL, gp.sel.data(), k);
    if (rc == WIN_TWIN_INVALID || (!rc && gw.sel.seen != gp.records)) rc = (int)FX_UNPROVEN;
    if (rc) { gw = WinTwinOut(); return rc; }
    win_twin_mapped_back(gw, gp, gm);
    return 0;
}
// ---- the seek map of bzip2 (fx_seek.h FX_SEEK_BZIP2) ----
// The census with a map on bzip2 bytes: bz_run over the twin's backend with the recorder the device uses (round_blocks as
// bz_twin_inflate; entries every `spacing` text bytes), the text through the windows with the point rule, the entries attached to the
// points.  A stream bz_run does not accept is FX_UNPROVEN, as on the device.  The text by fastx_twin_gz_text, bz_run's counts by
// fastx_twin_bz_stats (blocks, candidates, rejected candidates, rounds, bytes out)
int fastx_twin_bz_census_map(const uint8_t *d, uint64_t n, uint64_t round_blocks, uint64_t spacing, uint64_t tile, uint64_t window, uint64_t piece, uint64_t stride, uint64_t out[4]) {
    gw = WinTwinOut(); gm = FxSeekMap(); gz_text.clear(); bz_st = BzStats{0, 0, 0, 0, 0};
    out[0] = out[1] = out[2] = out[3] = 0;
    if (tile < 16 || tile % 16 || !piece || !stride || !spacing) return -1;
    FxSeekMap m;
    m.stride = stride; m.bz_spacing = spacing; m.kind = FX_SEEK_BZIP2; m.file_len = n; m.bz_level = n >= 4 ? d[3] : 0;
    BzTwin t;
    t.keep_marks = true;
    BzSeekRec<BzTwin, FxSeekMap> rec = {&m, spacing};
    if (bz_run(t, d, n, round_blocks, [&](const uint8_t *b, uint64_t k) { gz_text.insert(gz_text.end(), b, b + k); return true; }, bz_st, nullptr, nullptr, &rec))
        return (int)FX_UNPROVEN;
    Scan sc = {tile};
    const int rc = win_twin_run(sc, gz_text.data(), gz_text.size(), window, piece, true, gw, FX_KEEP_NONE, nullptr, 0, &m);
    if (rc) { m.pts.clear(); m.n_blocks = m.bz_ent.size(); gm = m; return rc; }   // (blocks, marks and text stay readable: they are the bzip2 side's alone)
    out[0] = gw.sel.seen; out[1] = gw.sel.bases_seen; out[2] = gz_text.size(); out[3] = gw.st.windows;
    m.records = gw.sel.seen; m.bases = gw.sel.bases_seen; m.text_bytes = gz_text.size(); m.windows = gw.st.windows; m.fmt = gw.fmt;
    fx_seek_attach_bzip2(m);
    gm = m;
    return 0;
}
void fastx_twin_bz_stats(uint64_t out[5]) { out[0] = bz_st.blocks; out[1] = bz_st.candidates; out[2] = bz_st.rejected; out[3] = bz_st.rounds; out[4] = bz_st.bytes_out; }
// would the device enter the last map (fx_bz_enterable)?  The twin's own passes enter every map: they test the decode
int fastx_twin_bz_enterable(void) { return fx_bz_enterable(gm) ? 1 : 0; }

// the entries of the last map, six words each: first block, the block behind the last, text offset, text length, first file byte, the
// file byte behind the last; returns how many there are
uint64_t fastx_twin_bz_entries(uint64_t *out, uint64_t cap) {
    for (uint64_t i = 0; i < gm.bz_ent.size() && i < cap; ++i) {
        const FxBzEntry &e = gm.bz_ent[i];
        uint64_t *o = out + 6 * i;
        o[0] = e.b0; o[1] = e.b1; o[2] = e.off; o[3] = e.len; o[4] = fx_bz_cover_begin(gm, i); o[5] = fx_bz_cover_end(gm, i);
    }
    return gm.bz_ent.size();
}
// ... its blocks, eight words each: bit, end bit, text offset, text length, n, origPtr, stored CRC, entry
uint64_t fastx_twin_bz_blocks(uint64_t *out, uint64_t cap) {
    for (uint64_t i = 0; i < gm.bz.size() && i < cap; ++i) {
        const FxBzBlock &b = gm.bz[i];
        uint64_t *o = out + 8 * i;
        o[0] = b.bit; o[1] = b.end_bit; o[2] = b.off; o[3] = b.len; o[4] = b.n; o[5] = b.orig; o[6] = b.crc; o[7] = b.ent;
    }
    return gm.bz.size();
}
// ... the marks of block b, four words each (at, state, text offset, CRC register), FX_BZ_MARKS of them; and one word of one overwritten (a damaged map)
void fastx_twin_bz_marks(uint64_t b, uint32_t *out) { memcpy(out, &gm.bz_marks[b * FX_BZ_MARKS], FX_BZ_MARKS * sizeof(BzMark)); }
void fastx_twin_bz_poke_mark(uint64_t b, uint32_t j, uint32_t word, uint32_t v) { ((uint32_t *)&gm.bz_marks[b * FX_BZ_MARKS + j])[word] = v; }

// Block b of the last map entered out of file d[0, n) -- which may be a damaged copy of the census's -- the text at byte `skew` of a 4-byte
// aligned area: lane j alone from its mark (its segment, out[0, *len) the bytes between mark j's text offset and the next's), or, with
// j >= FX_BZ_MARKS, the whole block by every lane (out[0, *len) its text).  0, a decode status or BZ_E_ENTRY; -1 when a byte outside
// the lane's (the block's) text range was written
int fastx_twin_bz_segment(const uint8_t *d, uint64_t n, uint64_t b, uint32_t j, uint32_t skew, uint8_t *out, uint64_t *len) {
    *len = 0;
    if (b >= gm.bz.size() || n < 4) return -1;
    const FxBzBlock &k = gm.bz[b];
    const BzMark *m = &gm.bz_marks[b * FX_BZ_MARKS];
    const uint32_t nm = bz_mark_count(k.n);
    uint64_t t0 = 0, t1 = k.len;
    if (j < FX_BZ_MARKS) { if (j >= nm) return 0; t0 = m[j].off; t1 = j + 1 < nm ? m[j + 1].off : k.len; }
    if (t0 > t1 || t1 > k.len) return (int)BZ_E_ENTRY;
    std::vector<uint32_t> area((size_t)((skew + k.len + 64) / 4 + 1), 0xA5A5A5A5u);
    uint8_t *a = (uint8_t *)area.data();
    const uint32_t rc = bz_twin_seeded(d, n, (uint32_t)(gm.bz_level - '0') * 100000u, k.bit, k.end_bit - k.bit, k.n, k.orig, k.crc, (uint32_t)k.len, m, a + skew, j);
    for (uint64_t i = 0; i < area.size() * 4; ++i) if ((i < skew + t0 || i >= skew + t1) && a[i] != 0xA5) return -1;
    if (!rc && t1 > t0) memcpy(out, a + skew + t0, (size_t)(t1 - t0));
    if (!rc) *len = t1 - t0;
    return (int)rc;
}

// The mapped second pass over bzip2 file d, which must have the length of the last map's (WIN_TWIN_INVALID): the plan, every block of the
// entries the runs touch entered once at its marks, the sub-text built from what the runs take of them, and the selecting run over it,
// as fastx_twin_mapped.  A block that fails its checks is FX_UNPROVEN (*status: its decode status or BZ_E_ENTRY): the map does not fit the input
int fastx_twin_bz_mapped(const uint8_t *d, uint64_t n, uint64_t tile, uint64_t window, uint64_t piece, const uint32_t *sel, uint64_t k, uint32_t *status) {
    gw = WinTwinOut(); gp = FxSeekPlan();
    if (status) *status = 0;
    if (tile < 16 || tile % 16 || !piece) return -1;
    if (n != gm.file_len || gm.kind != FX_SEEK_BZIP2 || win_twin_sel_fits(gm, sel, k)) return WIN_TWIN_INVALID;
    fx_seek_plan(gm, sel, k, &gp);
    std::vector<uint8_t> sub;
    uint64_t prev_b1 = 0, decoded = 0;
    bool any = false;
    for (const FxSeekRun &r : gp.runs) {
        for (uint64_t e = r.b0; e < r.b1; ++e) {
            if (any && e < prev_b1) continue;                // (decoded for the run before: its text is in `last`)
            ++decoded;
        }
        for (uint64_t e = r.b0; e < r.b1; ++e)
            for (uint64_t b = gm.bz_ent[e].b0; b < gm.bz_ent[e].b1; ++b) {
                const FxBzBlock &q = gm.bz[b];
                const uint64_t a = std::max(r.t0, q.off), z = std::min(r.t1, q.off + q.len);
                std::vector<uint32_t> al((size_t)(q.len / 4 + 4));
                uint8_t *txt = (uint8_t *)al.data() + (sub.size() & 3);
                const uint32_t rc = bz_twin_seeded(d, n, (uint32_t)(gm.bz_level - '0') * 100000u, q.bit, q.end_bit - q.bit, q.n, q.orig, q.crc, (uint32_t)q.len, &gm.bz_marks[b * FX_BZ_MARKS], txt);
                if (rc) { if (status) *status = rc; return (int)FX_UNPROVEN; }
                if (a < z) sub.insert(sub.end(), txt + (a - q.off), txt + (z - q.off));
            }
        prev_b1 = r.b1; any = true;
    }
    if (decoded != gp.blocks || sub.size() != gp.text_bytes) return (int)FX_UNPROVEN;       // (never: the planner counts what is decoded)
    Scan sc = {tile, false};
    int rc = win_twin_run(sc, sub.data(), sub.size(), window, piece, true, gw, FX_KEEP_SEL, gp.sel.data(), k);
    if (rc == WIN_TWIN_INVALID || (!rc && gw.sel.seen != gp.records)) rc = (int)FX_UNPROVEN;
    if (rc) { gw = WinTwinOut(); return rc; }
    win_twin_mapped_back(gw, gp, gm);
    return 0;
}
void fastx_twin_plan_stats(uint64_t out[4]) { out[0] = gp.runs.size(); out[1] = gp.text_bytes; out[2] = gp.file_bytes; out[3] = gp.blocks; }

void fastx_twin_select_stats(uint64_t out[4]) { gw.select_stats(out); }
// the dense store of the kept bases, bytes [0, fastx_twin_windowed_stats()[1])
uint64_t fastx_twin_windowed_store(uint8_t *out, uint64_t bytes) { return gw.store_to(out, bytes < gw.store.size() ? bytes : gw.store.size()); }

// the records of every window of the last run, in order (at most `cap` are written); returns how many windows took records or a cut
uint64_t fastx_twin_windowed_cuts(uint64_t *out, uint64_t cap) { return gw.cuts(out, cap); }

uint64_t fastx_twin_windowed_count(void) { return gw.recs.size(); }
int fastx_twin_windowed_format(void) { return gw.fmt; }
void fastx_twin_windowed_table(FxRec *out) { gw.table(out); }
void fastx_twin_windowed_stats(uint64_t out[4]) { gw.stats(out); }
uint64_t fastx_twin_windowed_seq(uint64_t i, uint8_t *out) { return gw.seq(i, out); }

}  // extern "C"
}  // namespace fastx_twin
