// sam_twin.cpp -- the host twin of the device SAM record scan (k_sam.h, host_sam.inl; g++): the same passes over the same core
// (sam_core.h, fastx_core.h) as loops on the CPU -- line starts from 16-byte groups, a mark and a rank per line, then every
// record line in steps of SAM_STEP bytes, 64 "lanes" of one 16-byte group each, the tabs ranked by an inclusive scan of the
// lanes' popcounts -- so the CPU suite checks the stepping against the host parser (tests/test_sam_twin.py); and the windowed
// ingest of fx_window.h over the same passes, with the window and the appended piece as parameters
// (tests/test_sam_window_twin.py).
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
    int scan(const std::vector<uint8_t> &blk, bool first, bool end, uint64_t *cut, int *fmt) {
        if (first && !sam_sniff(blk.data(), blk.size())) return (int)FX_UNPROVEN;     // (later windows are SAM by the run, not by their first bytes)
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
    gw = WinTwinOut();
    if (!piece) return -1;
    Scan sc;
    return win_twin_run(sc, t, n, window, piece, false, gw);
}

uint64_t sam_twin_windowed_count(void) { return gw.recs.size(); }
void sam_twin_windowed_table(FxRec *out) { gw.table(out); }
void sam_twin_windowed_stats(uint64_t out[4]) { gw.stats(out); }
uint64_t sam_twin_windowed_store(uint8_t *out) { return gw.store_to(out, gw.store.size()); }
uint64_t sam_twin_windowed_seq(uint64_t i, uint8_t *out) { return gw.seq(i, out); }

uint64_t sam_twin_count(void) { return g_recs.size(); }
void sam_twin_table(FxRec *out) { if (!g_recs.empty()) memcpy(out, g_recs.data(), g_recs.size() * sizeof(FxRec)); }

}  // extern "C"
}  // namespace sam_twin
