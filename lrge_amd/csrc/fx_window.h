// fx_window.h -- FASTA / FASTQ text that passes through one block in windows while only the bases stay:
// the cut rule and the driver of the windows, shared by the device (host_fastx.inl; hipcc) and the host twin (fastx_twin.cpp;
// g++).  The backend supplies the block and the record scan; the rules of the scan itself are those of fastx_core.h.
// The same driver carries unaligned BAM and SAM (bam_twin.cpp, sam_twin.cpp): only the cut differs -- the
// first incomplete record start of the proven chain (bam_round.h), the offset behind the last line feed (host_sam.inl) -- and
// the prefix is a complete run of records or lines in the same sense.
//
// Text is appended to the block piece by piece.  Once the block holds `window` bytes the driver asks for a cut: an offset
// directly behind a line feed such that the prefix [0, cut), taken as a complete text, is proven by the record scan.  The
// prefix's identifiers and lengths go to the host, its bases to the store, and [cut, end) is carried to the front of the block.
// A block without a cut keeps growing (the next attempt waits until it has doubled, so a record of many windows is scanned a
// logarithmic number of times); what is left when the input ends is the last window, a complete text with the end-of-text rules.
//
// Why the records are the host parser's: a prefix proven as a stand-alone text is leading empty lines, whole records, and --
// in the last window only -- trailing empty lines, so the host's line reader stands between two records at the cut, and the
// next window starts at a line start.  By induction over the windows the concatenation of the proven prefixes is what the host
// parser returns on the whole text; a window the scan does not prove makes the whole call unproven.
//
// The cut:
//   FASTA  the offset of the last header of the window (the prefix ends in front of a header line); no cut while that is 0.
//   FASTQ  with c line feeds and l0 / l_last the first / last non-empty line: the start of line l0 + 4k,
//          k = min((c - l0) / 4, (l_last - l0 + 1) / 4) -- whole groups of complete lines, none of them behind the last
//          non-empty line (groups of empty lines stay in the tail: they may be an empty record's, or trail the file).
// The prefix is scanned with the window's own tables: the byte in front of the cut is a line feed, so every mask of the prefix
// is what a scan of the prefix alone gives, and the parameters below are that scan's.
#pragma once
#include <stdint.h>

#include "fastx_core.h"

// windows flushed (0: the text stayed resident), bases in the store, the largest window, the bytes carried over cuts
struct FxWinStats { uint64_t windows, bases, max_window, carried; };

// the groups of four lines a FASTQ window gives to its prefix (0: no cut yet)
static inline uint64_t fx_win_fastq_groups(uint64_t n_lf, uint64_t l0, uint64_t l_last) {
    const uint64_t a = (n_lf - l0) / 4, b = (l_last - l0 + 1) / 4;
    return a < b ? a : b;
}

// What a run keeps of the records it proves.  Every mode passes the same text through the same windows with
// the same cuts and proves every window; the mode decides only what leaves the block.
//   FX_KEEP_ALL   identifiers and lengths to the host, bases to the store (every call before the selected ingest)
//   FX_KEEP_NONE  nothing: the records and their bases are counted (the census pass)
//   FX_KEEP_SEL   those of a strictly ascending list of record ordinals (file order, 0-based)
enum FxKeepMode { FX_KEEP_ALL = 0, FX_KEEP_NONE = 1, FX_KEEP_SEL = 2 };
// records seen, records kept, sequence bases seen, bases kept
struct FxSelStats { uint64_t seen, kept, bases_seen, bases_kept; };

// is sel[0, k) strictly ascending?
static inline bool fx_sel_ascending(const uint32_t *sel, uint64_t k) {
    for (uint64_t i = 1; i < k; ++i) if (sel[i] <= sel[i - 1]) return false;
    return true;
}

// The slice of a selection that falls into one window: the window holds the records [r0, r0 + n_rec), sel[0, k) is strictly
// ascending and sel[0, a) lies below r0 (the windows before took it).  Returns b: sel[a, b) are the window's, sel[b] is a later one's.
static inline uint64_t fx_sel_slice(const uint32_t *sel, uint64_t k, uint64_t a, uint64_t r0, uint64_t n_rec) {
    uint64_t lo = a, hi = k;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)sel[mid] < r0 + n_rec) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the sniff for BAM, CRAM and SAM (fx_format) belongs to the first window: a read named HD.., SQ.. or RG.. may start a later one
static inline void fx_win_census(FxCensus &c, bool first) {
    if (!first) c.head[0] = c.head[1] = c.head[2] = c.head[3] = 0;
}

// Backend B:
//   uint64_t len()                                          bytes in the block
//   int resident_format(bool *yes)                          the sniff of the block's first four bytes.  Called once, before the
//                                                           first flush: a backend that scans several formats fixes the run's
//                                                           here.  *yes: the format is not windowed (BAM, SAM with their flags
//                                                           but without the flag that windows them) -- the driver is off from
//                                                           here on, and the backend lets the block grow as a resident text
//                                                           does.  0 or the backend's code
//   int flush(bool first, bool end, uint64_t *cut, int *fmt)  the record scan of the block.  end: all of it as a complete text
//                                                           (*cut = len).  Otherwise up to the cut of the rules above (*cut = 0:
//                                                           there is none yet, nothing was taken).  The records found are
//                                                           appended to the backend's tables and store.  0 or the backend's code
//   int carry(uint64_t cut)                                 [cut, len) to the front of the block
//   int unproven(const char *what)                          the backend's code for input that is left to the host
template <class B> struct FxWindow {
    B &b;
    uint64_t window, next;
    int fmt = FX_FMT_EMPTY;
    bool sniffed = false, off = false;
    FxWinStats st = {0, 0, 0, 0};
    FxWindow(B &be, uint64_t w) : b(be), window(w ? w : 1), next(window) {}

    // behind every append, and once more with end = true when the input is over (only if a window was flushed before: text
    // that ends before its first flush is the caller's, resident as without windows).  0 or the backend's code
    int step(bool end) {
        const uint64_t len = b.len();
        if (off || (!end && len < next) || (end && len == 0)) return 0;
        if (!sniffed) {                                     // (the sniff needs the first four bytes: a smaller window waits for them)
            if (len < 4 && !end) return 0;
            sniffed = true;
            bool yes = false;
            const int src = b.resident_format(&yes);
            if (src) return src;
            if (yes) { off = true; return 0; }
        }
        if (len >> 32) return b.unproven("a window of 2^32 bytes or more");
        uint64_t cut = 0;
        int f = FX_FMT_EMPTY;
        const int rc = b.flush(st.windows == 0, end, &cut, &f);
        if (rc) return rc;
        if (!end && cut == 0) { next = 2 * len; return 0; }
        if (f != FX_FMT_EMPTY) {
            if (fmt == FX_FMT_EMPTY) fmt = f;
            else if (f != fmt) return b.unproven("a window of another format than the first");
        }
        ++st.windows;
        if (len > st.max_window) st.max_window = len;
        if (end) return 0;
        st.carried += len - cut;
        next = window;
        return b.carry(cut);
    }
};
