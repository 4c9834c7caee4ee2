// fx_seek.h -- the seek map of a FASTA / FASTQ text, of unaligned BAM or of unaligned SAM and the plan of a pass that brings only the
// chosen runs (DESIGN sections 24, 25 and 27), shared by the device (host_fastx.inl; hipcc) and the host twins (fastx_twin.cpp,
// bam_twin.cpp, sam_twin.cpp; g++), as fx_window.h is.
//
// The census that proves the text (fx_window.h FX_KEEP_NONE) can leave a map behind.  The whole text is cut into cells of
// `stride` bytes; a cell in which at least one record starts gets one point: the first record that starts in it.  Where a record
// starts is fx_rec_start: FASTA / FASTQ at the first byte of its header line, the '>' or '@' (FxRec::name_off - FX_LEAD_TEXT); BAM at
// its block_size field (FxRec::name_off - FX_LEAD_BAM, bam_record), so the BAM header lies in front of record 0's point at hdr_end as
// leading blank lines do; SAM at the first byte of its line (FxRec::name_off itself, sam_record: FX_LEAD_SAM is 0), so header, @CO
// and empty lines lie in front of whichever point follows them.  A point holds the record's ordinal (file order,
// 0-based), its text offset and, for BGZF, the block that holds that offset.  Cells inside one long record have no point; the
// points ascend strictly in ordinal and in offset, and the first point is record 0.
//
// The plan of a selection (strictly ascending ordinals): for each chosen ordinal the run from the last point at or below it to
// the first point above it, or to the end of the text; runs that touch or overlap are merged.  The sub-text -- the runs'
// bytes, concatenated -- is a text of whole records (a run starts at a header line and ends directly behind a line feed or at the
// end of the text; a BAM run starts at a block_size field and ends in front of the next, so the sub-text is a record stream without
// a header; a SAM run is whole lines, the sub-text a SAM text without a header), and the selection renumbered into its ordinals names the same records.
#pragma once
#include <stdint.h>

#include <vector>

#include "bgzf_scan.h"
#include "bz_core.h"
#include "fx_window.h"

// OTHER: a container that cannot be entered (xz), or is not worth entering; CRAM: no text at all -- a point is a slice (cram_round.h cram_seek_map:
// ord the first record that starts in it, off its base offset, c_off the file offset of its BA block, blk the slice), n_blocks the slices;
// GZIP: plain or multi-member gzip, entered at the entries below, n_blocks the entries;
// BZIP2: entered at whole blocks, a block at its marks, n_blocks the entries
enum { FX_SEEK_PLAIN = 0, FX_SEEK_BGZF = 1, FX_SEEK_OTHER = 2, FX_SEEK_CRAM = 3, FX_SEEK_GZIP = 4, FX_SEEK_BZIP2 = 5 };
#define FX_SEEK_NONE 0xFFFFFFFFu                                     // a cell's slot without a record start

// the record-start rule: a record starts `lead` bytes in front of its identifier
#define FX_LEAD_TEXT 1u                                              // the '>' or '@'
#define FX_LEAD_BAM 36u                                              // block_size and the 32 bytes of fixed fields (bam_record)
#define FX_LEAD_SAM 0u                                               // the identifier is the first field of the line (sam_record)
FX_HD uint64_t fx_rec_start(uint64_t name_off, uint32_t lead) { return name_off - lead; }

// blk: the index of the block that holds text offset `off` (o_off <= off < o_off + ISIZE), c_off / o_off / c_len its file offset,
// text offset and member length; plain input: all 0
struct FxSeekPoint { uint64_t ord, off, c_off, o_off; uint32_t c_len; uint32_t blk; };

// One entry of a gzip file (gzip_round.h GzSeekRec): a true boundary of the stream at absolute bit offset `bit`, where text offset
// `off` starts; the stream is inside a member there (in_member) of which `valid` bytes of the 32 KiB window in front belong to it; the text
// from here to the next entry (the last: to the end) has `len` bytes and CRC-32 `crc`.  Entry i's window is ent_win[i * FX_GZ_WIN ..]:
// the text [off - 32768, off), zeros in front of the text.  The windows are host memory outside INGEST_MAX_BYTES: 32 KiB an
// entry, 1.6 % of the text at the default spacing and chunk (an entry every 2 MiB of text or so).
// An entry is decoded from file bytes [bit >> 3, fx_gz_cover_end): FX_GZ_SLACK bytes past the next entry's byte, so that the stop rule
// (gzip_core.h gz_canon, gz_is_header) sees the boundary it ends at as the census saw it
#define FX_GZ_WIN 32768u
#define FX_GZ_SLACK 16u
struct FxGzEntry { uint64_t bit, off, len; uint32_t crc, valid, in_member, pad; };

// One accepted block of a bzip2 file (bz_round.h BzSeekRec): it starts at absolute bit offset `bit` (its magic) and ends in front of
// `end_bit`; n bytes in front of the run-length layer, origPtr `orig`, the stored block CRC `crc`; its text is [off, off + len) and it
// belongs to entry `ent`.  Block b's marks are bz_marks[b * FX_BZ_MARKS ..] (bz_core.h BzMark): 1 KiB a block of host memory outside
// INGEST_MAX_BYTES, about 0.1 % of a level-9 block.
// An entry is a group of whole consecutive blocks [b0, b1): a new one opens at the first accepted block whose text offset is at least
// the spacing behind the previous entry's.  Its file bytes run from bit >> 3 of its first block to (end_bit + 7) >> 3 of its last,
// without slack: a block decoded from a true start stops by itself
#define FX_BZ_MARKS BZ_MARKS
struct FxBzBlock { uint64_t bit, end_bit, off, len; uint32_t n, orig, crc, ent; };
struct FxBzEntry { uint64_t b0, b1, off, len; };

struct FxSeekMap {
    uint64_t records = 0, bases = 0, text_bytes = 0, file_len = 0, n_blocks = 0, stride = 65536, windows = 0;
    int kind = FX_SEEK_PLAIN, fmt = FX_FMT_EMPTY;
    std::vector<FxSeekPoint> pts;
    uint64_t last_cell = 0;                      // the cell of the last point (the builder's)
    std::vector<FxGzEntry> ent;                  // FX_SEEK_GZIP: the entries, ascending in bit and in text offset; entry 0 is bit 0
    std::vector<uint8_t> ent_win;                // ... and their windows
    uint64_t gz_spacing = 0;                     // ... and the spacing they were taken at (option INGEST_SEEK_GZIP_BYTES)
    uint64_t gz_links = 0;                       // ... and the accepted chunks of the census they were taken from
    std::vector<FxBzBlock> bz;                   // FX_SEEK_BZIP2: the accepted blocks in file order; block 0 is bit 32
    std::vector<BzMark> bz_marks;                // ... their marks
    std::vector<FxBzEntry> bz_ent;               // ... the entries
    uint64_t bz_spacing = 0;                     // ... the spacing they were taken at (option INGEST_SEEK_BZIP2_BYTES)
    uint32_t bz_level = 0;                       // ... and the level byte of the stream header ('1'..'9')
};

// Is a gzip map worth entering?  Not when the spacing left entry 0 alone although the census walked several chunks: the mapped open
// could skip nothing and would decode by one wavefront what the selected pass decodes by one a chunk.  Such a map gets the kind
// "other" (the full selected pass, 0 runs).  A file of one chunk is one entry either way and is entered
static inline bool fx_gz_enterable(const FxSeekMap &m) { return m.ent.size() > 1 || m.gz_links <= 1; }

// the file bytes of entry i end here
static inline uint64_t fx_gz_cover_end(const FxSeekMap &m, uint64_t i) {
    if (i + 1 >= m.ent.size()) return m.file_len;
    const uint64_t e = (m.ent[i + 1].bit >> 3) + FX_GZ_SLACK;
    return e < m.file_len ? e : m.file_len;
}

// Is a bzip2 map worth entering?  Not when its only entry spans several blocks: nothing could be skipped.  A file of one block is one
// entry and is entered
static inline bool fx_bz_enterable(const FxSeekMap &m) { return m.bz_ent.size() > 1 || m.bz.size() <= 1; }
static inline uint64_t fx_bz_cover_begin(const FxSeekMap &m, uint64_t i) { return m.bz[m.bz_ent[i].b0].bit >> 3; }
static inline uint64_t fx_bz_cover_end(const FxSeekMap &m, uint64_t i) { return (m.bz[m.bz_ent[i].b1 - 1].end_bit + 7) >> 3; }

// the point rule: record `ord` starts at text offset `off`; records arrive in file order.  A window's first cell may be one an
// earlier window gave a point to: the earlier point stands
static inline void fx_seek_add(FxSeekMap &m, uint64_t ord, uint64_t off) {
    const uint64_t cell = off / m.stride;
    if (!m.pts.empty() && cell == m.last_cell) return;
    m.pts.push_back(FxSeekPoint{ord, off, 0, 0, 0, 0});
    m.last_cell = cell;
}

// the block fields of every point from the block table of the file the census read
static inline void fx_seek_attach(FxSeekMap &m, const BgzfBlock *t, uint64_t n) {
    uint64_t b = 0;
    for (FxSeekPoint &p : m.pts) {
        while (b < n && t[b].o_off + t[b].isize <= p.off) ++b;
        if (b == n) return;                      // (never: a point lies inside the text)
        p.c_off = t[b].c_off; p.o_off = t[b].o_off; p.c_len = t[b].c_len; p.blk = (uint32_t)b;
    }
}

// ... and from the entry table of a gzip map: the entry that holds the point's offset, c_off its byte, c_len the bytes that cover it
static inline void fx_seek_attach_gzip(FxSeekMap &m) {
    const uint64_t n = m.ent.size();
    m.n_blocks = n;
    uint64_t b = 0;
    for (FxSeekPoint &p : m.pts) {
        while (b < n && m.ent[b].off + m.ent[b].len <= p.off) ++b;
        if (b == n) return;                      // (never: a point lies inside the text)
        p.c_off = m.ent[b].bit >> 3; p.o_off = m.ent[b].off; p.c_len = (uint32_t)(fx_gz_cover_end(m, b) - p.c_off); p.blk = (uint32_t)b;
    }
}

// ... and from the entry table of a bzip2 map, in the same way
static inline void fx_seek_attach_bzip2(FxSeekMap &m) {
    const uint64_t n = m.bz_ent.size();
    m.n_blocks = n;
    uint64_t b = 0;
    for (FxSeekPoint &p : m.pts) {
        while (b < n && m.bz_ent[b].off + m.bz_ent[b].len <= p.off) ++b;
        if (b == n) return;                      // (never: a point lies inside the text)
        p.c_off = fx_bz_cover_begin(m, b); p.o_off = m.bz_ent[b].off; p.c_len = (uint32_t)(fx_bz_cover_end(m, b) - p.c_off); p.blk = (uint32_t)b;
    }
}

// one run: records [ord0, ord0 + n_rec), text [t0, t1).  BGZF: blocks [b0, b1), which are file bytes [f0, f1), the first of them
// starting at text offset o0; gzip: entries [b0, b1), file bytes [f0, f1) with the slack of the last; bzip2: entries [b0, b1), file bytes
// [f0, f1) -- two entries may share the byte in which one ends and the next starts; plain: f0 = t0, f1 = t1, no blocks
struct FxSeekRun { uint64_t ord0, n_rec, t0, t1, f0, f1, b0, b1, o0; };

struct FxSeekPlan {
    std::vector<FxSeekRun> runs;
    std::vector<uint32_t> sel;                   // the selection in ordinals of the sub-text
    uint64_t records = 0, text_bytes = 0, file_bytes = 0, blocks = 0;      // of the sub-text; a block or file byte shared by two runs counts once
};

// sel[0, k): strictly ascending, every ordinal below m.records (the caller has checked both)
static inline void fx_seek_plan(const FxSeekMap &m, const uint32_t *sel, uint64_t k, FxSeekPlan *p) {
    *p = FxSeekPlan();
    p->sel.resize((size_t)k);
    const uint64_t np = m.pts.size();
    std::vector<uint64_t> first, behind;         // a run as points [first, behind); behind == np: to the end of the text
    uint64_t i = 0;
    for (uint64_t j = 0; j < k; ++j) {
        while (i + 1 < np && m.pts[i + 1].ord <= sel[j]) ++i;       // the last point at or below the ordinal
        if (!first.empty() && i <= behind.back()) { if (i == behind.back()) ++behind.back(); }      // touches or lies inside: merged
        else { first.push_back(i); behind.push_back(i + 1); }
    }
    // the runs' fields, and the renumbering (the selection is ascending: one sweep)
    uint64_t at = 0, prev_b1 = 0, prev_f1 = 0;
    for (size_t r = 0; r < first.size(); ++r) {
        const FxSeekPoint &a = m.pts[first[r]];
        const bool to_end = behind[r] >= np;
        FxSeekRun run;
        run.ord0 = a.ord; run.t0 = a.off;
        run.n_rec = (to_end ? m.records : m.pts[behind[r]].ord) - a.ord;
        run.t1 = to_end ? m.text_bytes : m.pts[behind[r]].off;
        if (m.kind == FX_SEEK_BGZF || m.kind == FX_SEEK_GZIP || m.kind == FX_SEEK_BZIP2) {
            run.b0 = a.blk; run.f0 = a.c_off; run.o0 = a.o_off;
            if (to_end) { run.b1 = m.n_blocks; run.f1 = m.file_len; }
            else {
                const FxSeekPoint &z = m.pts[behind[r]];
                const bool whole = z.off == z.o_off;                // the run ends where z's block starts: that block is not the run's
                run.b1 = whole ? z.blk : (uint64_t)z.blk + 1;
                run.f1 = whole ? z.c_off : z.c_off + z.c_len;
            }
            if (m.kind == FX_SEEK_GZIP) run.f1 = fx_gz_cover_end(m, run.b1 - 1);     // (an entry's bytes reach past the next entry's first)
            if (m.kind == FX_SEEK_BZIP2) run.f1 = fx_bz_cover_end(m, run.b1 - 1);    // (... may share the next entry's first; the last ends in front of the stream's trailer)
            const uint64_t b_from = r && prev_b1 > run.b0 ? prev_b1 : run.b0, f_from = r && prev_f1 > run.f0 ? prev_f1 : run.f0;
            p->blocks += run.b1 > b_from ? run.b1 - b_from : 0;
            p->file_bytes += run.f1 > f_from ? run.f1 - f_from : 0;
            prev_b1 = run.b1; prev_f1 = run.f1;
        } else {
            run.b0 = run.b1 = 0; run.f0 = run.t0; run.f1 = run.t1; run.o0 = 0;
            p->file_bytes += run.t1 - run.t0;
        }
        p->runs.push_back(run);
        p->text_bytes += run.t1 - run.t0;
        for (; at < k && (uint64_t)sel[at] < run.ord0 + run.n_rec; ++at) p->sel[(size_t)at] = (uint32_t)(p->records + (sel[at] - run.ord0));
        p->records += run.n_rec;
    }
}
