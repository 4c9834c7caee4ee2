// host_fastx.inl -- read sets built on the device from FASTA / FASTQ text (k_fastx.h), from unaligned BAM
// (k_bam.h, host_bam.inl), from unaligned SAM (k_sam.h, host_sam.inl) and, without any text, from
// unaligned CRAM (k_cram.h, host_cram.inl): the text reaches HBM
// decompressed (BGZF chunks decoded into one block by the pipeline of host_inflate.inl, the gzip, bzip2, xz and (sliding: DESIGN section 26) Zstandard rounds appended device-to-device, plain input copied once), the
// record scan runs there, only identifiers and lengths come back, and lrge_hip_seqset_from_reads gathers the selected reads
// into dense ASCII for the device-source pack of host_seqset.inl.  Whatever the scan cannot prove is LRGE_ERR_UNPROVEN: the
// caller takes lrge_hip_read_records*, which parses the file or reports it with the reference's messages.  With
// LRGE_GPU_INGEST_WINDOWED FASTA / FASTQ text larger than option INGEST_WINDOW_BYTES passes through HBM in windows and only the
// bases stay (fx_window.h); with LRGE_GPU_INGEST_WINDOWED_ALN beside it so does unaligned BAM and SAM, BAM's
// bases staying packed.  lrge_hip_reads_census* and lrge_hip_reads_open_selected* pass FASTA / FASTQ text through
// the same windows and keep nothing, or only the records of a list of ordinals (FxKeepMode); lrge_hip_reads_census_map*
// leaves a seek map behind, with which lrge_hip_reads_open_mapped* brings only the runs of plain or BGZF input that hold chosen records
// (fx_seek.h, fx_src_seek_raw, fx_src_seek_bgzf); with the formats' own opt-in flags the four sampled calls take unaligned
// BAM, Zstandard (section 26), unaligned SAM through its windows and unaligned CRAM through fx_cram_sampled (section 27).
// With LRGE_GPU_INGEST_STREAM the four first-pass calls that take a path read plain, BGZF and gzip files in pinned pieces instead of whole
// (fx_input.h, fx_open_stream, fx_src_raw_stream, fx_src_bgzf_stream).
// Included into lrge_hip.hip.
// A call (lrge_hip_reads_open_mem) is one source (fx_src_raw, _bgzf, _gzip, _bzip2), which brings the text to the sink (FxSink) resident
// or through the windows of the sink's FxWinRun, and one record scan (fx_parse_kind), chosen by the sniff (fx_kind).

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "dev_keep.h"
#include "fx_input.h"
#include "fx_window.h"
#include "fx_seek.h"
#include "cram_round.h"

struct lrge_hip_reads {
    lrge_hip_ctx *ctx = nullptr;
    u8 *d_text = nullptr; u64 n_text = 0;       // the decompressed text (FX_PAD bytes of slack behind it)
    FxRec *d_recs = nullptr; u64 n = 0;
    int fmt = FX_FMT_EMPTY;
    std::vector<u32> seq_len;
    std::vector<u64> name_off;                  // [n + 1]
    std::string names;
    float ms[4] = {0, 0, 0, 0};                 // text to HBM, record scan, identifiers and lengths to the host, the whole call
    BamStats bam = {0, 0, 0, 0, 0, 0};          // fmt == FX_FMT_BAM: the counts of the record scan, summed over the windows (lrge_hip_reads_bam_stats)
    u64 text_bytes = 0;                         // the decompressed text that was scanned (windowed: d_text holds its bases only, BAM's packed)
    FxWinStats win = {0, 0, 0, 0};              // lrge_hip_reads_window_stats
    bool is_cram = false;                       // opened from unaligned CRAM (host_cram.inl): d_text is a base store, as a windowed FASTA handle's
    CramStats cram;                             // lrge_hip_reads_cram_stats
    uint64_t zs_slide[4] = {0, 0, 0, 0};        // lrge_hip_reads_zstd_stats: the sliding Zstandard rounds of the call (zeros: it did not slide)
    FxSelStats sel = {0, 0, 0, 0};              // lrge_hip_reads_select_stats: the pass of lrge_hip_reads_open_selected* (a window: what it adds)
    u64 seek[4] = {0, 0, 0, 0};                 // lrge_hip_reads_seek_stats: runs, text bytes brought, file bytes read, BGZF blocks or gzip / bzip2 entries decoded (lrge_hip_reads_open_mapped*)
};

// the seek map of a census (fx_seek.h), as the caller holds it
struct lrge_hip_read_map { FxSeekMap m; };

static double fx_now_ms() { return DevPool::now_ms(); }

static u64 ingest_cap(lrge_hip_ctx *ctx) { return ctx->opt_u64("INGEST_MAX_BYTES", dev_budget(ctx)); }

// ---- what a call is refused with: every text has its one site here ----
static int fx_unproven(lrge_hip_ctx *ctx, const char *what) { LRGE_SET_ERR(ctx, "reads_open: not proven on the device (%s)", what); return LRGE_ERR_UNPROVEN; }
static int fx_verdict_rc(lrge_hip_ctx *ctx, u32 verdict, const char *what) {
    if (verdict & FX_UNPROVEN) return fx_unproven(ctx, what);
    LRGE_SET_ERR(ctx, "reads_open: 2^32 records or a sequence of 2^32 bases (%s)", what);
    return LRGE_ERR_TOO_MANY;
}
// the sampled calls: a container or a format they were not asked for by its flags (also: ", not Zstandard input")
static int fx_fastx_only(lrge_hip_ctx *ctx, const char *also = "") { ctx->err = std::string("reads_open_selected: selected ingest takes FASTA / FASTQ only") + also; return LRGE_ERR_UNPROVEN; }
static int fx_sel_checked(lrge_hip_ctx *ctx, const u32 *sel, u64 k) {
    if ((!k || sel) && fx_sel_ascending(sel, k)) return LRGE_OK;
    ctx->err = "reads_open_selected: the ordinals are not strictly ascending";
    return LRGE_ERR_INVALID;
}
static int fx_ordinal_rc(lrge_hip_ctx *ctx, u32 ordinal, u64 records) { LRGE_SET_ERR(ctx, "reads_open_selected: ordinal %u of %llu records", ordinal, (unsigned long long)records); return LRGE_ERR_INVALID; }
static int fx_read_failed(lrge_hip_ctx *ctx) { ctx->err = "reads_open_mapped: the file could not be read"; return LRGE_ERR_IO; }
// the streamed first pass
static int fx_open_failed(lrge_hip_ctx *ctx, const char *path) { LRGE_SET_ERR(ctx, "IO error: %s: cannot be opened for reading by range", path); return LRGE_ERR_IO; }
static int fx_stream_read_failed(lrge_hip_ctx *ctx) { ctx->err = "reads_open: the file could not be read"; return LRGE_ERR_IO; }
static int fx_stream_needs_windowed(lrge_hip_ctx *ctx) { ctx->err = "reads_open: LRGE_GPU_INGEST_STREAM without LRGE_GPU_INGEST_WINDOWED"; return LRGE_ERR_INVALID; }
static int fx_stream_needs_aln(lrge_hip_ctx *ctx) { ctx->err = "reads_open: BAM or SAM text under LRGE_GPU_INGEST_STREAM without LRGE_GPU_INGEST_WINDOWED_ALN"; return LRGE_ERR_UNPROVEN; }
static int fx_stream_not_bgzf(lrge_hip_ctx *ctx, u64 off) {
    LRGE_SET_ERR(ctx, "reads_open: no BGZF block at file offset %llu behind BGZF blocks: open without LRGE_GPU_INGEST_STREAM", (unsigned long long)off);
    return LRGE_ERR_UNPROVEN;
}
static int fx_map_other(lrge_hip_ctx *ctx) { ctx->err = "reads_open_mapped: the map is of another input"; return LRGE_ERR_INVALID; }
static int fx_map_misfit(lrge_hip_ctx *ctx, const char *what) { LRGE_SET_ERR(ctx, "reads_open_mapped: the map does not fit the input (%s)", what); return LRGE_ERR_UNPROVEN; }
static int fx_map_range(lrge_hip_ctx *ctx) { ctx->err = "reads_open_mapped: a file range does not hold the blocks of the map"; return LRGE_ERR_INVALID; }

// the record table of n records in R->d_recs
static int fx_alloc_recs(lrge_hip_ctx *ctx, lrge_hip_reads *R, u64 n) {
    hipError_t e = hipSuccess;
    if ((R->d_recs = (FxRec *)ctx->pool.alloc((size_t)n * sizeof(FxRec), &e))) return LRGE_OK;
    LRGE_SET_ERR(ctx, "reads_open: record table: %s", hipGetErrorString(e));
    return LRGE_ERR_DEVICE;
}
// ... the text block of `bytes` bytes in R->d_text, FX_PAD bytes of slack behind it
static int fx_alloc_text(lrge_hip_ctx *ctx, lrge_hip_reads *R, u64 bytes) {
    hipError_t e = hipSuccess;
    R->n_text = bytes;
    if ((R->d_text = (u8 *)ctx->pool.alloc((size_t)bytes + FX_PAD, &e))) return LRGE_OK;
    LRGE_SET_ERR(ctx, "reads_open: device allocation of %llu bytes failed: %s", (unsigned long long)bytes, hipGetErrorString(e));
    return LRGE_ERR_DEVICE;
}
// ... and a table made on the host -- the records of a base store -- copied into it (one record is allocated at least)
static int fx_upload_recs(lrge_hip_ctx *ctx, lrge_hip_reads *R, const std::vector<FxRec> &tab) {
    const int rc = fx_alloc_recs(ctx, R, std::max<u64>(1, tab.size()));
    if (rc) return rc;
    if (!tab.empty()) HIPCHK(ctx, hipMemcpyAsync(R->d_recs, tab.data(), tab.size() * sizeof(FxRec), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return LRGE_OK;
}

// the bytes a record of `len` bases takes in a base store: BAM's stay packed, two to a byte, and a record starts on a byte
static u64 fx_store_span(u64 len, bool packed) { return packed ? (len + 1) / 2 : len; }

// behind the kernel that fills the record table: the flag words come back in one copy -- f[0] the verdict bits (low word), f[1] the identifier
// bytes and, for a run that does not keep all (bases), f[2] the sum of d_seq_len, which k_fx_bases adds up first: no synchronisation of its own
static int fx_flags_back(lrge_hip_ctx *ctx, bool bases, u64 *d_flags, const u32 *d_seq_len, u64 n_rec, u64 f[3]) {
    f[0] = f[1] = f[2] = 0;
    if (bases && n_rec) {
        hipLaunchKernelGGL(k_fx_bases, dim3(std::min<u32>((u32)div_up(n_rec, FX_THREADS), (u32)ctx->n_cu * 8)), dim3(FX_THREADS), 0, ctx->stream, d_seq_len, n_rec,
                           (unsigned long long *)(d_flags + 2));
        KCHK(ctx);
    }
    HIPCHK(ctx, ctx->d2h(f, d_flags, bases ? 24 : 16, ctx->stream));
    HIPCHK(ctx, ctx->d2h_sync(ctx->stream));
    return LRGE_OK;
}

// identifiers and lengths to the host, behind a record scan that left the table in R->d_recs, the lengths in d_seq_len /
// d_name_len and the identifiers' bytes in name_bytes: k_fx_names compacts the identifiers, three copies bring the tables down
static int fx_tables_to_host(lrge_hip_ctx *ctx, lrge_hip_reads *R, Scratch &sc, u64 n_rec, const u32 *d_seq_len, const u32 *d_name_len, u64 name_bytes) {
    const double t_scan = fx_now_ms();
    hipStream_t st = ctx->stream;
    int rc;
    ALLOC_OR_FAIL(d_name_dst, sc, u32, n_rec);
    if ((rc = scan_exclusive_u32(ctx, sc, d_name_len, d_name_dst, n_rec, nullptr))) return rc;
    ALLOC_OR_FAIL(d_names, sc, u8, std::max<u64>(1, name_bytes));
    hipLaunchKernelGGL(k_fx_names, dim3((u32)div_up(n_rec, FX_THREADS)), dim3(FX_THREADS), 0, st, (const u8 *)R->d_text, (const FxRec *)R->d_recs, (const u32 *)d_name_dst, n_rec,
                       d_names);
    KCHK(ctx);
    R->n = n_rec;
    R->seq_len.resize((size_t)n_rec);
    std::vector<u32> name_len((size_t)n_rec);
    R->names.resize((size_t)name_bytes);
    HIPCHK(ctx, hipMemcpyAsync(R->seq_len.data(), d_seq_len, (size_t)n_rec * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(name_len.data(), d_name_len, (size_t)n_rec * 4, hipMemcpyDeviceToHost, st));
    if (name_bytes) HIPCHK(ctx, hipMemcpyAsync(&R->names[0], d_names, (size_t)name_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    R->name_off.resize((size_t)n_rec + 1);
    u64 o = 0;
    for (u64 i = 0; i < n_rec; ++i) { R->name_off[i] = o; o += name_len[i]; }
    R->name_off[n_rec] = o;
    R->ms[2] = (float)(fx_now_ms() - t_scan);
    return LRGE_OK;
}

// ---- the sniff: which record scan a text takes ----
// by its first min(4, n) bytes: FX_FMT_BAM and FX_FMT_SAM by their magic, when the caller asked for them; else FX_FMT_EMPTY --
// FASTA or FASTQ, which the record scan tells apart
static int fx_sniff(int flags, const u8 *head, u64 n) {
    if ((flags & LRGE_GPU_INGEST_BAM) && n >= 4 && head[0] == 'B' && head[1] == 'A' && head[2] == 'M' && head[3] == 1) return FX_FMT_BAM;
    return (flags & LRGE_GPU_INGEST_SAM) && n >= 3 && sam_sniff(head, n) ? FX_FMT_SAM : FX_FMT_EMPTY;
}

// the container of a file by its first min(6, n) bytes.  FX_BOX_XZ: the five bytes that name xz to a caller who did not ask for it;
// the device decoder is given the file only where the sixth is the magic's 0 as well (xz_whole)
enum FxBox { FX_BOX_OTHER, FX_BOX_CRAM, FX_BOX_GZIP, FX_BOX_BZIP2, FX_BOX_ZSTD, FX_BOX_XZ };
static FxBox fx_container(const u8 *d, u64 n, bool *xz_whole = nullptr) {
    const auto is = [&](const char *magic, u64 k) { return n >= k && !memcmp(d, magic, (size_t)k); };
    if (xz_whole) *xz_whole = is("\xfd" "7zXZ\0", 6);
    return is("CRAM", 4) ? FX_BOX_CRAM : is("\x1f\x8b", 2) ? FX_BOX_GZIP : is("BZ", 2) ? FX_BOX_BZIP2 : is("\x28\xb5\x2f\xfd", 4) ? FX_BOX_ZSTD : is("\xfd" "7zXZ", 5) ? FX_BOX_XZ : FX_BOX_OTHER;
}

// the kind of a text of n bytes, after obtaining those bytes: the file's own when they are the text (host), else four bytes
// copied from the block d_text.  Nothing is copied for a caller who asked for neither BAM nor SAM, or for a text below either magic
static int fx_kind(lrge_hip_ctx *ctx, int flags, const u8 *host, const u8 *d_text, u64 n, int *kind) {
    *kind = FX_FMT_EMPTY;
    if (!(flags & (LRGE_GPU_INGEST_BAM | LRGE_GPU_INGEST_SAM)) || n < 3) return LRGE_OK;
    u8 head[4] = {0, 0, 0, 0};
    const size_t k = (size_t)std::min<u64>(4, n);
    if (host) memcpy(head, host, k);
    else { HIPCHK(ctx, hipMemcpyAsync(head, d_text, k, hipMemcpyDeviceToHost, ctx->stream)); HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); }
    *kind = fx_sniff(flags, head, n);
    return LRGE_OK;
}

// BAM and SAM stay resident unless the caller asked for their windows as well
static bool fx_kind_windowed(int flags, int kind) { return kind == FX_FMT_EMPTY || (flags & LRGE_GPU_INGEST_WINDOWED_ALN); }

// the census and the selected open take FASTA / FASTQ, whatever flags came with the call: the sniff of the text's first bytes.
// With LRGE_GPU_INGEST_SELECT_ALN beside LRGE_GPU_INGEST_BAM the magic of BAM makes the run a BAM run, through
// the windows whatever LRGE_GPU_INGEST_WINDOWED / _WINDOWED_ALN say, as FASTA / FASTQ text is
static bool fx_select_aln(int flags) { return (flags & LRGE_GPU_INGEST_BAM) && (flags & LRGE_GPU_INGEST_SELECT_ALN); }
// ... and with LRGE_GPU_INGEST_SELECT_SAM beside LRGE_GPU_INGEST_SAM text that sam_sniff takes makes it a SAM run
static bool fx_select_sam(int flags) { return (flags & LRGE_GPU_INGEST_SAM) && (flags & LRGE_GPU_INGEST_SELECT_SAM); }

// ---- windowed ingest: the device backend of fx_window.h ----
struct FxWinDev;
// the scan of one window (fx_parse_kind): up to its cut (left in `cut`; 0: there is none yet) unless `end`
struct FxWinScan { FxWinDev *dev; bool first, end; u64 cut; };
// the record scan of R->d_text by its kind (fx_kind): bam_parse_device, sam_parse_device or fx_parse_device
static int fx_parse_kind(lrge_hip_ctx *ctx, lrge_hip_reads *R, int kind, FxWinScan *w = nullptr);

struct FxWinDev {
    lrge_hip_ctx *ctx;
    lrge_hip_reads *R;                          // collects the identifiers and lengths of every window
    int flags;
    u64 cap;                                    // INGEST_MAX_BYTES: the block and the store together
    u64 aside = 0;                              // ... and what a decoder holds beside them under the same cap (the sliding Zstandard work block)
    DevKeep *blk = nullptr;                     // the block the text is appended to (a decoder's own, or one of the call)
    DevKeep store;                              // the bases of the records flushed so far, dense, in file order (BAM: packed, a record starts on a byte)
    int kind = FX_FMT_EMPTY;                    // FX_FMT_BAM / FX_FMT_SAM: the run is that format's, by the sniff of its first bytes; else FASTA / FASTQ
    u64 through = 0;                            // text bytes cut off the block so far
    double ms_scan = 0, ms_names = 0;
    int rc = LRGE_OK;                           // what stopped the windows, with its message (a decoder's hook can only say "stop")
    std::string msg;
    // what the run keeps (fx_window.h).  FX_KEEP_SEL: sel[0, k), strictly ascending, on the host and -- uploaded
    // once -- in d_sel; sel[0, at) lay in the windows flushed so far, whose records are R->sel.seen
    FxKeepMode mode = FX_KEEP_ALL;
    const u32 *sel = nullptr;
    u32 *d_sel = nullptr;
    u64 k = 0, at = 0;
    FxSeekMap *map = nullptr;                   // a census that was asked for a seek map (fx_seek.h): seek_window adds every window's points
    bool mapped = false;                        // the text is the sub-text of a mapped open: whole records of a text the census proved, never sniffed
    bool scan_refused = false;                  // a window was not proven by the record scan or the driver (not: the budget) -- what a mapped open reports as a map that does not fit
    FxWinDev(lrge_hip_ctx *c, lrge_hip_reads *r, int f, u64 cap_) : ctx(c), R(r), flags(f), cap(cap_), store(c) {
        store.keep_slack = FX_PAD; store.keep_floor = 0;     // (block and store share one budget: neither takes more than it needs or doubles to)
        R->name_off.assign(1, 0);
    }
    ~FxWinDev() { ctx->pool.release(d_sel); }
    int select(FxKeepMode m, const u32 *s, u64 n) {
        mode = m; sel = s; k = n;
        if (m != FX_KEEP_SEL || !n) return LRGE_OK;
        hipError_t e = hipSuccess;
        if (!(d_sel = (u32 *)ctx->pool.alloc((size_t)n * 4, &e))) { LRGE_SET_ERR(ctx, "reads_open_selected: selection: %s", hipGetErrorString(e)); return LRGE_ERR_DEVICE; }
        HIPCHK(ctx, hipMemcpyAsync(d_sel, s, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));            // (the caller's list is pageable: its copy is done)
        return LRGE_OK;
    }
    u64 len() const { return blk->keep_len; }
    int unproven(const char *what) { scan_refused = true; return fx_unproven(ctx, what); }
    u32 lead() const { return kind == FX_FMT_BAM ? FX_LEAD_BAM : kind == FX_FMT_SAM ? FX_LEAD_SAM : FX_LEAD_TEXT; }      // where a record starts (fx_rec_start)
    int selected_format() {
        if (mapped) return LRGE_OK;             // (a run may start with a read named HD.., SQ.. or RG..: fx_win_census; the kind is the map's)
        u8 head[4] = {0, 0, 0, 0};
        const u64 n = blk->keep_len;
        if (n) { HIPCHK(ctx, hipMemcpyAsync(head, blk->keep, (size_t)std::min<u64>(4, n), hipMemcpyDeviceToHost, ctx->stream)); HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); }
        if (fx_select_aln(flags) && fx_sniff(LRGE_GPU_INGEST_BAM, head, n) == FX_FMT_BAM) { kind = FX_FMT_BAM; return LRGE_OK; }
        if (fx_select_sam(flags) && fx_sniff(LRGE_GPU_INGEST_SAM, head, n) == FX_FMT_SAM) { kind = FX_FMT_SAM; return LRGE_OK; }
        if (fx_sniff(LRGE_GPU_INGEST_BAM | LRGE_GPU_INGEST_SAM, head, n) == FX_FMT_EMPTY && !(n >= 4 && !memcmp(head, "CRAM", 4))) return LRGE_OK;
        return fx_fastx_only(ctx);
    }
    // the sniff of the first window makes the run a BAM or SAM run: a later window is never sniffed.  BAM and SAM that stay
    // resident turn the windows off: the block takes back the growth rule a resident text has without the flag (attach() had made it
    // a window's; keep_flush stays: it is running, and the driver returns at once from now on).  (Plain and BGZF input is sniffed
    // before a window is set up as well, FxSink::windowed; the round decoders' first bytes arrive with a round.)
    u64 was_hint = 0, was_floor = 0, was_grow = 2;
    int resident_format(bool *yes) {
        *yes = false;
        if (mode != FX_KEEP_ALL) return selected_format();
        const int rc = fx_kind(ctx, flags, nullptr, blk->keep, blk->keep_len, &kind);
        if (rc) return rc;
        if ((*yes = !fx_kind_windowed(flags, kind))) { blk->keep_hint = was_hint; blk->keep_floor = was_floor; blk->keep_grow = was_grow; blk->keep_max = cap - aside; }
        return LRGE_OK;
    }
    int flush(bool first, bool end, u64 *cut, int *fmt) {
        lrge_hip_reads W;                       // the window as a text of its own; the block stays the decoder's
        W.ctx = ctx; W.d_text = blk->keep; W.n_text = blk->keep_len;
        FxWinScan w = {this, first && !mapped, end, 0};
        const double t0 = fx_now_ms();
        const int prc = fx_parse_kind(ctx, &W, kind, &w);
        ctx->pool.release(W.d_recs);
        ms_names += W.ms[2]; ms_scan += fx_now_ms() - t0 - W.ms[2];
        if (prc == LRGE_ERR_UNPROVEN && !store.keep_over) scan_refused = true;      // (the scan's verdict; the store's budget is the other refusal a window has)
        if (prc) return prc;
        *cut = end ? W.n_text : w.cut; *fmt = W.fmt;
        if (*cut) bam_stats_add(R->bam, W.bam);
        if (*cut && mode != FX_KEEP_ALL) {        // (W.n, W.names and W.seq_len: the chosen records of the window, W.sel: all of them)
            if ((R->sel.seen + W.sel.seen) >> 32) return fx_verdict_rc(ctx, FX_UNPROVEN, "2^32 records or more");
            R->sel.seen += W.sel.seen; R->sel.bases_seen += W.sel.bases_seen;
            R->sel.kept += W.sel.kept; R->sel.bases_kept += W.sel.bases_kept;
            at += W.sel.kept;
        }
        if (!*cut || !W.n) return LRGE_OK;
        if ((R->n + W.n) >> 32) return fx_verdict_rc(ctx, FX_UNPROVEN, "2^32 records or more");
        if ((R->names.size() + W.names.size()) >> 32) return fx_verdict_rc(ctx, FX_UNPROVEN, "4 GiB of identifiers or more");
        const u64 names_at = R->names.size();
        R->names += W.names;
        R->seq_len.insert(R->seq_len.end(), W.seq_len.begin(), W.seq_len.end());
        for (u64 i = 1; i <= W.n; ++i) R->name_off.push_back(names_at + W.name_off[i]);
        R->n += W.n;
        return LRGE_OK;
    }
    // room for `sum` more bytes in the store, within the budget it shares with the block
    int store_room(u64 sum) {
        // the store doubles while that leaves the block room to double as well; close to the cap it grows by an eighth
        const u64 lim = cap - aside;
        const u64 need = store.keep_len + sum, room = lim > blk->keep_cap ? lim - blk->keep_cap : 0, soft = lim > 2 * blk->keep_cap ? lim - 2 * blk->keep_cap : 0;
        store.keep_max = need <= soft ? soft : std::min<u64>(room, need + need / 8);
        if (!store.keep_reserve(sum)) {
            if (store.keep_over) { LRGE_SET_ERR(ctx, "reads_open: bases and window above INGEST_MAX_BYTES (%llu)", (unsigned long long)cap); return LRGE_ERR_UNPROVEN; }
            LRGE_SET_ERR(ctx, "reads_open: base store: %s", hipGetErrorString(store.e));
            return LRGE_ERR_DEVICE;
        }
        blk->keep_max = lim > store.keep_cap ? lim - store.keep_cap : 0;
        return LRGE_OK;
    }
    // A window of a census that leaves a seek map, behind k_fx_records, k_bam_records or k_sam_records: k_fx_seek finds the first record start of every cell of the
    // window's prefix [0, n_use), the slots (record index and window offset, 8 bytes a cell) come down in one copy, and the point
    // rule of fx_seek.h takes those that hold a record.  The window's records are R->sel.seen onwards, its bytes `through` onwards
    int seek_window(Scratch &sc, const lrge_hip_reads *W, u64 n_rec, u64 n_use) {
        if (!n_rec) return LRGE_OK;
        const u64 S = map->stride, cell0 = through / S, n_cells = (through + n_use - 1) / S - cell0 + 1;
        ALLOC_OR_FAIL(d_slot, sc, u32, 2 * n_cells);
        HIPCHK(ctx, hipMemsetAsync(d_slot, 0xFF, (size_t)n_cells * 8, ctx->stream));
        hipLaunchKernelGGL(k_fx_seek, dim3((u32)div_up(n_rec, FX_THREADS)), dim3(FX_THREADS), 0, ctx->stream, (const FxRec *)W->d_recs, n_rec, through, S, cell0, n_cells,
                           lead(), d_slot);
        KCHK(ctx);
        std::vector<u32> slot((size_t)n_cells * 2);
        HIPCHK(ctx, hipMemcpyAsync(slot.data(), d_slot, (size_t)n_cells * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        for (u64 c = 0; c < n_cells; ++c)
            if (slot[c] != FX_SEEK_NONE) fx_seek_add(*map, R->sel.seen + slot[c], through + slot[n_cells + c]);
        return LRGE_OK;
    }
    // d_dst: where m records of d_len bases start behind the store's end -- the scan of their spans (fx_store_span; packed: k_bam_spans', in place)
    int store_offsets(Scratch &sc, bool packed, const u32 *d_len, u64 m, u32 *d_dst) {
        if (packed) {
            hipLaunchKernelGGL(k_bam_spans, dim3((u32)div_up(m, 256)), dim3(256), 0, ctx->stream, d_len, m, d_dst);
            KCHK(ctx);
            d_len = d_dst;
        }
        return scan_exclusive_u32(ctx, sc, d_len, d_dst, m, nullptr);
    }
    // A window of a run that does not keep all (FX_KEEP_NONE, FX_KEEP_SEL), behind k_fx_records: W.d_recs and the lengths of its
    // n_rec records are on the device, `bases` is their sum.  The slice of the selection that falls into the window is found
    // here; a window without a chosen record costs nothing more.  Else k_fx_pick gathers the chosen lengths, which come down and
    // are scanned, and k_fx_keep copies identifiers and bases.  W leaves as a window of the chosen records only.  A BAM run
    // (behind k_bam_records): the store takes the packed bytes, so k_bam_spans turns the picked lengths into the spans that are
    // scanned, and k_bam_keep copies; bases_kept still counts bases
    int keep_window(Scratch &sc, lrge_hip_reads *W, const u32 *d_seq_len, const u32 *d_name_len, u64 n_rec, u64 n_use, u64 bases) {
        W->sel = FxSelStats{n_rec, 0, bases, 0};
        W->n = 0;
        const u64 r0 = R->sel.seen, a = at, b = mode == FX_KEEP_SEL ? fx_sel_slice(sel, k, a, r0, n_rec) : a, m = b - a;
        if (!m) return LRGE_OK;
        const double t0 = fx_now_ms();
        hipStream_t st = ctx->stream;
        int rc;
        ALLOC_OR_FAIL(d_pick_seq, sc, u32, m);
        ALLOC_OR_FAIL(d_pick_name, sc, u32, m);
        hipLaunchKernelGGL(k_fx_pick, dim3((u32)div_up(m, FX_THREADS)), dim3(FX_THREADS), 0, st, (const u32 *)(d_sel + a), (u32)r0, m, d_seq_len, d_name_len, d_pick_seq, d_pick_name);
        KCHK(ctx);
        std::vector<u32> name_len((size_t)m);
        W->seq_len.resize((size_t)m);
        HIPCHK(ctx, hipMemcpyAsync(W->seq_len.data(), d_pick_seq, (size_t)m * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(name_len.data(), d_pick_name, (size_t)m * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        W->name_off.assign(1, 0);
        const bool packed = kind == FX_FMT_BAM;
        u64 sum = 0, kept = 0, name_bytes = 0;                     // sum: the bytes the store takes
        for (u64 j = 0; j < m; ++j) {
            const u64 l = W->seq_len[j];
            kept += l; sum += fx_store_span(l, packed); name_bytes += name_len[j]; W->name_off.push_back(name_bytes);
        }
        if (kept > bases || sum >> 32 || name_bytes >> 32) return fx_verdict_rc(ctx, FX_UNPROVEN, "a window of 2^32 bytes or more");      // (never: the window is below that)
        if ((rc = store_room(sum))) return rc;
        ALLOC_OR_FAIL(d_dst, sc, u32, m);
        ALLOC_OR_FAIL(d_name_dst, sc, u32, m);
        ALLOC_OR_FAIL(d_names, sc, u8, std::max<u64>(1, name_bytes));
        if ((rc = store_offsets(sc, packed, d_pick_seq, m, d_dst)) || (rc = scan_exclusive_u32(ctx, sc, d_pick_name, d_name_dst, m, nullptr))) return rc;
        const dim3 grid((u32)std::min<u64>(m, (u64)ctx->n_cu * 32));
        if (packed)
            hipLaunchKernelGGL(k_bam_keep, grid, dim3(64), 0, st, (const u8 *)W->d_text, (const FxRec *)W->d_recs, (const u32 *)(d_sel + a), (u32)r0, m, (const u32 *)d_dst,
                               (const u32 *)d_name_dst, store.keep + store.keep_len, d_names);
        else
            hipLaunchKernelGGL(k_fx_keep, grid, dim3(64), 0, st, (const u8 *)W->d_text, n_use, (const FxRec *)W->d_recs, (const u32 *)(d_sel + a), (u32)r0,
                               m, (const u32 *)d_dst, (const u32 *)d_name_dst, store.keep + store.keep_len, d_names);
        KCHK(ctx);
        W->names.resize((size_t)name_bytes);
        if (name_bytes) HIPCHK(ctx, hipMemcpyAsync(&W->names[0], d_names, (size_t)name_bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));                     // (also: the scratch and the table go back to the pool, which other streams draw from)
        store.keep_len += sum;
        W->n = m; W->sel.kept = m; W->sel.bases_kept = kept;
        W->ms[2] = (float)(fx_now_ms() - t0);
        return LRGE_OK;
    }
    // the bases of the window's records (table W.d_recs, lengths d_seq_len) behind those of the earlier windows; BAM: the packed
    // bytes, (seq_len + 1) / 2 a record
    int store_window(Scratch &sc, const lrge_hip_reads &W, const u32 *d_seq_len, u64 n_use) {
        const bool packed = W.fmt == FX_FMT_BAM;
        u64 sum = 0;
        for (u32 l : W.seq_len) sum += fx_store_span(l, packed);
        if (sum >> 32) return fx_verdict_rc(ctx, FX_UNPROVEN, "a window of 2^32 bytes or more");      // (never: the window is below that)
        const int rrc = store_room(sum);
        if (rrc) return rrc;
        if (W.n) {
            ALLOC_OR_FAIL(d_dst, sc, u32, W.n);
            const dim3 grid((u32)std::min<u64>(W.n, (u64)ctx->n_cu * 32));
            const int src = store_offsets(sc, packed, d_seq_len, W.n, d_dst);
            if (src) return src;
            if (packed)
                hipLaunchKernelGGL(k_bam_store, grid, dim3(64), 0, ctx->stream, (const u8 *)W.d_text, (const FxRec *)W.d_recs, (const u32 *)d_dst, W.n, store.keep + store.keep_len);
            else
                hipLaunchKernelGGL(k_fx_store, grid, dim3(64), 0, ctx->stream, (const u8 *)W.d_text, n_use, (const FxRec *)W.d_recs, (const u32 *)d_dst, W.n,
                                   store.keep + store.keep_len);
            KCHK(ctx);
        }
        store.keep_len += sum;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));            // (the scratch and the table go back to the pool, which other streams draw from)
        return LRGE_OK;
    }
    // [cut, len) to the front, in one copy: in place when the tail is no longer than the cut (source and destination are apart);
    // a longer tail -- a small record in front of a large one -- goes to a second block of the same size, which becomes the block
    int carry(u64 cut) {
        const u64 tail = blk->keep_len - cut;
        if (tail <= cut) {
            if (tail) HIPCHK(ctx, hipMemcpyAsync(blk->keep, blk->keep + cut, (size_t)tail, hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            hipError_t e = hipSuccess;
            u8 *p = (u8 *)ctx->pool.alloc((size_t)(blk->keep_cap + blk->keep_slack), &e);
            if (!p) { LRGE_SET_ERR(ctx, "reads_open: second block for the carried tail: %s", hipGetErrorString(e)); return LRGE_ERR_DEVICE; }
            const hipError_t ce = hipMemcpyAsync(p, blk->keep + cut, (size_t)tail, hipMemcpyDeviceToDevice, ctx->stream);
            const hipError_t se = ce == hipSuccess ? hipStreamSynchronize(ctx->stream) : ce;    // (the old block goes back to the pool, which other streams draw from)
            if (se != hipSuccess) { ctx->pool.release(p); HIPCHK(ctx, se); }
            ctx->pool.release(blk->keep);
            blk->keep = p;
        }
        blk->keep_len = tail; through += cut;
        return LRGE_OK;
    }
};

// one windowed call: the driver over its backend, attached to the block of whichever source delivers the text
struct FxWinRun {
    FxWinDev dev;
    FxWindow<FxWinDev> win;
    FxWinRun(lrge_hip_ctx *c, lrge_hip_reads *r, int flags, u64 cap, u64 window) : dev(c, r, flags, cap), win(dev, window) {}
    // behind every append to `b`; false: stop (dev.rc and dev.msg say why)
    bool appended() {
        if ((dev.rc = win.step(false))) dev.msg = dev.ctx->err;
        return dev.rc == LRGE_OK;
    }
    // b: the block as a resident text would have it.  While the windows are on, what it holds is bounded by window, piece and
    // record: it starts at two windows and grows to what it needs, the budget is shared with the store
    void attach(DevKeep *b) {
        dev.blk = b;
        dev.was_hint = b->keep_hint; dev.was_floor = b->keep_floor; dev.was_grow = b->keep_grow;
        b->keep_hint = std::min<u64>(b->keep_hint ? b->keep_hint : ~(u64)0, std::min<u64>(dev.cap, 2 * win.window));
        b->keep_floor = 0; b->keep_grow = 1;
        b->keep_flush = [this] { return appended(); };
    }
    int stopped() { if (dev.rc) dev.ctx->err = dev.msg; return dev.rc; }
    // the input is over and windows were flushed: what is left in the block (the handle's text so far, the run's now) is the
    // last window; the store becomes the handle's text, with a record table of its own
    int finish() {
        lrge_hip_ctx *ctx = dev.ctx;
        lrge_hip_reads *R = dev.R;
        DevKeep last(ctx);
        const u64 n_text = last.keep_len = last.keep_cap = R->n_text;
        last.keep = R->d_text; R->d_text = nullptr; R->n_text = 0;
        dev.blk = &last;
        int rc = win.step(true);
        if (rc) return rc;
        if (dev.mode == FX_KEEP_SEL && dev.at < dev.k) return fx_ordinal_rc(ctx, dev.sel[dev.at], R->sel.seen);      // (the selection is ascending: the first ordinal left over names the fault)
        if (!dev.store.keep && !dev.store.keep_reserve(0)) { LRGE_SET_ERR(ctx, "reads_open: device allocation failed"); return LRGE_ERR_DEVICE; }
        std::vector<FxRec> tab((size_t)R->n);
        const bool packed = win.fmt == FX_FMT_BAM;              // (the gather of BAM reads its records' spans as it reads the text)
        u64 o = 0;
        for (u64 i = 0; i < R->n; ++i) {
            const u64 span = fx_store_span(R->seq_len[i], packed);
            tab[i] = FxRec{0, o, span, (u32)(R->name_off[i + 1] - R->name_off[i]), R->seq_len[i]};
            o += span;
        }
        if ((rc = fx_upload_recs(ctx, R, tab))) return rc;
        R->d_text = dev.store.keep; R->n_text = dev.store.keep_len; dev.store.keep = nullptr;
        R->fmt = win.fmt;
        R->text_bytes = dev.through + n_text;
        R->win = win.st; R->win.bases = R->n_text;
        R->ms[1] = (float)dev.ms_scan; R->ms[2] = (float)dev.ms_names;
        return LRGE_OK;
    }
};

// does the scan serve a run that does not keep all (the census and the selected open)?  Its windows' bases are counted
static bool fx_scan_selects(const FxWinScan *w) { return w && w->dev->mode != FX_KEEP_ALL; }
// The tail of the three record scans, which left the table of the prefix [0, n_use) in R->d_recs, the lengths of its n_rec records in d_seq_len /
// d_name_len and the flag words in f (fx_flags_back; outside: what a record outside the strict form is refused with).  A run that does not keep
// all: the seek map takes the window's points, keep_window the chosen records.  Else the tables go to the host, a window's (w) bases to the store
static int fx_scan_tail(lrge_hip_ctx *ctx, lrge_hip_reads *R, Scratch &sc, FxWinScan *w, const u64 f[3], const char *outside, const u32 *d_seq_len, const u32 *d_name_len, u64 n_rec,
                        u64 n_use) {
    if ((u32)f[0]) return fx_verdict_rc(ctx, (u32)f[0], outside);
    if (f[1] >> 32) return fx_verdict_rc(ctx, FX_UNPROVEN, "4 GiB of identifiers or more");
    int rc;
    if (fx_scan_selects(w)) {
        if (w->dev->map && (rc = w->dev->seek_window(sc, R, n_rec, n_use))) return rc;
        return w->dev->keep_window(sc, R, d_seq_len, d_name_len, n_rec, n_use, f[2]);
    }
    if ((rc = fx_tables_to_host(ctx, R, sc, n_rec, d_seq_len, d_name_len, f[1])) || !w) return rc;
    return w->dev->store_window(sc, *R, d_seq_len, n_use);
}

// the prologue of the scans that work on lines (FASTA / FASTQ, SAM): the census of every tile of t[0, n) and its summary
struct FxTiles { u64 n_tiles; u32 *c_lf, *c_rem, *c_hdr; FxSummary hs; };
static int fx_census_device(lrge_hip_ctx *ctx, Scratch &sc, const u8 *t, u64 n, FxTiles *o) {
    hipStream_t st = ctx->stream;
    ctx->pin_items.clear(); ctx->pin_used = 0;
    const u64 n_tiles = o->n_tiles = div_up(n, FX_TILE);
    if (n_tiles >> 31) return fx_verdict_rc(ctx, FX_UNPROVEN, "text of 8 TiB or more");
    if (!(o->c_lf = sc.get<u32>(n_tiles)) || !(o->c_rem = sc.get<u32>(n_tiles)) || !(o->c_hdr = sc.get<u32>(n_tiles))) return LRGE_ERR_DEVICE;
    ALLOC_OR_FAIL(d_sum, sc, FxSummary, 1);
    hipLaunchKernelGGL(k_fx_census, dim3((u32)n_tiles), dim3(FX_THREADS), 0, st, t, n, o->c_lf, o->c_rem, o->c_hdr);
    KCHK(ctx);
    hipLaunchKernelGGL(k_fx_summary, dim3(1), dim3(FX_THREADS), 0, st, t, n, (const u32 *)o->c_lf, (const u32 *)o->c_rem, (const u32 *)o->c_hdr, n_tiles, d_sum);
    KCHK(ctx);
    HIPCHK(ctx, ctx->d2h(&o->hs, d_sum, sizeof o->hs, st));
    HIPCHK(ctx, ctx->d2h_sync(st));
    return LRGE_OK;
}

// the record scan over R->d_text: fills the table, the lengths and the identifiers.  w: the text is a window (fx_window.h) --
// scanned up to its cut unless it is the last, its bases copied to the store
static int fx_parse_device(lrge_hip_ctx *ctx, lrge_hip_reads *R, FxWinScan *w) {
    const u64 n = R->n_text;
    const u8 *t = R->d_text;
    R->name_off.assign(1, 0);
    if (n == 0) return LRGE_OK;
    hipStream_t st = ctx->stream;
    Scratch sc(ctx);
    FxTiles tl;
    int rc = fx_census_device(ctx, sc, t, n, &tl);
    if (rc) return rc;
    const auto &[n_tiles, c_lf, c_rem, c_hdr, hs] = tl;
    FxCensus c;
    c.n_lf = hs.n_lf; c.n_rem = hs.n_rem; c.n_hdr = hs.n_hdr; c.first = hs.first; c.last = hs.last;
    for (int i = 0; i < 4; ++i) c.head[i] = (u8)(hs.head >> (8 * i));
    c.at_first = (u8)hs.at_first; c.tail = (u8)hs.tail;
    if (w) fx_win_census(c, w->first);
    u32 verdict = 0;
    const int fmt = fx_format(n, c, &verdict);
    if (verdict) return fx_verdict_rc(ctx, verdict, "neither FASTA nor FASTQ by its first line");
    R->fmt = fmt;
    if (fmt == FX_FMT_EMPTY) return LRGE_OK;
    if ((verdict = fx_limits(fmt, c))) return fx_verdict_rc(ctx, verdict, "line or header count");
    u64 *ls = nullptr, *d_lines = nullptr, *hpos = nullptr;
    u32 *hrem = nullptr;
    u64 n_rec = 0, n_lines = 0, l0 = 0;
    u64 n_use = n, n_lf = c.n_lf, n_rem = c.n_rem;         // a window's prefix is scanned as a text of its own: its size and counts
    const bool to_cut = w && !w->end;
    if (fmt == FX_FMT_FASTQ) {
        if ((rc = scan_exclusive_u32(ctx, sc, c_lf, c_lf, n_tiles, nullptr))) return rc;
        if (!(ls = sc.get<u64>(c.n_lf + 1)) || !(d_lines = sc.get<u64>(2))) return LRGE_ERR_DEVICE;
    } else {
        if ((rc = scan_exclusive_u32(ctx, sc, c_hdr, c_hdr, n_tiles, nullptr))) return rc;
        if ((rc = scan_exclusive_u32(ctx, sc, c_rem, c_rem, n_tiles, nullptr))) return rc;
        if (!(hpos = sc.get<u64>(c.n_hdr)) || !(hrem = sc.get<u32>(c.n_hdr))) return LRGE_ERR_DEVICE;
        n_rec = c.n_hdr;
    }
    hipLaunchKernelGGL(k_fx_scatter, dim3((u32)n_tiles), dim3(FX_THREADS), 0, st, t, n, fmt, (const u32 *)c_lf, (const u32 *)c_rem, (const u32 *)c_hdr, c.first, c.last,
                       ls, d_lines, hpos, hrem);
    KCHK(ctx);
    if (fmt == FX_FMT_FASTQ) {
        u64 lines[2] = {0, 0};
        HIPCHK(ctx, ctx->d2h(lines, d_lines, sizeof lines, st));
        HIPCHK(ctx, ctx->d2h_sync(st));
        l0 = lines[0];
        fx_fastq_shape(n, c, lines[0], lines[1], &n_lines, &n_rec);
        if (to_cut) {
            if (!(n_rec = fx_win_fastq_groups(c.n_lf, lines[0], lines[1]))) { R->fmt = FX_FMT_EMPTY; return LRGE_OK; }
            n_lf = n_lines = l0 + 4 * n_rec;
            HIPCHK(ctx, ctx->d2h(&n_use, ls + n_lf, 8, st));
            HIPCHK(ctx, ctx->d2h_sync(st));
        }
    } else if (to_cut) {
        u32 rem_last = 0;
        n_rec = c.n_hdr - 1;
        HIPCHK(ctx, ctx->d2h(&n_use, hpos + n_rec, 8, st));
        HIPCHK(ctx, ctx->d2h(&rem_last, hrem + n_rec, 4, st));
        HIPCHK(ctx, ctx->d2h_sync(st));
        n_rem = rem_last;
        if (!n_use) { R->fmt = FX_FMT_EMPTY; return LRGE_OK; }
        if (!n_rec) { R->fmt = FX_FMT_EMPTY; w->cut = n_use; return LRGE_OK; }     // (the empty lines in front of the first header: no record, no launch)
    }
    if (w) w->cut = n_use;
    if (n_rec >> 32) return fx_verdict_rc(ctx, FX_TOO_MANY, "records");
    if ((rc = fx_alloc_recs(ctx, R, n_rec))) return rc;
    ALLOC_OR_FAIL(d_seq_len, sc, u32, n_rec);
    ALLOC_OR_FAIL(d_name_len, sc, u32, n_rec);
    ALLOC_OR_FAIL(d_flags, sc, u64, 3);                   // [0]: verdict bits (low word), [1]: identifier bytes, [2]: bases (a run that does not keep all)
    HIPCHK(ctx, hipMemsetAsync(d_flags, 0, 24, st));
    hipLaunchKernelGGL(k_fx_records, dim3((u32)div_up(n_rec, FX_THREADS)), dim3(FX_THREADS), 0, st, t, n_use, fmt, n_rec, (const u64 *)ls, n_lf, n_lines, l0, (const u64 *)hpos,
                       (const u32 *)hrem, n_rem, R->d_recs, d_seq_len, d_name_len, (u32 *)d_flags, (unsigned long long *)(d_flags + 1));
    KCHK(ctx);
    u64 f[3];
    if ((rc = fx_flags_back(ctx, fx_scan_selects(w), d_flags, d_seq_len, n_rec, f))) return rc;
    return fx_scan_tail(ctx, R, sc, w, f, "a record outside the strict form", d_seq_len, d_name_len, n_rec, n_use);
}

#include "host_bam.inl"      // bam_parse_device: the same for unaligned BAM (needs the struct and the tail above)
#include "host_sam.inl"      // sam_parse_device: the same for unaligned SAM

static int fx_parse_kind(lrge_hip_ctx *ctx, lrge_hip_reads *R, int kind, FxWinScan *w) {
    return kind == FX_FMT_BAM ? bam_parse_device(ctx, R, w) : kind == FX_FMT_SAM ? sam_parse_device(ctx, R, w) : fx_parse_device(ctx, R, w);
}

// ---- the sink: where every source leaves the text ----
// The text ends up in R->d_text / R->n_text: all of it (resident), or what is left behind the last flushed window.  A source that
// has no block of its own appends to `blk`; a decoder appends to its own (fx_inflate_to_device).  INGEST_MAX_BYTES bounds either.
struct FxSink {
    lrge_hip_ctx *ctx;
    lrge_hip_reads *R;
    int flags;
    u64 cap, window;
    std::unique_ptr<FxWinRun> run;              // LRGE_GPU_INGEST_WINDOWED: text larger than a window passes through the block in windows (fx_window.h)
    DevKeep blk;
    const u8 *host_text = nullptr;              // the file's bytes, when they are the text
    FxKeepMode mode;                            // the census and the selected open: every text goes through the windows, whatever its size
    static u64 window_bytes(lrge_hip_ctx *c, u64 cap) { return std::max<u64>(1, c->opt_u64("INGEST_WINDOW_BYTES", std::min<u64>((u64)1 << 30, cap / 4))); }
    FxSink(lrge_hip_ctx *c, lrge_hip_reads *r, int f, FxKeepMode m = FX_KEEP_ALL) : ctx(c), R(r), flags(f), cap(ingest_cap(c)),
        window(window_bytes(c, cap)), blk(c), mode(m) {
        if ((flags & LRGE_GPU_INGEST_WINDOWED) || mode != FX_KEEP_ALL) run.reset(new FxWinRun(ctx, R, flags, cap, window));
        blk.keep_max = cap; blk.keep_slack = FX_PAD;
    }
    int over_cap() { LRGE_SET_ERR(ctx, "reads_open: text above INGEST_MAX_BYTES (%llu)", (unsigned long long)cap); return LRGE_ERR_UNPROVEN; }
    // does a text of n bytes go through windows in `blk`?  kind_of(int *kind): the sniff of its first bytes (fx_kind), asked for
    // only where it decides: BAM and SAM that stay resident take the resident route exactly as without the windowed flag
    template <class F> int windowed(u64 n, F kind_of, bool *yes) {
        *yes = false;
        if (mode != FX_KEEP_ALL) { run->attach(&blk); *yes = true; return LRGE_OK; }       // (the first flush sniffs: FxWinDev::selected_format)
        if (!run || n <= window) return LRGE_OK;
        int kind = FX_FMT_EMPTY;
        if (flags & (LRGE_GPU_INGEST_BAM | LRGE_GPU_INGEST_SAM)) { const int rc = kind_of(&kind); if (rc) return rc; }
        if ((*yes = fx_kind_windowed(flags, kind))) run->attach(&blk);
        return LRGE_OK;
    }
    // room for `more` bytes behind what blk holds
    int room(u64 more) {
        // (a block that moved was copied on the main stream, and its old bytes are the pool's again: other streams draw from it)
        if (blk.keep_reserve(more)) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); return LRGE_OK; }
        if (blk.keep_over) return over_cap();
        LRGE_SET_ERR(ctx, "reads_open: device allocation of %llu bytes failed: %s", (unsigned long long)more, hipGetErrorString(blk.e));
        return LRGE_ERR_DEVICE;
    }
    // behind every append to blk: the windows' turn; not 0: the code they stopped the call with
    int appended() { return run->appended() ? (int)LRGE_OK : run->stopped(); }
    // a resident text of `bytes` bytes: its block, the handle's from the start
    int resident(u64 bytes) { return bytes > cap ? over_cap() : fx_alloc_text(ctx, R, bytes); }
    // the text is complete in block b: it becomes the handle's
    void hand_over(DevKeep &b) { R->d_text = b.keep; R->n_text = b.keep_len; b.keep = nullptr; }
};

// ---- the sources ----  the file's bytes are the text: one copy, or copies of a window's size
static int fx_src_raw(FxSink &s, const u8 *d, u64 len) {
    lrge_hip_ctx *ctx = s.ctx;
    s.host_text = d;
    bool windowed;
    int rc = s.windowed(len, [&](int *kind) { return fx_kind(ctx, s.flags, d, nullptr, len, kind); }, &windowed);
    if (rc) return rc;
    if (!windowed) {
        if ((rc = s.resident(len))) return rc;
        if (len) HIPCHK(ctx, hipMemcpyAsync(s.R->d_text, d, (size_t)len, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return LRGE_OK;
    }
    for (u64 off = 0; off < len; off += s.window) {
        const u64 m = std::min<u64>(s.window, len - off);
        if ((rc = s.room(m))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(s.blk.keep + s.blk.keep_len, d + off, (size_t)m, hipMemcpyHostToDevice, ctx->stream));
        s.blk.keep_len += m;
        if ((rc = s.appended())) return rc;
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    s.hand_over(s.blk);
    return LRGE_OK;
}

// blocks `t` of BGZF file d decoded to dst + their o_off by the chunk pipeline of host_inflate.inl, every block checked
static int fx_bgzf_decode(lrge_hip_ctx *ctx, const u8 *d, const std::vector<BgzfBlock> &t, u8 *dst, bool d_pinned = false) {
    BgzfBad bad;
    const int rc = bgzf_inflate_chunks(ctx, d, t, nullptr, dst, "reads_open: bgzf inflate", &bad, d_pinned);
    if (rc) return rc;
    if (bad.status != INF_OK) { ctx->err = "reads_open: a BGZF block failed its checks"; return LRGE_ERR_UNPROVEN; }
    return LRGE_OK;
}

// A batch of the pieces a decoding source works through (BGZF blocks, gzip entries): items [i, the end it returns) of n_items -- items
// until they hold a window of text, at least one.  size(j): the text bytes of item j; *bytes: those of the batch
template <class F> static size_t fx_batch_end(size_t i, size_t n_items, u64 window, F size, u64 *bytes) {
    size_t j = i;
    for (*bytes = 0; j < n_items && (j == i || *bytes < window); ++j) *bytes += size(j);
    return j;
}
// ... and the text bytes of the largest batch: what a staging block for every batch holds
template <class F> static u64 fx_batch_largest(size_t n_items, u64 window, F size) {
    u64 largest = 0, bytes;
    for (size_t i = 0; i < n_items; largest = std::max(largest, bytes)) i = fx_batch_end(i, n_items, window, size, &bytes);
    return largest;
}

// blocks [i, j) of table t as a run of their own for the chunk pipeline: their text lies back to back from offset `at`
static std::vector<BgzfBlock> fx_bgzf_part(const std::vector<BgzfBlock> &t, size_t i, size_t j, u64 at) {
    std::vector<BgzfBlock> part(t.begin() + i, t.begin() + j);
    for (BgzfBlock &b : part) { b.o_off = at; at += b.isize; }
    return part;
}

// BGZF (block table t, `total` text bytes): all blocks in one run of the pipeline, or runs of a window's size
static int fx_src_bgzf(FxSink &s, const u8 *d, const std::vector<BgzfBlock> &t, u64 total) {
    lrge_hip_ctx *ctx = s.ctx;
    if (!(s.flags & LRGE_GPU_INFLATE_BGZF)) { ctx->err = "reads_open: BGZF input without LRGE_GPU_INFLATE_BGZF"; return LRGE_ERR_UNPROVEN; }
    bool windowed;
    int rc = s.windowed(total, [&](int *kind) -> int {      // the first blocks that hold four bytes of text are decoded for the sniff
        std::vector<BgzfBlock> first;
        u64 bytes = 0;
        for (size_t i = 0; i < t.size() && bytes < 4; ++i) { first.push_back(t[i]); bytes += t[i].isize; }
        Scratch sc(ctx);
        ALLOC_OR_FAIL(d_first, sc, u8, bytes + FX_PAD);
        const int drc = fx_bgzf_decode(ctx, d, first, d_first);
        return drc ? drc : fx_kind(ctx, s.flags, nullptr, d_first, total, kind);
    }, &windowed);
    if (rc) return rc;
    if (!windowed) return (rc = s.resident(total)) ? rc : fx_bgzf_decode(ctx, d, t, s.R->d_text);
    // runs of blocks of a window's size, each decoded behind the tail the window before it left
    const auto isize = [&](size_t b) { return (u64)t[b].isize; };
    for (size_t i = 0, j; i < t.size(); i = j) {
        u64 bytes;
        j = fx_batch_end(i, t.size(), s.window, isize, &bytes);
        if ((rc = s.room(bytes)) || (rc = fx_bgzf_decode(ctx, d, fx_bgzf_part(t, i, j, s.blk.keep_len), s.blk.keep))) return rc;
        s.blk.keep_len += bytes;
        if ((rc = s.appended())) return rc;
    }
    s.hand_over(s.blk);
    return LRGE_OK;
}

// gzip, bzip2, Zstandard and xz: the rounds of the decoder's driver (run(&bad): gz_run, bz_run, zs_run, xz_run) with the decoder `dev` keeping
// every round's text in its own block (dev_keep.h), which becomes the handle's.  A windowed call flushes that block through the
// sink's run whenever a round has been appended (DevKeep::keep_flush); whether its windows stay on is the first flush's sniff.
// refused: the message for a stream the decoder does not take, with status(rc) and the file offset.  (One set of driver codes: the
// static_assert beside codec_inflate, host_gzip.inl.)
template <class Dev, class Run, class Status>
static int fx_inflate_to_device(FxSink &s, Dev &dev, Run run, const char *codec, const char *refused, Status status) {
    lrge_hip_ctx *ctx = s.ctx;
    u64 bad = 0;
    dev.to_host = false; dev.keep_max = s.cap; dev.keep_slack = FX_PAD;
    if (s.run) s.run->attach(&dev);
    const int rc = dev.e == hipSuccess ? run(&bad) : (int)GZ_RUN_DEVICE;
    (void)hipStreamSynchronize(ctx->stream);
    if (rc == GZ_RUN_OK) {
        if (!dev.keep && !dev.keep_reserve(0)) { LRGE_SET_ERR(ctx, "reads_open: device allocation failed"); return LRGE_ERR_DEVICE; }
        s.hand_over(dev);
        return LRGE_OK;
    }
    if (s.run && s.run->stopped()) return s.run->stopped();
    if (dev.keep_over) return s.over_cap();
    if (rc == GZ_RUN_DEVICE) {
        LRGE_SET_ERR(ctx, "reads_open: %s inflate: %s", codec, hipGetErrorString(dev.e != hipSuccess ? dev.e : hipErrorUnknown));
        (void)hipGetLastError();
        return LRGE_ERR_DEVICE;
    }
    LRGE_SET_ERR(ctx, refused, status(rc), (unsigned long long)bad);
    return LRGE_ERR_UNPROVEN;
}

// any other gzip input.  map: the census leaves the entry table of a seek map behind (gzip_round.h GzSeekRec)
// src: the streamed first pass -- d is null, and the rounds' ranges [off, off + n) of the file are read from src as they are staged (GzDev::stage)
static int fx_src_gzip(FxSink &s, const u8 *d, u64 len, FxSeekMap *map = nullptr, const FxInput *src = nullptr) {
    lrge_hip_ctx *ctx = s.ctx;
    if (!(s.flags & LRGE_GPU_INFLATE_GZIP)) { ctx->err = "reads_open: gzip input without LRGE_GPU_INFLATE_GZIP"; return LRGE_ERR_UNPROVEN; }
    const GzCfg cfg = gz_cfg(ctx);
    GzStats st;
    GzDev dev(ctx, cfg);
    dev.src = src;
    // a first size: the last member's ISIZE (the whole text of a single-member file below 4 GiB); later rounds grow the block
    u32 isize = 0;
    if (src && !src->gzip_isize(&isize)) return fx_stream_read_failed(ctx);
    if (len >= 18) dev.keep_hint = std::min<u64>(s.cap, src ? isize : bgzf_u32(d + len - 4));
    GzSeekRec<GzDev> rec = {map, map ? map->gz_spacing : 0};
    const int rc = fx_inflate_to_device(s, dev, [&](u64 *bad) {
        return map ? gz_run(dev, d, len, cfg, [](const uint8_t *, uint64_t) { return true; }, st, bad, &rec) : gz_run(dev, d, len, cfg, [](const uint8_t *, uint64_t) { return true; }, st, bad);
    }, "gzip", "reads_open: gzip data not proven on the device (status %d near file offset %llu)", [](int rc) { return rc; });
    return dev.io_failed ? fx_stream_read_failed(ctx) : rc;
}

// bzip2.  map: the census leaves the block table, the marks and the entries of a seek map behind (bz_round.h BzSeekRec)
static int fx_src_bzip2(FxSink &s, const u8 *d, u64 len, FxSeekMap *map = nullptr) {
    BzStats st;
    BzDev dev(s.ctx);
    dev.keep_marks = map != nullptr;
    BzSeekRec<BzDev, FxSeekMap> rec = {map, map ? map->bz_spacing : 0};
    const u64 round = s.ctx->opt_u64("BZIP2_ROUND_BLOCKS", 0);
    const int rc = fx_inflate_to_device(s, dev, [&](u64 *bad) {
        return map ? bz_run(dev, d, len, round, [](const uint8_t *, uint64_t) { return true; }, st, bad, nullptr, &rec) : bz_run(dev, d, len, round, [](const uint8_t *, uint64_t) { return true; }, st, bad);
    }, "bzip2", "reads_open: bzip2 data not accepted by the device (%s near file offset %llu)", bz_status_name);
    if (map) dev.print_timing();                // (option BZIP2_TIMING: the stages of a census that recorded marks; tools/ingest_bench.py)
    return rc;
}

// Zstandard: a match reaches back through the frame's earlier text, so the text is never windowed without
// LRGE_GPU_INGEST_WINDOWED_ZSTD: with LRGE_GPU_INGEST_WINDOWED alone it is taken resident, within INGEST_MAX_BYTES.  With the flag
// the decoder slides (host_zstd.inl): it keeps the history a round needs in a work block of its own, which comes
// out of INGEST_MAX_BYTES beside the window block and the store, and every finished round passes through the windows as a gzip
// round does
static bool fx_zstd_slides(int flags) { return (flags & LRGE_GPU_INFLATE_ZSTD) && (flags & LRGE_GPU_INGEST_WINDOWED_ZSTD); }
static int fx_src_zstd(FxSink &s, const u8 *d, u64 len) {
    ZsStats st;
    ZsSlide sl = {0, 0, 0, 0};
    ZsDev dev(s.ctx);
    if (!fx_zstd_slides(s.flags)) s.run.reset();
    if (s.run) {
        dev.sliding = true; dev.slide_window = s.window;
        dev.work_budget = [&](u64 bytes) {
            if (bytes > s.cap) return false;
            s.run->dev.aside = bytes; dev.keep_max = s.cap - bytes;
            return true;
        };
    }
    const int rc = fx_inflate_to_device(s, dev, [&](u64 *bad) {
        return zs_run(dev, d, len, s.ctx->opt_u64("ZSTD_ROUND_BLOCKS", 0), zs_checksum_on(s.ctx), [](const uint8_t *, uint64_t) { return true; }, st, bad, &sl);
    }, "zstd", "reads_open: zstd data not accepted by the device (%s near file offset %llu)", zs_status_name);
    s.R->zs_slide[0] = sl.rounds; s.R->zs_slide[1] = sl.max_history; s.R->zs_slide[2] = sl.max_work; s.R->zs_slide[3] = sl.moved;
    if (s.ctx->opt("VERBOSE")) fprintf(stderr, "[lrge_hip] reads_open: zstd content checksums %.2f ms of the text-to-HBM share\n", dev.ms[5]);
    return rc;
}

// xz: a block needs no earlier text, so a windowed call flushes every finished round through the sink's windows, as for bzip2
static int fx_src_xz(FxSink &s, const u8 *d, u64 len) {
    XzStats st;
    XzDev dev(s.ctx);
    const int rc = fx_inflate_to_device(s, dev, [&](u64 *bad) { return xz_run(dev, d, len, xz_cfg(s.ctx), [](const uint8_t *, uint64_t) { return true; }, st, bad); },
                                        "xz", "reads_open: xz data not accepted by the device (%s near file offset %llu)", xz_status_name);
    if (s.ctx->opt("VERBOSE")) fprintf(stderr, "[lrge_hip] reads_open: xz decode %.2f ms, block checks %.2f ms of the text-to-HBM share\n", dev.ms[1], dev.ms[2]);
    return rc;
}

#include "host_cram.inl"     // fx_open_cram: unaligned CRAM under LRGE_GPU_INGEST_CRAM (needs the struct, ingest_cap and fx_upload_recs above)

// What the sampled calls refuse by the container's magic and the flags alone, before any device work: CRAM without both of its flags, whatever
// the others (FxWinDev::selected_format), and Zstandard that does not slide -- its text is never windowed without LRGE_GPU_INGEST_WINDOWED_ZSTD
static int fx_sampled_refusal(lrge_hip_ctx *ctx, FxBox box, int flags) {
    if (box == FX_BOX_CRAM && !cram_select_flags(flags)) return fx_fastx_only(ctx);
    if (box == FX_BOX_ZSTD && (flags & LRGE_GPU_INFLATE_ZSTD) && !fx_zstd_slides(flags)) return fx_fastx_only(ctx, ", not Zstandard input");
    return LRGE_OK;
}

// ---- the two ends of a call ----  windows were flushed: the rest of the block is the last, the store the handle's text
static int fx_finish_windowed(FxSink &s, double t0) {
    lrge_hip_reads *R = s.R;
    const int rc = s.run->finish();
    if (rc) return rc;
    R->ms[3] = (float)(fx_now_ms() - t0); R->ms[0] = R->ms[3] - R->ms[1] - R->ms[2];
    if (s.ctx->opt("VERBOSE")) fprintf(stderr, "[lrge_hip] reads_open: %llu text bytes in %llu windows, %llu records, %llu store bytes; record scan %.2f ms, identifiers and lengths %.2f ms\n",
                                       (unsigned long long)R->text_bytes, (unsigned long long)R->win.windows, (unsigned long long)R->n, (unsigned long long)R->n_text, R->ms[1], R->ms[2]);
    return LRGE_OK;
}

// the text is resident: its kind by the sniff (the first bytes are here already for raw input), and the record scan over all of it
static int fx_finish_resident(FxSink &s, double t0) {
    lrge_hip_ctx *ctx = s.ctx;
    lrge_hip_reads *R = s.R;
    R->text_bytes = R->n_text;
    const double t1 = fx_now_ms();
    int kind;
    int rc = fx_kind(ctx, s.flags, s.host_text, R->d_text, R->n_text, &kind);
    if (rc || (rc = fx_parse_kind(ctx, R, kind))) return rc;
    const double t2 = fx_now_ms();
    R->ms[0] = (float)(t1 - t0); R->ms[1] = (float)(t2 - t1) - R->ms[2]; R->ms[3] = (float)(t2 - t0);
    if (ctx->opt("VERBOSE")) fprintf(stderr, "[lrge_hip] reads_open: %llu text bytes, %llu records; text to HBM %.2f ms, record scan %.2f ms, identifiers and lengths %.2f ms\n",
                                    (unsigned long long)R->n_text, (unsigned long long)R->n, R->ms[0], R->ms[1], R->ms[2]);
    return LRGE_OK;
}

extern "C" void lrge_hip_reads_free(lrge_hip_reads *r) {
    if (!r) return;
    bool ctx_alive;
    { std::lock_guard<std::mutex> g(g_live_mu); ctx_alive = g_live_ctx.count(r->ctx) != 0; }
    if (ctx_alive) { r->ctx->pool.release(r->d_text); r->ctx->pool.release(r->d_recs); }     // (a destroyed context has already freed its pool)
    delete r;
}
// the handle a call fills: freed unless the call releases it to the caller
using FxReadsGuard = std::unique_ptr<lrge_hip_reads, void (*)(lrge_hip_reads *)>;
static FxReadsGuard fx_new_reads(lrge_hip_ctx *ctx) {
    FxReadsGuard guard(new lrge_hip_reads(), lrge_hip_reads_free);
    guard->ctx = ctx;
    return guard;
}

// a census that leaves a seek map: the map as every source finds it
static void fx_map_begin(FxSink &s, FxSeekMap *map, u64 file_len) {
    *map = FxSeekMap();
    map->stride = std::max<u64>(1, s.ctx->opt_u64("INGEST_SEEK_STRIDE_BYTES", 65536));
    map->kind = FX_SEEK_OTHER; map->file_len = file_len;
    s.run->dev.map = map;
}
static void fx_map_gzip(lrge_hip_ctx *ctx, FxSeekMap *map) { map->kind = FX_SEEK_GZIP; map->gz_spacing = std::max<u64>(1, ctx->opt_u64("INGEST_SEEK_GZIP_BYTES", (u64)1 << 20)); }

// behind the source of a call: the end that fits how the text arrived (windowed: windows were flushed, or the run does not keep all), the
// tables of the seek map (t: the block table of a BGZF file), and the handle is the caller's
static int fx_open_finish(FxSink &s, FxReadsGuard &guard, bool windowed, FxSeekMap *map, const std::vector<BgzfBlock> &t, double t0, lrge_hip_reads **out) {
    int rc;
    if ((rc = windowed ? fx_finish_windowed(s, t0) : fx_finish_resident(s, t0))) return rc;
    if (map) {
        map->records = guard->sel.seen; map->bases = guard->sel.bases_seen; map->text_bytes = guard->text_bytes; map->windows = guard->win.windows;
        map->fmt = guard->fmt;
        if (map->kind == FX_SEEK_BGZF) fx_seek_attach(*map, t.data(), t.size());
        // (BAM and SAM inside plain gzip keep the full selected pass: DESIGN section 28 -- the entry table is dropped)
        // ... and so does a map that is not worth entering (fx_gz_enterable)
        if (map->kind == FX_SEEK_GZIP && (map->fmt == FX_FMT_BAM || map->fmt == FX_FMT_SAM || !fx_gz_enterable(*map))) { map->kind = FX_SEEK_OTHER; map->ent = {}; map->ent_win = {}; map->gz_spacing = 0; }
        if (map->kind == FX_SEEK_GZIP) fx_seek_attach_gzip(*map);
        // (BAM and SAM inside bzip2 too; and a sole entry over several blocks could skip nothing: fx_bz_enterable)
        if (map->kind == FX_SEEK_BZIP2 && (map->fmt == FX_FMT_BAM || map->fmt == FX_FMT_SAM || !fx_bz_enterable(*map))) {
            map->kind = FX_SEEK_OTHER; map->bz = {}; map->bz_marks = {}; map->bz_ent = {}; map->bz_spacing = 0; map->bz_level = 0;
        }
        if (map->kind == FX_SEEK_BZIP2) fx_seek_attach_bzip2(*map);
    }
    *out = guard.release();
    return LRGE_OK;
}

// one call: lrge_hip_reads_open_mem (FX_KEEP_ALL), the census (FX_KEEP_NONE) or the selected open (FX_KEEP_SEL with sel[0, k))
// map: a census (FX_KEEP_NONE) that leaves the seek map of the text behind (fx_seek.h)
static int fx_open_mem(lrge_hip_ctx *ctx, const void *file_bytes, uint64_t len, int flags, FxKeepMode mode, const u32 *sel, u64 k, lrge_hip_reads **out, FxSeekMap *map = nullptr) {
    if (!ctx || !out || (!file_bytes && len)) return LRGE_ERR_INVALID;
    *out = nullptr;
    int rc;
    if (mode == FX_KEEP_SEL && (rc = fx_sel_checked(ctx, sel, k))) return rc;
    const u8 *d = (const u8 *)file_bytes;
    bool xz_whole;
    const FxBox box = fx_container(d, len, &xz_whole);
    if (mode != FX_KEEP_ALL && (rc = fx_sampled_refusal(ctx, box, flags))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const double t0 = fx_now_ms();
    FxReadsGuard guard = fx_new_reads(ctx);
    // unaligned CRAM, for the caller who asked for it: a host walk and a device decode of the base blocks, no text and no record scan;
    // its sampled ingest: no text and no windows either -- the walk, then the rounds into a scratch
    if (box == FX_BOX_CRAM && (mode != FX_KEEP_ALL || (flags & LRGE_GPU_INGEST_CRAM))) {
        if ((rc = mode != FX_KEEP_ALL ? fx_cram_sampled(ctx, guard.get(), d, len, mode, sel, k, false, map, t0) : fx_open_cram(ctx, guard.get(), d, len, t0))) return rc;
        *out = guard.release();
        return LRGE_OK;
    }
    FxSink s(ctx, guard.get(), flags, mode);
    // the source, by the file's magic
    std::vector<BgzfBlock> t;
    uint64_t total = 0;
    if (mode != FX_KEEP_ALL && (rc = s.run->dev.select(mode, sel, k))) return rc;
    if (map) fx_map_begin(s, map, len);
    if (box == FX_BOX_GZIP) {
        const bool bgzf = bgzf_scan_blocks(d, len, &t, &total);
        if (map && bgzf) { map->kind = FX_SEEK_BGZF; map->n_blocks = t.size(); }
        if (map && !bgzf) fx_map_gzip(ctx, map);
        rc = bgzf ? fx_src_bgzf(s, d, t, total) : fx_src_gzip(s, d, len, map);
    }
    else if (box == FX_BOX_BZIP2 && (flags & LRGE_GPU_INFLATE_BZIP2)) {
        if (map) { map->kind = FX_SEEK_BZIP2; map->bz_spacing = std::max<u64>(1, ctx->opt_u64("INGEST_SEEK_BZIP2_BYTES", (u64)512 << 10)); map->bz_level = len >= 4 ? d[3] : 0; }
        rc = fx_src_bzip2(s, d, len, map);
    }
    else if (box == FX_BOX_ZSTD && (flags & LRGE_GPU_INFLATE_ZSTD)) rc = fx_src_zstd(s, d, len);
    else if (box == FX_BOX_XZ && xz_whole && (flags & LRGE_GPU_INFLATE_XZ)) rc = fx_src_xz(s, d, len);
    else if (box == FX_BOX_BZIP2 || box == FX_BOX_ZSTD || box == FX_BOX_XZ) {
        ctx->err = "reads_open: bzip2, zstd and xz input is decompressed on the host";
        rc = LRGE_ERR_UNPROVEN;
    } else { if (map) map->kind = FX_SEEK_PLAIN; rc = fx_src_raw(s, d, len); }
    if (rc) return rc;
    return fx_open_finish(s, guard, s.run && (s.run->win.st.windows || mode != FX_KEEP_ALL), map, t, t0, out);
}

extern "C" int lrge_hip_reads_open_mem(lrge_hip_ctx *ctx, const void *file_bytes, uint64_t len, int flags, lrge_hip_reads **out) {
    return fx_open_mem(ctx, file_bytes, len, flags, FX_KEEP_ALL, nullptr, 0, out);
}

// ---- the selected ingest: a pass that keeps nothing, and one that keeps the chosen records ----
// the census, with the seek map it leaves behind when one is asked for; out is zeroed by the caller
static int fx_census(lrge_hip_ctx *ctx, const void *file_bytes, uint64_t len, int flags, uint64_t out[4], FxSeekMap *map) {
    lrge_hip_reads *r = nullptr;
    const int rc = fx_open_mem(ctx, file_bytes, len, flags, FX_KEEP_NONE, nullptr, 0, &r, map);
    if (rc) return rc;
    out[0] = r->sel.seen; out[1] = r->sel.bases_seen; out[2] = r->text_bytes; out[3] = r->win.windows;
    lrge_hip_reads_free(r);
    return LRGE_OK;
}

extern "C" int lrge_hip_reads_census_mem(lrge_hip_ctx *ctx, const void *file_bytes, uint64_t len, int flags, uint64_t out[4]) {
    if (!ctx || !out) return LRGE_ERR_INVALID;
    out[0] = out[1] = out[2] = out[3] = 0;
    return fx_census(ctx, file_bytes, len, flags, out, nullptr);
}

extern "C" int lrge_hip_reads_open_selected_mem(lrge_hip_ctx *ctx, const void *file_bytes, uint64_t len, int flags, const uint32_t *sel, uint32_t k, lrge_hip_reads **out) {
    return fx_open_mem(ctx, file_bytes, len, flags, FX_KEEP_SEL, sel, k, out);
}

// the file at `path` as one buffer (raw holds it)
static int fx_slurp(lrge_hip_ctx *ctx, const char *path, std::string *raw) {
    try { *raw = lrge::io::slurp(path); } catch (const std::exception &e) { ctx->err = e.what(); return LRGE_ERR_IO; }
    return LRGE_OK;
}
// ... for the call that takes a path: mem(bytes, len) is its form that takes a buffer
template <class F> static int fx_with_file(lrge_hip_ctx *ctx, const char *path, F mem) {
    std::string raw;
    const int rc = fx_slurp(ctx, path, &raw);
    return rc ? rc : mem(raw.data(), (uint64_t)raw.size());
}

// ---- the streamed first pass (LRGE_GPU_INGEST_STREAM): the file is read in pieces into two pinned slots ----
// Two pinned host buffers that grow on demand, an event each that says when the copy out of it is done.  peak: the most bytes both held
struct FxSlots {
    lrge_hip_ctx *ctx;
    u8 *p[2] = {nullptr, nullptr};
    u64 cap[2] = {0, 0}, peak = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool busy[2] = {false, false};
    explicit FxSlots(lrge_hip_ctx *c) : ctx(c) {}
    ~FxSlots() { release(); }
    void release() {
        for (int i = 0; i < 2; ++i) {
            if (busy[i]) (void)hipEventSynchronize(ev[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
            if (p[i]) (void)hipHostFree(p[i]);
            p[i] = nullptr; cap[i] = 0; ev[i] = nullptr; busy[i] = false;
        }
    }
    // slot i holds `bytes` bytes at least; its contents are not kept
    int need(int i, u64 bytes) {
        if (p[i] && cap[i] >= bytes) return LRGE_OK;
        int rc;
        if ((rc = wait(i))) return rc;
        if (p[i]) (void)hipHostFree(p[i]);
        p[i] = nullptr; cap[i] = 0;
        HIPCHK(ctx, hipHostMalloc((void **)&p[i], (size_t)std::max<u64>(bytes, 64), hipHostMallocDefault));
        cap[i] = std::max<u64>(bytes, 64);
        peak = std::max(peak, cap[0] + cap[1]);
        return LRGE_OK;
    }
    // a copy out of slot i was queued on `st`: the slot is written again only behind it
    int sent(int i, hipStream_t st) {
        if (!ev[i]) HIPCHK(ctx, hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        HIPCHK(ctx, hipEventRecord(ev[i], st));
        busy[i] = true;
        return LRGE_OK;
    }
    int wait(int i) {
        if (busy[i]) { busy[i] = false; HIPCHK(ctx, hipEventSynchronize(ev[i])); }
        return LRGE_OK;
    }
};

// plain input: slot 0 holds the file's first n0 bytes; pread fills one slot while the copy of the other is in flight, a piece at a time
static int fx_src_raw_stream(FxSink &s, const FxInput &in, FxSlots &sl, u64 n0, u64 piece) {
    lrge_hip_ctx *ctx = s.ctx;
    s.run->attach(&s.blk);
    int rc, cur = 0;
    for (u64 fill = n0, fpos = n0;;) {
        if ((rc = s.room(fill))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(s.blk.keep + s.blk.keep_len, sl.p[cur], (size_t)fill, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = sl.sent(cur, ctx->stream))) return rc;
        s.blk.keep_len += fill;
        const u64 next = std::min<u64>(piece, in.len - fpos);
        if (next) {
            if ((rc = sl.need(cur ^ 1, next)) || (rc = sl.wait(cur ^ 1))) return rc;
            if (!in.read(fpos, next, sl.p[cur ^ 1])) return fx_stream_read_failed(ctx);
        }
        if ((rc = s.appended())) return rc;
        if (s.run->win.off) return fx_stream_needs_aln(ctx);
        if (!next) break;
        cur ^= 1; fill = next; fpos += next;
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    s.hand_over(s.blk);
    return LRGE_OK;
}

// BGZF: slot 0 holds the file's first n0 bytes.  A slot holds the partial member the slot before it ended in and up to P bytes read
// behind it (more where one member needs more); its whole members are found by the walk of bgzf_scan.h and decoded from where they
// lie, in batches of a window of text as fx_src_bgzf makes them; the partial member at its end moves to the front of the other
// slot.  Whether the file is BGZF is its first member's word (*is_bgzf false: nothing was delivered, the gzip source takes the
// file); a later member that is no BGZF block, a truncated one and trailing bytes end the call.  all (may be null): the whole
// file's block table, for a seek map
static int fx_src_bgzf_stream(FxSink &s, const FxInput &in, FxSlots &sl, u64 n0, u64 P, std::vector<BgzfBlock> *all, bool *is_bgzf) {
    lrge_hip_ctx *ctx = s.ctx;
    *is_bgzf = false;
    int rc, cur = 0;
    u64 fill = n0, base = 0, fpos = n0, o = 0, need = 18;      // the slot holds file [base, base + fill); fpos: the next byte to read; o: text bytes so far
    for (;;) {
        std::vector<BgzfBlock> part;                           // the slot's whole members, c_off counted from the slot's front
        u64 used = 0, bad = 0;
        const int w = bgzf_walk_members(sl.p[cur], fill, base, 0, &o, &part, &used, &need, &bad);
        const bool over = fpos == in.len;
        if (w == BGZF_MEMBER_BAD || (w == BGZF_MEMBER_MORE && over)) {
            if (!*is_bgzf && part.empty()) return LRGE_OK;
            return fx_stream_not_bgzf(ctx, w == BGZF_MEMBER_BAD ? bad : base + used);
        }
        if (w == BGZF_MEMBER_OK) need = 18;
        if (!part.empty()) {
            if (!*is_bgzf) {
                *is_bgzf = true;
                if (!(s.flags & LRGE_GPU_INFLATE_BGZF)) { ctx->err = "reads_open: BGZF input without LRGE_GPU_INFLATE_BGZF"; return LRGE_ERR_UNPROVEN; }
                s.run->attach(&s.blk);
            }
            if (all) for (BgzfBlock b : part) { b.c_off += base; all->push_back(b); }
            const auto isize = [&](size_t b) { return (u64)part[b].isize; };
            for (size_t i = 0, j; i < part.size(); i = j) {
                u64 bytes;
                j = fx_batch_end(i, part.size(), s.window, isize, &bytes);
                if ((rc = s.room(bytes)) || (rc = fx_bgzf_decode(ctx, sl.p[cur], fx_bgzf_part(part, i, j, s.blk.keep_len), s.blk.keep, true))) return rc;
                s.blk.keep_len += bytes;
                if ((rc = s.appended())) return rc;
                if (s.run->win.off) return fx_stream_needs_aln(ctx);
            }
        }
        const u64 rest = fill - used;
        if (over && !rest) break;
        const u64 more = std::min<u64>(in.len - fpos, std::max<u64>(P, need > rest ? need - rest : 0));
        if ((rc = sl.need(cur ^ 1, std::max<u64>(sl.cap[0], rest + more)))) return rc;     // (slot 0 was made for P bytes and one member: the two are the same size whatever the file's length)
        if (rest) memcpy(sl.p[cur ^ 1], sl.p[cur] + used, (size_t)rest);
        if (!in.read(fpos, more, sl.p[cur ^ 1] + rest)) return fx_stream_read_failed(ctx);
        cur ^= 1; base += used; fill = rest + more; fpos += more;
    }
    s.hand_over(s.blk);
    return LRGE_OK;
}

// One call that takes a path under LRGE_GPU_INGEST_STREAM: plain text, BGZF and gzip are read in pieces of option INGEST_STREAM_BYTES
// and every text passes through the windows whatever its size; every other container, and an empty file, is read whole as without
// the flag.  The call's reading is left in ctx->stream_stats
static int fx_open_stream(lrge_hip_ctx *ctx, FxInput &in, int flags, FxKeepMode mode, const u32 *sel, u64 k, lrge_hip_reads **out, FxSeekMap *map = nullptr) {
    *out = nullptr;
    int rc;
    if (mode == FX_KEEP_SEL && (rc = fx_sel_checked(ctx, sel, k))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const double t0 = fx_now_ms();
    const u64 P = std::max<u64>(1, ctx->opt_u64("INGEST_STREAM_BYTES", (u64)64 << 20));
    const u64 piece = std::min<u64>(P, FxSink::window_bytes(ctx, ingest_cap(ctx)));
    const u64 n0 = std::min<u64>(in.len, std::max<u64>(piece, 6));      // (the sniff of the container wants six bytes)
    FxSlots sl(ctx);
    u64 pinned = 0;
    const auto stats = [&](bool streamed) { ctx->stream_stats[0] = in.n_reads; ctx->stream_stats[1] = in.n_bytes; ctx->stream_stats[2] = std::max(pinned, sl.peak); ctx->stream_stats[3] = streamed; };
    stats(false);
    // (P bytes and the partial member in front of them: the size a BGZF slot needs, so that the pinned bytes do not depend on where the members lie)
    if (n0 && ((rc = sl.need(0, std::max<u64>(n0, std::min<u64>(P, in.len)) + 65536)) || (rc = in.read(0, n0, sl.p[0]) ? (int)LRGE_OK : fx_stream_read_failed(ctx)))) return rc;
    const FxBox box = fx_container(sl.p[0], n0);
    if (!n0 || (box != FX_BOX_OTHER && box != FX_BOX_GZIP)) {  // read whole: the route without the flag
        sl.release();
        std::string raw;
        if (!(rc = fx_slurp(ctx, in.path, &raw))) { ++in.n_reads; in.n_bytes += raw.size(); rc = fx_open_mem(ctx, raw.data(), raw.size(), flags, mode, sel, k, out, map); }
        stats(false);
        return rc;
    }
    FxReadsGuard guard = fx_new_reads(ctx);
    FxSink s(ctx, guard.get(), flags, mode);
    std::vector<BgzfBlock> t;
    if (mode != FX_KEEP_ALL && (rc = s.run->dev.select(mode, sel, k))) return rc;
    if (map) fx_map_begin(s, map, in.len);
    if (box == FX_BOX_GZIP) {
        bool bgzf = false;
        rc = fx_src_bgzf_stream(s, in, sl, n0, P, map ? &t : nullptr, &bgzf);
        if (map && bgzf) { map->kind = FX_SEEK_BGZF; map->n_blocks = t.size(); }
        if (!rc && !bgzf) {
            sl.release();
            if (map) fx_map_gzip(ctx, map);
            rc = fx_src_gzip(s, nullptr, in.len, map, &in);
            pinned = ctx->gz_pin_cap[0];
        }
    } else { if (map) map->kind = FX_SEEK_PLAIN; rc = fx_src_raw_stream(s, in, sl, n0, piece); }
    stats(true);
    if (rc) return rc;
    if (s.run->win.off) return fx_stream_needs_aln(ctx);
    sl.release();
    rc = fx_open_finish(s, guard, true, map, t, t0, out);
    if (!rc && s.run->win.off) { lrge_hip_reads_free(*out); *out = nullptr; return fx_stream_needs_aln(ctx); }      // (a text that ended before its first flush was sniffed by the last window)
    return rc;
}
// the census of a streamed call, as fx_census
static int fx_census_stream(lrge_hip_ctx *ctx, FxInput &in, int flags, uint64_t out[4], FxSeekMap *map) {
    lrge_hip_reads *r = nullptr;
    const int rc = fx_open_stream(ctx, in, flags, FX_KEEP_NONE, nullptr, 0, &r, map);
    if (rc) return rc;
    out[0] = r->sel.seen; out[1] = r->sel.bases_seen; out[2] = r->text_bytes; out[3] = r->win.windows;
    lrge_hip_reads_free(r);
    return LRGE_OK;
}
// ... for the four calls that take a path: with the flag `streamed(in)`, else mem(bytes, len) over the whole file
template <class S, class F> static int fx_with_path(lrge_hip_ctx *ctx, const char *path, int flags, S streamed, F mem) {
    if (flags & LRGE_GPU_INGEST_STREAM) {
        FxInput in;
        memset(ctx->stream_stats, 0, sizeof ctx->stream_stats);
        if (!in.open_path(path)) return fx_open_failed(ctx, path);
        return streamed(in);
    }
    const int rc = fx_with_file(ctx, path, [&](const void *d, uint64_t n) {
        ctx->stream_stats[0] = 1; ctx->stream_stats[1] = n; ctx->stream_stats[2] = ctx->stream_stats[3] = 0;
        return mem(d, n);
    });
    if (rc == LRGE_ERR_IO) memset(ctx->stream_stats, 0, sizeof ctx->stream_stats);
    return rc;
}

extern "C" int lrge_hip_last_stream_stats(const lrge_hip_ctx *ctx, uint64_t out[4]) {
    if (!ctx || !out) return LRGE_ERR_INVALID;
    memcpy(out, ctx->stream_stats, sizeof ctx->stream_stats);
    return LRGE_OK;
}

extern "C" int lrge_hip_reads_census(lrge_hip_ctx *ctx, const char *path, int flags, uint64_t out[4]) {
    if (!ctx || !path || !out) return LRGE_ERR_INVALID;
    return fx_with_path(ctx, path, flags, [&](FxInput &in) {
        out[0] = out[1] = out[2] = out[3] = 0;
        return fx_census_stream(ctx, in, flags, out, nullptr);
    }, [&](const void *d, uint64_t n) { return lrge_hip_reads_census_mem(ctx, d, n, flags, out); });
}

extern "C" int lrge_hip_reads_open_selected(lrge_hip_ctx *ctx, const char *path, int flags, const uint32_t *sel, uint32_t k, lrge_hip_reads **out) {
    if (!ctx || !path || !out) return LRGE_ERR_INVALID;
    *out = nullptr;
    return fx_with_path(ctx, path, flags, [&](FxInput &in) { return fx_open_stream(ctx, in, flags, FX_KEEP_SEL, sel, k, out); },
                        [&](const void *d, uint64_t n) { return lrge_hip_reads_open_selected_mem(ctx, d, n, flags, sel, k, out); });
}

extern "C" int lrge_hip_reads_select_stats(const lrge_hip_reads *r, uint64_t out[4]) {
    if (!r || !out) return LRGE_ERR_INVALID;
    out[0] = r->sel.seen; out[1] = r->sel.kept; out[2] = r->sel.bases_seen; out[3] = r->sel.bases_kept;
    return LRGE_OK;
}

// ---- the seek map and the mapped second pass (fx_seek.h) ----
extern "C" int lrge_hip_reads_census_map_mem(lrge_hip_ctx *ctx, const void *file_bytes, uint64_t len, int flags, uint64_t out[4], lrge_hip_read_map **map) {
    if (!ctx || !out || !map) return LRGE_ERR_INVALID;
    *map = nullptr;
    out[0] = out[1] = out[2] = out[3] = 0;
    std::unique_ptr<lrge_hip_read_map> m(new lrge_hip_read_map());
    const int rc = fx_census(ctx, file_bytes, len, flags, out, &m->m);
    if (!rc) *map = m.release();
    return rc;
}

extern "C" int lrge_hip_reads_census_map(lrge_hip_ctx *ctx, const char *path, int flags, uint64_t out[4], lrge_hip_read_map **map) {
    if (!ctx || !path || !out || !map) return LRGE_ERR_INVALID;
    *map = nullptr;
    return fx_with_path(ctx, path, flags, [&](FxInput &in) {
        out[0] = out[1] = out[2] = out[3] = 0;
        std::unique_ptr<lrge_hip_read_map> m(new lrge_hip_read_map());
        const int rc = fx_census_stream(ctx, in, flags, out, &m->m);
        if (!rc) *map = m.release();
        return rc;
    }, [&](const void *d, uint64_t n) { return lrge_hip_reads_census_map_mem(ctx, d, n, flags, out, map); });
}

extern "C" void lrge_hip_read_map_free(lrge_hip_read_map *map) { delete map; }

// (a CRAM map, kind FX_SEEK_CRAM: out[1] counts its points, one a slice in which a record starts; out[2], the stride, is 0; out[3] the bases.
// lrge_hip_read_map_points: text_off is the slice's base offset, c_off the file offset of its BA block)
extern "C" int lrge_hip_read_map_stats(const lrge_hip_read_map *map, uint64_t out[4]) {
    if (!map || !out) return LRGE_ERR_INVALID;
    out[0] = map->m.records; out[1] = map->m.pts.size(); out[2] = map->m.stride; out[3] = map->m.text_bytes;
    return LRGE_OK;
}

extern "C" int lrge_hip_read_map_points(const lrge_hip_read_map *map, uint64_t *ord, uint64_t *text_off, uint64_t *c_off, uint64_t cap) {
    if (!map) return LRGE_ERR_INVALID;
    for (u64 i = 0; i < map->m.pts.size() && i < cap; ++i) {
        if (ord) ord[i] = map->m.pts[i].ord;
        if (text_off) text_off[i] = map->m.pts[i].off;
        if (c_off) c_off[i] = map->m.pts[i].c_off;
    }
    return LRGE_OK;
}

extern "C" int lrge_hip_read_map_entries(const lrge_hip_read_map *map, uint64_t out[4]) {
    if (!map || !out) return LRGE_ERR_INVALID;
    out[0] = map->m.ent.size(); out[1] = map->m.ent_win.size(); out[2] = (uint64_t)map->m.kind; out[3] = map->m.gz_spacing;
    if (map->m.kind == FX_SEEK_BZIP2) { out[0] = map->m.bz_ent.size(); out[1] = map->m.bz_marks.size() * sizeof(BzMark); out[3] = map->m.bz_spacing; }
    return LRGE_OK;
}

extern "C" int lrge_hip_reads_seek_stats(const lrge_hip_reads *r, uint64_t out[4]) {
    if (!r || !out) return LRGE_ERR_INVALID;
    memcpy(out, r->seek, sizeof r->seek);
    return LRGE_OK;
}

// (the file of a mapped open -- the whole buffer, or a descriptor that is read by range: FxInput, fx_input.h)
// the whole file in memory, for what takes a buffer: the input is read by its path into raw, unless it is a buffer already
static int fx_input_whole(lrge_hip_ctx *ctx, FxInput &in, std::string *raw) {
    if (in.d) return LRGE_OK;
    const int rc = fx_slurp(ctx, in.path, raw);
    if (!rc) { in.d = (const u8 *)raw->data(); in.len = raw->size(); }
    return rc;
}
struct FxPinned {
    u8 *p = nullptr;
    ~FxPinned() { if (p) (void)hipHostFree(p); }
};

// plain input: the runs' bytes gathered into pinned staging, one copy per window's worth of sub-text
static int fx_src_seek_raw(FxSink &s, const FxInput &in, const FxSeekPlan &plan) {
    lrge_hip_ctx *ctx = s.ctx;
    const u64 piece = std::min<u64>(s.window, plan.text_bytes);
    int rc;
    FxPinned stage;
    if (piece) HIPCHK(ctx, hipHostMalloc((void **)&stage.p, (size_t)piece, hipHostMallocDefault));
    u64 fill = 0;
    const auto send = [&]() -> int {
        if ((rc = s.room(fill))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(s.blk.keep + s.blk.keep_len, stage.p, (size_t)fill, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));            // (the staging is filled again)
        s.blk.keep_len += fill; fill = 0;
        return s.appended();
    };
    for (const FxSeekRun &r : plan.runs)
        for (u64 at = r.t0; at < r.t1;) {
            const u64 m = std::min<u64>(piece - fill, r.t1 - at);
            if (!in.read(at, m, stage.p + fill)) return fx_read_failed(ctx);
            fill += m; at += m;
            if (fill == piece && (rc = send())) return rc;
        }
    if (fill && (rc = send())) return rc;
    s.hand_over(s.blk);
    return LRGE_OK;
}

// A batch of decoded pieces lies in a staging block: text [o_off, o_off + len) at d_stage + src, the pieces ascending in o_off (BGZF
// blocks, gzip entries).  What the runs take of them, in order, is the sub-text's next bytes: k_fx_runs copies it to the tail of the
// sink's block, and the windows take their turn (take).  ri / rpos: the run that is being brought and its next text byte.  Behind the
// last batch every run has been brought, and the block becomes the handle's (finish)
struct FxPiece { u64 o_off, len, src; };
struct FxRunsTaker {
    FxSink &s; const FxSeekPlan &plan;
    size_t ri = 0; u64 rpos;
    FxRunsTaker(FxSink &s_, const FxSeekPlan &p) : s(s_), plan(p), rpos(p.runs.empty() ? 0 : p.runs[0].t0) {}
    int take(const std::vector<FxPiece> &pc, const u8 *d_stage, u64 bytes) {
        lrge_hip_ctx *ctx = s.ctx;
        int rc;
        std::vector<FxRunCopy> copies;
        u64 sum = 0;
        for (size_t b = 0; b < pc.size() && ri < plan.runs.size();) {
            const FxSeekRun &r = plan.runs[ri];
            const u64 bo = pc[b].o_off, be = bo + pc[b].len;
            if (rpos >= r.t1) { if (++ri < plan.runs.size()) rpos = plan.runs[ri].t0; continue; }
            if (rpos >= be) { ++b; continue; }
            if (rpos < bo) return fx_map_range(ctx);               // (never: the pieces cover the runs)
            const u64 m = std::min<u64>(r.t1, be) - rpos, src = pc[b].src + (rpos - bo);
            if (src + m > bytes) return fx_map_range(ctx);         // (never)
            if (!copies.empty() && copies.back().src + copies.back().len == src) copies.back().len += m;
            else copies.push_back(FxRunCopy{src, sum, m});
            sum += m; rpos += m;
        }
        if (!sum) return LRGE_OK;
        if (sum >> 32) return s.run->dev.unproven("a window of 2^32 bytes or more");     // (the driver refuses such a block anyway; the grid below is a tile a wavefront)
        if ((rc = s.room(sum))) return rc;
        Scratch tables(ctx);                                       // (the batch's: released before the next)
        std::vector<u64> first(copies.size() + 1, 0);
        for (size_t c = 0; c < copies.size(); ++c) first[c + 1] = first[c] + div_up(copies[c].len, (u64)FX_RUN_TILE);
        ALLOC_OR_FAIL(d_copies, tables, FxRunCopy, copies.size());
        ALLOC_OR_FAIL(d_first, tables, u64, first.size());
        HIPCHK(ctx, hipMemcpyAsync(d_copies, copies.data(), copies.size() * sizeof(FxRunCopy), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_first, first.data(), first.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_fx_runs, dim3((u32)first.back()), dim3(64), 0, ctx->stream, d_stage, s.blk.keep + s.blk.keep_len,
                           (const FxRunCopy *)d_copies, (const u64 *)d_first, (u32)copies.size());
        KCHK(ctx);
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));            // (the tables are pageable, and the staging is decoded into again)
        s.blk.keep_len += sum;
        return s.appended();
    }
    int finish() {
        while (ri < plan.runs.size() && rpos >= plan.runs[ri].t1) if (++ri < plan.runs.size()) rpos = plan.runs[ri].t0;
        if (ri < plan.runs.size()) return fx_map_range(s.ctx);
        s.hand_over(s.blk);
        return LRGE_OK;
    }
};

// BGZF: only the blocks some run touches are decoded, each once, in batches of about a window into a staging block; k_fx_runs
// copies the parts of the runs that lie in a batch to the tail of the sink's block.  The file ranges of the plan are read (or, from
// a buffer, copied) back to back into `comp`, which the chunk pipeline takes as a file of its own -- a chunk's blocks must be
// contiguous --, and scanned: every range must hold the blocks the map says
static int fx_src_seek_bgzf(FxSink &s, const FxInput &in, const FxSeekPlan &plan) {
    lrge_hip_ctx *ctx = s.ctx;
    if (!(s.flags & LRGE_GPU_INFLATE_BGZF)) { ctx->err = "reads_open: BGZF input without LRGE_GPU_INFLATE_BGZF"; return LRGE_ERR_UNPROVEN; }
    std::vector<BgzfBlock> fb;                  // the blocks of the runs, once each: c_off in `comp`, o_off in the whole text
    std::vector<u8> comp;
    u64 prev_b1 = 0, prev_f1 = 0;
    for (const FxSeekRun &r : plan.runs) {
        const bool joins = !fb.empty() && prev_b1 > r.b0;          // the run starts in a block the run before ended in
        const u64 b_from = joins ? prev_b1 : r.b0;
        if (b_from < r.b1) {
            const u64 f_from = joins ? prev_f1 : r.f0, o_from = joins ? fb.back().o_off + fb.back().isize : r.o0, at = comp.size();
            if (r.f1 <= f_from || r.f1 > in.len) return fx_map_range(ctx);
            comp.resize((size_t)(at + (r.f1 - f_from)));
            if (!in.read(f_from, r.f1 - f_from, comp.data() + at)) return fx_read_failed(ctx);
            std::vector<BgzfBlock> part;
            u64 total = 0;
            if (!bgzf_scan_blocks(comp.data() + at, r.f1 - f_from, &part, &total) || part.size() != r.b1 - b_from) return fx_map_range(ctx);
            for (BgzfBlock &b : part) { b.c_off += at; b.o_off += o_from; fb.push_back(b); }
        }
        if (fb.empty() || r.t0 < r.o0 || r.t1 > fb.back().o_off + fb.back().isize) return fx_map_range(ctx);
        prev_b1 = r.b1; prev_f1 = r.f1;
    }
    const u8 *base = comp.data();
    // batches of blocks of a window's size, as fx_src_bgzf makes them; the staging holds the largest
    const auto isize = [&](size_t b) { return (u64)fb[b].isize; };
    Scratch sc(ctx);
    ALLOC_OR_FAIL(d_stage, sc, u8, fx_batch_largest(fb.size(), s.window, isize) + FX_PAD);
    int rc;
    FxRunsTaker runs(s, plan);
    for (size_t i = 0, j; i < fb.size(); i = j) {
        u64 bytes;
        j = fx_batch_end(i, fb.size(), s.window, isize, &bytes);
        const std::vector<BgzfBlock> part = fx_bgzf_part(fb, i, j, 0);
        if ((rc = fx_bgzf_decode(ctx, base, part, d_stage))) return rc;
        std::vector<FxPiece> pc;
        for (size_t b = i; b < j; ++b) pc.push_back(FxPiece{fb[b].o_off, fb[b].isize, part[b - i].o_off});
        if ((rc = runs.take(pc, d_stage, bytes))) return rc;
    }
    return runs.finish();
}

// Plain and multi-member gzip: only the entries some run touches are decoded, each once and each from its seed by
// one wavefront (k_gz_entry), in batches of about a window of text.  The file ranges of the plan go back to back through pinned
// staging to the device in one copy, the entries' windows in another.  An entry's text length is the map's, so a batch's entries lie
// back to back in the staging block by a prefix: no slot ratio, no retry.  An entry that does not end where the map says, or whose
// length or CRC-32 differs, is a map that does not fit the input
static int fx_src_seek_gzip(FxSink &s, const FxInput &in, const FxSeekMap &m, const FxSeekPlan &plan) {
    lrge_hip_ctx *ctx = s.ctx;
    if (!(s.flags & LRGE_GPU_INFLATE_GZIP)) { ctx->err = "reads_open: gzip input without LRGE_GPU_INFLATE_GZIP"; return LRGE_ERR_UNPROVEN; }
    // the entries of the runs, once each, and where their file bytes lie in the staging (ranges that touch or overlap are one)
    struct Need { u64 ent, c_at; };
    std::vector<Need> need;
    u64 comp_len = 0, range_f0 = 0, range_f1 = 0, range_at = 0, prev_b1 = 0;
    std::vector<std::pair<u64, u64>> ranges;    // file [first, second)
    for (const FxSeekRun &r : plan.runs)
        for (u64 b = need.empty() ? r.b0 : std::max<u64>(r.b0, prev_b1); b < r.b1; prev_b1 = ++b) {
            if (b >= m.ent.size()) return fx_map_range(ctx);
            const u64 f0 = m.ent[b].bit >> 3, f1 = fx_gz_cover_end(m, b);
            if (f1 < f0 || f1 > in.len || f1 - f0 >= ((u64)1 << 29)) return f1 > in.len || f1 < f0 ? fx_map_range(ctx) : s.over_cap();      // (bit offsets of a decode are 32 bits wide)
            if (ranges.empty() || f0 > range_f1) { range_at = comp_len; range_f0 = f0; range_f1 = f1; ranges.push_back({f0, f1}); comp_len += f1 - f0; }
            else if (f1 > range_f1) { comp_len += f1 - range_f1; range_f1 = f1; ranges.back().second = f1; }
            need.push_back(Need{b, range_at + (f0 - range_f0)});
        }
    if (need.size() != plan.blocks || comp_len != plan.file_bytes) return fx_map_range(ctx);        // (never: the planner counts the same entries and bytes)
    // batches of about a window of text, as fx_src_seek_bgzf makes them; the staging holds the largest
    const auto ent_len = [&](size_t a) { return (u64)m.ent[need[a].ent].len; };
    const u64 stage_cap = fx_batch_largest(need.size(), s.window, ent_len);
    if (stage_cap > s.cap || stage_cap >> 32) return s.over_cap();     // (one entry's text above the budget: its length is a 32-bit count on the device)
    FxPinned pin;
    const u64 win_bytes = (u64)need.size() * GZ_WIN;
    if (comp_len + win_bytes) HIPCHK(ctx, hipHostMalloc((void **)&pin.p, (size_t)(comp_len + win_bytes), hipHostMallocDefault));
    {
        u64 at = 0;
        for (const auto &r : ranges) { if (!in.read(r.first, r.second - r.first, pin.p + at)) return fx_read_failed(ctx); at += r.second - r.first; }
        for (size_t i = 0; i < need.size(); ++i) memcpy(pin.p + comp_len + i * (size_t)GZ_WIN, m.ent_win.data() + need[i].ent * (size_t)GZ_WIN, GZ_WIN);
    }
    Scratch sc(ctx);
    ALLOC_OR_FAIL(d_comp, sc, u8, comp_len + win_bytes + 16);
    ALLOC_OR_FAIL(d_stage, sc, u8, stage_cap + FX_PAD);
    const u8 *d_wins = d_comp + comp_len;       // (read by bytes: no alignment asked)
    if (comp_len + win_bytes) HIPCHK(ctx, hipMemcpyAsync(d_comp, pin.p, (size_t)(comp_len + win_bytes), hipMemcpyHostToDevice, ctx->stream));
    int rc;
    FxRunsTaker runs(s, plan);
    for (size_t i = 0, end; i < need.size(); i = end) {
        std::vector<GzEntryTask> task;
        std::vector<FxPiece> pc;
        u64 bytes, at = 0;                      // at: where the entry's text lies in the staging block
        end = fx_batch_end(i, need.size(), s.window, ent_len, &bytes);
        for (size_t j = i; j < end; ++j) {
            const u64 b = need[j].ent;
            const FxGzEntry &e = m.ent[b];
            const bool last = b + 1 == m.ent.size();
            const u64 f0 = e.bit >> 3;
            task.push_back(GzEntryTask{need[j].c_at, at, (u32)(fx_gz_cover_end(m, b) - f0), (u32)(e.bit & 7), last ? GZ_NONE : (u32)(m.ent[b + 1].bit - 8 * f0), (u32)e.len,
                                       e.crc, e.valid, b ? (u32)j : GZ_NONE, last ? 1u : 0u});
            pc.push_back(FxPiece{e.off, e.len, at});
            at += e.len;
        }
        Scratch tables(ctx);
        std::vector<u32> status(task.size());
        ALLOC_OR_FAIL(d_task, tables, GzEntryTask, task.size());
        ALLOC_OR_FAIL(d_status, tables, u32, task.size());
        HIPCHK(ctx, hipMemcpyAsync(d_task, task.data(), task.size() * sizeof(GzEntryTask), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_gz_entry, dim3((u32)task.size()), dim3(64), 0, ctx->stream, (const u8 *)d_comp, (const GzEntryTask *)d_task, (u32)task.size(), d_wins, d_stage, d_status);
        KCHK(ctx);
        HIPCHK(ctx, hipMemcpyAsync(status.data(), d_status, task.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t k = 0; k < status.size(); ++k)
            if (status[k]) {
                char why[96];
                snprintf(why, sizeof why, "gzip entry %llu: status %u", (unsigned long long)need[i + k].ent, status[k]);
                return fx_map_misfit(ctx, why);
            }
        if ((rc = runs.take(pc, d_stage, bytes))) return rc;
    }
    return runs.finish();
}

// bzip2: only the entries some run touches are decoded, each block of them once.  The file ranges of the plan go back
// to back through pinned staging to the device in one copy, the needed blocks' marks behind them.  k_bz_decode and k_bz_scatter run
// unchanged on positions rebased to the staged ranges; a block is accepted only if the decode's n, origPtr, stored CRC and length in
// bits are the map's.  Then one wavefront a block enters it at its 64 marks (k_bz_marks_text).  A block's text length is the map's, so
// a batch's blocks lie back to back in the staging block by a prefix, and no length comes back.  Batches are about a window of text
// inside groups of at most the blocks a round of the decoder holds (BzDev::default_round), which the entropy decode takes at once
static int fx_src_seek_bzip2(FxSink &s, const FxInput &in, const FxSeekMap &m, const FxSeekPlan &plan) {
    lrge_hip_ctx *ctx = s.ctx;
    if (!(s.flags & LRGE_GPU_INFLATE_BZIP2)) { ctx->err = "reads_open: bzip2, zstd and xz input is decompressed on the host"; return LRGE_ERR_UNPROVEN; }
    // the blocks of the runs' entries, once each, and where their first byte lies in the staging (ranges that touch or overlap are one)
    struct Need { u64 blk, c_at; };
    std::vector<Need> need;
    u64 comp_len = 0, range_f0 = 0, range_f1 = 0, range_at = 0, prev_b1 = 0, n_ent = 0;
    std::vector<std::pair<u64, u64>> ranges;    // file [first, second)
    for (const FxSeekRun &r : plan.runs)
        for (u64 b = n_ent ? std::max<u64>(r.b0, prev_b1) : r.b0; b < r.b1; prev_b1 = ++b, ++n_ent) {
            if (b >= m.bz_ent.size() || m.bz_ent[b].b0 >= m.bz_ent[b].b1 || m.bz_ent[b].b1 > m.bz.size()) return fx_map_range(ctx);
            const u64 f0 = fx_bz_cover_begin(m, b), f1 = fx_bz_cover_end(m, b);
            if (f1 < f0 || f1 > in.len) return fx_map_range(ctx);
            if (ranges.empty() || f0 > range_f1) { range_at = comp_len; range_f0 = f0; range_f1 = f1; ranges.push_back({f0, f1}); comp_len += f1 - f0; }
            else if (f1 > range_f1) { comp_len += f1 - range_f1; range_f1 = f1; ranges.back().second = f1; }
            for (u64 q = m.bz_ent[b].b0; q < m.bz_ent[b].b1; ++q) {
                const FxBzBlock &k = m.bz[q];
                if (k.bit >> 3 < f0 || k.end_bit <= k.bit || (k.end_bit + 7) >> 3 > f1 || k.len >> 32) return fx_map_range(ctx);
                need.push_back(Need{q, range_at + ((k.bit >> 3) - range_f0)});
            }
        }
    if (n_ent != plan.blocks || comp_len != plan.file_bytes) return fx_map_range(ctx);        // (never: the planner counts the same entries and bytes)
    const u32 bs = (u32)(m.bz_level - '0') * 100000u;
    BzDev dev(ctx);
    // The entropy decode is one serial chain a block, so its latency is one block's however many blocks a launch holds: it runs once
    // for a group of as many blocks as a round of the decoder holds.  The text of a group is then made in batches of about a window
    const size_t most = dev.default_round(bs);
    const auto blk_len = [&](size_t a) { return (u64)m.bz[need[a].blk].len; };
    struct Batch { size_t i, end; u64 bytes; };
    std::vector<Batch> batches;
    u64 stage_cap = 0;
    for (size_t g = 0; g < need.size(); g = std::min(need.size(), g + most))
        for (size_t i = g, g_end = std::min(need.size(), g + most), end; i < g_end; i = end) {
            u64 bytes;
            end = fx_batch_end(i, g_end, s.window, blk_len, &bytes);
            batches.push_back(Batch{i, end, bytes});
            stage_cap = std::max(stage_cap, bytes);
        }
    if (stage_cap > s.cap || stage_cap >> 32) return s.over_cap();     // (the text of one batch above the budget)
    const auto dev_rc = [&]() -> int {
        LRGE_SET_ERR(ctx, "reads_open: bzip2 inflate: %s", hipGetErrorString(dev.e != hipSuccess ? dev.e : hipErrorUnknown));
        (void)hipGetLastError();
        return LRGE_ERR_DEVICE;
    };
    FxPinned pin;
    const u64 marks_at = ((comp_len + 15) & ~(u64)15) + BZ_PAD, total = marks_at + (u64)need.size() * FX_BZ_MARKS * sizeof(BzMark);
    HIPCHK(ctx, hipHostMalloc((void **)&pin.p, (size_t)total, hipHostMallocDefault));
    {
        u64 at = 0;
        for (const auto &r : ranges) { if (!in.read(r.first, r.second - r.first, pin.p + at)) return fx_read_failed(ctx); at += r.second - r.first; }
        memset(pin.p + comp_len, 0, (size_t)(marks_at - comp_len));
        for (size_t i = 0; i < need.size(); ++i) memcpy(pin.p + marks_at + i * (size_t)FX_BZ_MARKS * sizeof(BzMark), &m.bz_marks[need[i].blk * (size_t)FX_BZ_MARKS], FX_BZ_MARKS * sizeof(BzMark));
    }
    if (!dev.stage_up(pin.p, comp_len, marks_at, total)) return dev_rc();
    Scratch sc(ctx);
    ALLOC_OR_FAIL(d_stage, sc, u8, stage_cap + FX_PAD);
    int rc;
    FxRunsTaker runs(s, plan);
    size_t g = 0, g_end = 0;                    // the group whose blocks the decode left in slots 0 .. g_end - g - 1
    for (const Batch &bt : batches) {
        if (bt.i >= g_end) {
            g = bt.i; g_end = std::min(need.size(), g + most);
            const u32 k = (u32)(g_end - g);
            std::vector<u64> pos(k);
            std::vector<BzRes> res(k);
            for (u32 j = 0; j < k; ++j) pos[j] = 8 * need[g + j].c_at + (m.bz[need[g + j].blk].bit & 7);
            if (!dev.decode(pos.data(), k, bs, res.data())) return dev_rc();
            for (u32 j = 0; j < k; ++j) {
                const FxBzBlock &b = m.bz[need[g + j].blk];
                const BzRes &r = res[j];
                if (r.status == BZ_OK && r.n == b.n && r.orig == b.orig && r.crc == b.crc && r.end_bit - pos[j] == b.end_bit - b.bit) continue;
                char why[128];
                snprintf(why, sizeof why, "bzip2 block %llu: %s", (unsigned long long)need[g + j].blk, r.status != BZ_OK ? bz_status_name((int)r.status) : "another block than the map's");
                return fx_map_misfit(ctx, why);
            }
        }
        const u32 k = (u32)(bt.end - bt.i);
        std::vector<BzLink> links(k);
        std::vector<BzMarkTask> task(k);
        std::vector<u32> status(k);
        std::vector<FxPiece> pc;
        u64 at = 0;                             // where the block's text lies in the staging block
        for (u32 j = 0; j < k; ++j) {
            const FxBzBlock &b = m.bz[need[bt.i + j].blk];
            links[j] = BzLink{0, 0, (u32)(bt.i + j - g), b.n, b.orig, 0};
            task[j] = BzMarkTask{0, at, b.n, b.orig, b.crc, (u32)b.len, (u32)(bt.i + j), 0};
            pc.push_back(FxPiece{b.off, b.len, at});
            at += b.len;
        }
        if (!dev.seeded(links.data(), task.data(), k, d_stage, status.data())) return dev_rc();
        for (u32 j = 0; j < k; ++j)
            if (status[j]) {
                char why[128];
                snprintf(why, sizeof why, "bzip2 block %llu: %s", (unsigned long long)need[bt.i + j].blk, bz_status_name((int)status[j]));
                return fx_map_misfit(ctx, why);
            }
        if ((rc = runs.take(pc, d_stage, bt.bytes))) return rc;
    }
    dev.print_timing();
    return runs.finish();
}

// One mapped open.  Everything that can be refused is refused before any device work: a selection that is not ascending, a map of
// another input, an ordinal at or above the map's records
static int fx_open_mapped(lrge_hip_ctx *ctx, FxInput &in, int flags, const lrge_hip_read_map *map, const u32 *sel, u64 k, lrge_hip_reads **out) {
    *out = nullptr;
    int rc = fx_sel_checked(ctx, sel, k);
    if (rc) return rc;
    const FxSeekMap &m = map->m;
    u8 h[6] = {0, 0, 0, 0, 0, 0};
    const u64 nh = std::min<u64>(6, in.len);
    if (!in.read(0, nh, h)) return fx_read_failed(ctx);
    const FxBox box = fx_container(h, nh);
    if (m.kind == FX_SEEK_CRAM && box != FX_BOX_CRAM) return fx_map_other(ctx);
    // what the census and the selected open refuse by name, whatever the map
    if ((rc = fx_sampled_refusal(ctx, box, flags))) return rc;
    std::string raw;                            // the whole file, where it is not read by range
    if (box == FX_BOX_CRAM) {                   // the mapped open of a CRAM: the walk again, then only the touched slices' blocks
        if ((rc = fx_input_whole(ctx, in, &raw))) return rc;
        HIPCHK(ctx, hipSetDevice(ctx->device));
        FxReadsGuard guard = fx_new_reads(ctx);
        FxSeekMap of = m;
        if ((rc = fx_cram_sampled(ctx, guard.get(), in.d, in.len, FX_KEEP_SEL, sel, k, true, &of, fx_now_ms()))) return rc;
        *out = guard.release();
        return LRGE_OK;
    }
    // (a BAM map: DESIGN section 25; a SAM map: section 27)
    if ((m.fmt == FX_FMT_BAM && !fx_select_aln(flags)) || (m.fmt == FX_FMT_SAM && !fx_select_sam(flags))) return fx_fastx_only(ctx);
    const bool gz = box == FX_BOX_GZIP, packed = gz || box == FX_BOX_BZIP2 || box == FX_BOX_ZSTD || box == FX_BOX_XZ;
    std::vector<BgzfBlock> t;
    u64 total = 0;
    bool fits = m.file_len == in.len && (m.kind == FX_SEEK_PLAIN ? !packed && m.text_bytes == in.len : m.kind == FX_SEEK_BGZF || m.kind == FX_SEEK_GZIP ? gz :
                                         m.kind == FX_SEEK_BZIP2 ? box == FX_BOX_BZIP2 : packed);
    if (fits && m.kind == FX_SEEK_BZIP2) {      // the level byte is the census's; the tables are whole: as many entries as the points name, all blocks in them, a set of marks a block, all of the text
        fits = nh >= 4 && h[3] == m.bz_level && m.bz_level >= '1' && m.bz_level <= '9' && !m.bz_ent.empty() && m.bz_ent.size() == m.n_blocks && m.bz_ent.back().b1 == m.bz.size() &&
               m.bz_marks.size() == m.bz.size() * (size_t)FX_BZ_MARKS && m.bz[0].bit == 32 && m.bz.back().off + m.bz.back().len == m.text_bytes;
    }
    if (fits && m.kind == FX_SEEK_GZIP) {       // the entry table is whole: as many entries as the points name, a window each but the first, all of the text
        fits = !m.ent.empty() && m.ent.size() == m.n_blocks && m.ent_win.size() == m.ent.size() * (size_t)FX_GZ_WIN && m.ent[0].bit == 0 &&
               m.ent.back().off + m.ent.back().len == m.text_bytes;
    }
    if (fits && in.d && gz) {                   // the whole buffer is here: its block table says which kind it is
        const bool bgzf = bgzf_scan_blocks(in.d, in.len, &t, &total);
        fits = bgzf == (m.kind == FX_SEEK_BGZF) && (!bgzf || (t.size() == m.n_blocks && total == m.text_bytes));
    }
    if (!fits) return fx_map_other(ctx);
    for (u64 j = 0; j < k; ++j)
        if (sel[j] >= m.records) return fx_ordinal_rc(ctx, sel[j], m.records);
    if (m.kind == FX_SEEK_OTHER) {              // a container that cannot be entered: the full selected pass, the same handle
        lrge_hip_reads *r = nullptr;
        // (the path form under LRGE_GPU_INGEST_STREAM: that pass streams where the container allows)
        if (!in.d && (flags & LRGE_GPU_INGEST_STREAM)) { if ((rc = fx_open_stream(ctx, in, flags, FX_KEEP_SEL, sel, k, &r))) return rc; }
        else if ((rc = fx_input_whole(ctx, in, &raw)) || (rc = fx_open_mem(ctx, in.d, in.len, flags, FX_KEEP_SEL, sel, k, &r))) return rc;
        if (r->sel.seen != m.records || r->text_bytes != m.text_bytes) { lrge_hip_reads_free(r); return fx_map_misfit(ctx, "another record count"); }
        *out = r;
        return LRGE_OK;
    }
    FxSeekPlan plan;
    fx_seek_plan(m, sel, k, &plan);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const double t0 = fx_now_ms();
    FxReadsGuard guard = fx_new_reads(ctx);
    lrge_hip_reads *R = guard.get();
    FxSink s(ctx, R, flags, FX_KEEP_SEL);
    s.run->dev.mapped = true;
    if (m.fmt == FX_FMT_BAM || m.fmt == FX_FMT_SAM) s.run->dev.kind = m.fmt;      // (the sub-text is never sniffed: it is a record stream, or whole SAM lines, without a header)
    if ((rc = s.run->dev.select(FX_KEEP_SEL, plan.sel.data(), k))) return rc;
    s.run->attach(&s.blk);
    rc = m.kind == FX_SEEK_PLAIN ? fx_src_seek_raw(s, in, plan) : m.kind == FX_SEEK_GZIP ? fx_src_seek_gzip(s, in, m, plan) : m.kind == FX_SEEK_BZIP2 ? fx_src_seek_bzip2(s, in, m, plan) :
                                                                                                                                     fx_src_seek_bgzf(s, in, plan);
    if (!rc) rc = fx_finish_windowed(s, t0);
    // the sub-text is proven again, and holds exactly the planner's records: else the input is not the one the map was made of
    if (rc == LRGE_ERR_INVALID && s.run->dev.at < s.run->dev.k) return fx_map_misfit(ctx, "fewer records than the plan");
    if (rc == LRGE_ERR_UNPROVEN && s.run->dev.scan_refused) { const std::string why = ctx->err; return fx_map_misfit(ctx, why.c_str()); }
    if (rc) return rc;
    if (R->sel.seen != plan.records) return fx_map_misfit(ctx, "another record count");
    R->sel.seen = m.records; R->sel.bases_seen = m.bases; R->text_bytes = m.text_bytes;
    if (R->fmt == FX_FMT_EMPTY) R->fmt = m.fmt;
    R->seek[0] = plan.runs.size(); R->seek[1] = plan.text_bytes; R->seek[2] = plan.file_bytes; R->seek[3] = plan.blocks;
    *out = guard.release();
    return LRGE_OK;
}

extern "C" int lrge_hip_reads_open_mapped_mem(lrge_hip_ctx *ctx, const void *file_bytes, uint64_t len, int flags, const lrge_hip_read_map *map, const uint32_t *sel, uint32_t k,
                                              lrge_hip_reads **out) {
    if (!ctx || !out || !map || (!file_bytes && len)) return LRGE_ERR_INVALID;
    static const u8 none = 0;
    FxInput in;
    in.d = file_bytes ? (const u8 *)file_bytes : &none; in.len = len;
    return fx_open_mapped(ctx, in, flags, map, sel, k, out);
}

extern "C" int lrge_hip_reads_open_mapped(lrge_hip_ctx *ctx, const char *path, int flags, const lrge_hip_read_map *map, const uint32_t *sel, uint32_t k, lrge_hip_reads **out) {
    if (!ctx || !path || !out || !map) return LRGE_ERR_INVALID;
    *out = nullptr;
    FxInput in;
    if (!in.open_path(path)) return fx_open_failed(ctx, path);
    return fx_open_mapped(ctx, in, flags, map, sel, k, out);
}

extern "C" int lrge_hip_reads_open(lrge_hip_ctx *ctx, const char *path, int flags, lrge_hip_reads **out) {
    if (!ctx || !path || !out) return LRGE_ERR_INVALID;
    *out = nullptr;
    if ((flags & LRGE_GPU_INGEST_STREAM) && !(flags & LRGE_GPU_INGEST_WINDOWED)) return fx_stream_needs_windowed(ctx);
    return fx_with_path(ctx, path, flags, [&](FxInput &in) { return fx_open_stream(ctx, in, flags, FX_KEEP_ALL, nullptr, 0, out); },
                        [&](const void *d, uint64_t n) { return lrge_hip_reads_open_mem(ctx, d, n, flags, out); });
}

extern "C" uint64_t lrge_hip_reads_count(const lrge_hip_reads *r) { return r ? r->n : 0; }
extern "C" uint64_t lrge_hip_reads_name_bytes(const lrge_hip_reads *r) { return r ? r->names.size() : 0; }
extern "C" uint64_t lrge_hip_reads_text_bytes(const lrge_hip_reads *r) { return r ? r->text_bytes : 0; }

extern "C" int lrge_hip_reads_table(const lrge_hip_reads *r, uint32_t *seq_len, uint64_t *name_off, char *names) {
    if (!r) return LRGE_ERR_INVALID;
    if (seq_len && r->n) memcpy(seq_len, r->seq_len.data(), (size_t)r->n * 4);
    if (name_off) memcpy(name_off, r->name_off.data(), ((size_t)r->n + 1) * 8);
    if (names && !r->names.empty()) memcpy(names, r->names.data(), r->names.size());
    return LRGE_OK;
}

extern "C" int lrge_hip_reads_timings(const lrge_hip_reads *r, float ms[4]) {
    if (!r || !ms) return LRGE_ERR_INVALID;
    memcpy(ms, r->ms, sizeof r->ms);
    return LRGE_OK;
}

extern "C" int lrge_hip_reads_window_stats(const lrge_hip_reads *r, uint64_t out[4]) {
    if (!r || !out) return LRGE_ERR_INVALID;
    out[0] = r->win.windows; out[1] = r->win.bases; out[2] = r->win.max_window; out[3] = r->win.carried;
    return LRGE_OK;
}

extern "C" int lrge_hip_reads_zstd_stats(const lrge_hip_reads *r, uint64_t out[4]) {
    if (!r || !out) return LRGE_ERR_INVALID;
    memcpy(out, r->zs_slide, sizeof r->zs_slide);
    return LRGE_OK;
}

extern "C" int lrge_hip_seqset_from_reads(lrge_hip_ctx *ctx, const lrge_hip_reads *r, const uint32_t *idx, uint32_t n, const uint32_t *name_rank,
                                          lrge_hip_seqset **out) {
    if (!ctx || !r || !out || r->ctx != ctx || (n && !idx)) return LRGE_ERR_INVALID;
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<u64> boff((size_t)n + 1);
    u64 o = 0;
    for (u32 j = 0; j < n; ++j) {
        if (idx[j] >= r->n) { LRGE_SET_ERR(ctx, "seqset_from_reads: index %u of %llu reads", idx[j], (unsigned long long)r->n); return LRGE_ERR_INVALID; }
        boff[j] = o; o += r->seq_len[idx[j]];
    }
    boff[n] = o;
    Scratch sc(ctx);
    ALLOC_OR_FAIL(d_dense, sc, u8, o + FX_PAD);
    ALLOC_OR_FAIL(d_idx, sc, u32, std::max<u32>(1, n));
    ALLOC_OR_FAIL(d_boff, sc, u64, (size_t)n + 1);
    if (n) {
        HIPCHK(ctx, hipMemcpyAsync(d_idx, idx, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_boff, boff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        const u32 grid = std::min<u32>(n, (u32)ctx->n_cu * 32);
        if (r->fmt == FX_FMT_BAM)
            hipLaunchKernelGGL(k_bam_gather, dim3(grid), dim3(64), 0, ctx->stream, (const u8 *)r->d_text, (const FxRec *)r->d_recs, (const u32 *)d_idx, (const u64 *)d_boff, n,
                               d_dense);
        else
            hipLaunchKernelGGL(k_fx_gather, dim3(grid), dim3(64), 0, ctx->stream, (const u8 *)r->d_text, r->n_text, (const FxRec *)r->d_recs, (const u32 *)d_idx,
                               (const u64 *)d_boff, n, d_dense);
        KCHK(ctx);
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));        // (idx and boff are pageable: their copies are done; the pack below is ordered behind the gather anyway)
    }
    // the dense ASCII is a device source of the ordinary upload: the packed image is the one a host upload of the same reads gives
    return seqset_upload_impl(ctx, (const char *)d_dense, boff.data(), n, name_rank, false, out);
}
