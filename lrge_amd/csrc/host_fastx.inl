// host_fastx.inl -- read sets built on the device from FASTA / FASTQ text (k_fastx.h), from unaligned BAM
// (k_bam.h, host_bam.inl) and from unaligned SAM (k_sam.h, host_sam.inl): the text reaches HBM
// decompressed (BGZF chunks decoded into one block by the pipeline of host_inflate.inl, the gzip and bzip2 rounds appended device-to-device, plain input copied once), the
// record scan runs there, only identifiers and lengths come back, and lrge_hip_seqset_from_reads gathers the selected reads
// into dense ASCII for the device-source pack of host_seqset.inl.  Whatever the scan cannot prove is LRGE_ERR_UNPROVEN: the
// caller takes lrge_hip_read_records*, which parses the file or reports it with the reference's messages.  With
// LRGE_GPU_INGEST_WINDOWED FASTA / FASTQ text larger than option INGEST_WINDOW_BYTES passes through HBM in windows and only the
// bases stay (fx_window.h); with LRGE_GPU_INGEST_WINDOWED_ALN beside it so does unaligned BAM and SAM, BAM's
// bases staying packed.  Included into lrge_hip.hip.

#include "fx_window.h"

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
};

static double fx_now_ms() { return DevPool::now_ms(); }

static u64 ingest_cap(lrge_hip_ctx *ctx) {
    size_t mfree = 0, mtot = 0;
    if (hipMemGetInfo(&mfree, &mtot) != hipSuccess) { (void)hipGetLastError(); mfree = 0; }
    return ctx->opt_u64("INGEST_MAX_BYTES", ((u64)mfree + ctx->pool.idle()) / 2);       // (the batch planner's accounting: idle arena bytes are reusable)
}

static int fx_over_cap_rc(lrge_hip_ctx *ctx, u64 cap) {
    LRGE_SET_ERR(ctx, "reads_open: text above INGEST_MAX_BYTES (%llu)", (unsigned long long)cap);
    return LRGE_ERR_UNPROVEN;
}

static int fx_verdict_rc(lrge_hip_ctx *ctx, u32 verdict, const char *what) {
    if (verdict & FX_UNPROVEN) { LRGE_SET_ERR(ctx, "reads_open: not proven on the device (%s)", what); return LRGE_ERR_UNPROVEN; }
    LRGE_SET_ERR(ctx, "reads_open: 2^32 records or a sequence of 2^32 bases (%s)", what);
    return LRGE_ERR_TOO_MANY;
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

// BAM and SAM by their magic, when the caller asked for them (head: the first min(4, n) text bytes)
static void fx_sniff_bam_sam(int flags, const u8 head[4], u64 n, bool *is_bam, bool *is_sam) {
    *is_bam = (flags & LRGE_GPU_INGEST_BAM) && n >= 4 && head[0] == 'B' && head[1] == 'A' && head[2] == 'M' && head[3] == 1;
    *is_sam = (flags & LRGE_GPU_INGEST_SAM) && n >= 3 && sam_sniff(head, n);
}

// BAM and SAM that stay resident: all of them, unless the caller asked for their windows as well
static bool fx_stays_resident(int flags, bool is_bam, bool is_sam) { return (is_bam || is_sam) && !(flags & LRGE_GPU_INGEST_WINDOWED_ALN); }

// ---- windowed ingest: the device backend of fx_window.h ----
struct FxWinDev;
// the scan of one window (fx_parse_device, bam_parse_device, sam_parse_device): up to its cut (left in `cut`; 0: there is none
// yet) unless `end`
struct FxWinScan { FxWinDev *dev; bool first, end; u64 cut; };
static int fx_parse_device(lrge_hip_ctx *ctx, lrge_hip_reads *R, FxWinScan *w = nullptr);
static int bam_parse_device(lrge_hip_ctx *ctx, lrge_hip_reads *R, FxWinScan *w = nullptr);
static int sam_parse_device(lrge_hip_ctx *ctx, lrge_hip_reads *R, FxWinScan *w = nullptr);

struct FxWinDev {
    lrge_hip_ctx *ctx;
    lrge_hip_reads *R;                          // collects the identifiers and lengths of every window
    int flags;
    u64 cap;                                    // INGEST_MAX_BYTES: the block and the store together
    DevKeep *blk = nullptr;                     // the block the text is appended to (a decoder's own, or one of the call)
    DevKeep store;                              // the bases of the records flushed so far, dense, in file order (BAM: packed, a record starts on a byte)
    int kind = FX_FMT_EMPTY;                    // FX_FMT_BAM / FX_FMT_SAM: the run is that format's, by the sniff of its first bytes; else FASTA / FASTQ
    u64 through = 0;                            // text bytes cut off the block so far
    double ms_scan = 0, ms_names = 0;
    int rc = LRGE_OK;                           // what stopped the windows, with its message (a decoder's hook can only say "stop")
    std::string msg;
    FxWinDev(lrge_hip_ctx *c, lrge_hip_reads *r, int f, u64 cap_) : ctx(c), R(r), flags(f), cap(cap_), store(c) {
        store.keep_on = true; store.keep_slack = FX_PAD; store.keep_floor = 0;      // (block and store share one budget: neither takes more than it needs or doubles to)
        R->name_off.assign(1, 0);
    }
    u64 len() const { return blk->keep_len; }
    int unproven(const char *what) { LRGE_SET_ERR(ctx, "reads_open: not proven on the device (%s)", what); return LRGE_ERR_UNPROVEN; }
    // BAM and SAM with their flags are not windowed unless LRGE_GPU_INGEST_WINDOWED_ALN says so; with it this sniff, the first
    // window's, makes the run a BAM or SAM run: a later window is never sniffed.  (Plain and BGZF input is sniffed before a
    // window is set up as well, lrge_hip_reads_open_mem; the round decoders' first bytes arrive with a round.)
    int resident_format(bool *yes) {
        *yes = false;
        if (!(flags & (LRGE_GPU_INGEST_BAM | LRGE_GPU_INGEST_SAM))) return LRGE_OK;
        u8 head[4] = {0, 0, 0, 0};
        HIPCHK(ctx, hipMemcpyAsync(head, blk->keep, (size_t)std::min<u64>(4, blk->keep_len), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        bool is_bam, is_sam;
        fx_sniff_bam_sam(flags, head, blk->keep_len, &is_bam, &is_sam);
        *yes = fx_stays_resident(flags, is_bam, is_sam);
        if (!*yes) kind = is_bam ? FX_FMT_BAM : is_sam ? FX_FMT_SAM : FX_FMT_EMPTY;
        return LRGE_OK;
    }
    // the growth rule a resident text has without the flag (attach() had made the block a window's)
    u64 was_hint = 0, was_floor = 0, was_grow = 2;
    void resident_again() { blk->keep_hint = was_hint; blk->keep_floor = was_floor; blk->keep_grow = was_grow; blk->keep_max = cap; }     // (keep_flush stays: it is running, and the driver returns at once from now on)
    int flush(bool first, bool end, u64 *cut, int *fmt) {
        lrge_hip_reads W;                       // the window as a text of its own; the block stays the decoder's
        W.ctx = ctx; W.d_text = blk->keep; W.n_text = blk->keep_len;
        FxWinScan w = {this, first, end, 0};
        const double t0 = fx_now_ms();
        const int prc = kind == FX_FMT_BAM ? bam_parse_device(ctx, &W, &w) : kind == FX_FMT_SAM ? sam_parse_device(ctx, &W, &w) : fx_parse_device(ctx, &W, &w);
        ctx->pool.release(W.d_recs);
        ms_names += W.ms[2]; ms_scan += fx_now_ms() - t0 - W.ms[2];
        if (prc) return prc;
        *cut = end ? W.n_text : w.cut; *fmt = W.fmt;
        if (*cut) { u64 *sum = &R->bam.segments; const u64 *add = &W.bam.segments; for (int i = 0; i < 6; ++i) sum[i] += add[i]; }
        if (!*cut || !W.n) return LRGE_OK;
        if ((R->n + W.n) >> 32) return fx_verdict_rc(ctx, FX_UNPROVEN, "2^32 records or more");
        if ((R->names.size() + W.names.size()) >> 32) return fx_verdict_rc(ctx, FX_UNPROVEN, "4 GiB of identifiers or more");
        const u64 at = R->names.size();
        R->names += W.names;
        R->seq_len.insert(R->seq_len.end(), W.seq_len.begin(), W.seq_len.end());
        for (u64 i = 1; i <= W.n; ++i) R->name_off.push_back(at + W.name_off[i]);
        R->n += W.n;
        return LRGE_OK;
    }
    // the bases of the window's records (table W.d_recs, lengths d_seq_len) behind those of the earlier windows; BAM: the packed
    // bytes, (seq_len + 1) / 2 a record
    int store_window(Scratch &sc, const lrge_hip_reads &W, const u32 *d_seq_len, u64 n_use) {
        const bool packed = W.fmt == FX_FMT_BAM;
        u64 sum = 0;
        for (u32 l : W.seq_len) sum += packed ? ((u64)l + 1) / 2 : l;
        if (sum >> 32) return fx_verdict_rc(ctx, FX_UNPROVEN, "a window of 2^32 bytes or more");      // (never: the window is below that)
        // the store doubles while that leaves the block room to double as well; close to the cap it grows by an eighth
        const u64 need = store.keep_len + sum, room = cap > blk->keep_cap ? cap - blk->keep_cap : 0, soft = cap > 2 * blk->keep_cap ? cap - 2 * blk->keep_cap : 0;
        store.keep_max = need <= soft ? soft : std::min<u64>(room, need + need / 8);
        if (!store.keep_reserve(sum)) {
            if (store.keep_over) { LRGE_SET_ERR(ctx, "reads_open: bases and window above INGEST_MAX_BYTES (%llu)", (unsigned long long)cap); return LRGE_ERR_UNPROVEN; }
            LRGE_SET_ERR(ctx, "reads_open: base store: %s", hipGetErrorString(store.e));
            return LRGE_ERR_DEVICE;
        }
        blk->keep_max = cap > store.keep_cap ? cap - store.keep_cap : 0;
        if (W.n) {
            ALLOC_OR_FAIL(d_dst, sc, u32, W.n);
            const dim3 grid((u32)std::min<u64>(W.n, (u64)ctx->n_cu * 32));
            if (packed) {
                hipLaunchKernelGGL(k_bam_spans, dim3((u32)div_up(W.n, 256)), dim3(256), 0, ctx->stream, d_seq_len, W.n, d_dst);
                KCHK(ctx);
                d_seq_len = d_dst;                               // (the scan runs in place, as the record scans' do)
            }
            const int src = scan_exclusive_u32(ctx, sc, d_seq_len, d_dst, W.n, nullptr);
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
    // the input is over and windows were flushed: what is left in the block (d_text, the run's now) is the last window; the
    // store becomes the handle's text, with a record table of its own
    int finish(u8 *d_text, u64 n_text) {
        lrge_hip_ctx *ctx = dev.ctx;
        lrge_hip_reads *R = dev.R;
        DevKeep last(ctx);
        last.keep = d_text; last.keep_len = n_text; last.keep_cap = n_text;
        dev.blk = &last;
        int rc = win.step(true);
        if (rc) return rc;
        if (!dev.store.keep && !dev.store.keep_reserve(0)) { LRGE_SET_ERR(ctx, "reads_open: device allocation failed"); return LRGE_ERR_DEVICE; }
        std::vector<FxRec> tab((size_t)R->n);
        const bool packed = win.fmt == FX_FMT_BAM;              // (the gather of BAM reads its records' spans as it reads the text)
        u64 o = 0;
        for (u64 i = 0; i < R->n; ++i) {
            const u64 span = packed ? ((u64)R->seq_len[i] + 1) / 2 : R->seq_len[i];
            tab[i] = FxRec{0, o, span, (u32)(R->name_off[i + 1] - R->name_off[i]), R->seq_len[i]};
            o += span;
        }
        hipError_t e = hipSuccess;
        if (!(R->d_recs = (FxRec *)ctx->pool.alloc(std::max<size_t>(1, tab.size()) * sizeof(FxRec), &e))) { LRGE_SET_ERR(ctx, "reads_open: record table: %s", hipGetErrorString(e)); return LRGE_ERR_DEVICE; }
        if (!tab.empty()) HIPCHK(ctx, hipMemcpyAsync(R->d_recs, tab.data(), tab.size() * sizeof(FxRec), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        R->d_text = dev.store.keep; R->n_text = dev.store.keep_len; dev.store.keep = nullptr;
        R->fmt = win.fmt;
        R->text_bytes = dev.through + n_text;
        R->win = win.st; R->win.bases = R->n_text;
        R->ms[1] = (float)dev.ms_scan; R->ms[2] = (float)dev.ms_names;
        return LRGE_OK;
    }
};

static void fx_win_attach(FxWinRun *run, DevKeep *blk) { run->attach(blk); }
static int fx_win_stopped(FxWinRun *run) { return run->stopped(); }

// the record scan over R->d_text: fills the table, the lengths and the identifiers.  w: the text is a window (fx_window.h) --
// scanned up to its cut unless it is the last, its bases copied to the store
static int fx_parse_device(lrge_hip_ctx *ctx, lrge_hip_reads *R, FxWinScan *w) {
    const u64 n = R->n_text;
    const u8 *t = R->d_text;
    R->name_off.assign(1, 0);
    if (n == 0) return LRGE_OK;
    hipStream_t st = ctx->stream;
    Scratch sc(ctx);
    ctx->pin_items.clear(); ctx->pin_used = 0;
    const u64 n_tiles = div_up(n, FX_TILE);
    if (n_tiles >> 31) return fx_verdict_rc(ctx, FX_UNPROVEN, "text of 8 TiB or more");
    ALLOC_OR_FAIL(c_lf, sc, u32, n_tiles);
    ALLOC_OR_FAIL(c_rem, sc, u32, n_tiles);
    ALLOC_OR_FAIL(c_hdr, sc, u32, n_tiles);
    ALLOC_OR_FAIL(d_sum, sc, FxSummary, 1);
    hipLaunchKernelGGL(k_fx_census, dim3((u32)n_tiles), dim3(FX_THREADS), 0, st, t, n, c_lf, c_rem, c_hdr);
    KCHK(ctx);
    hipLaunchKernelGGL(k_fx_summary, dim3(1), dim3(FX_THREADS), 0, st, t, n, (const u32 *)c_lf, (const u32 *)c_rem, (const u32 *)c_hdr, n_tiles, d_sum);
    KCHK(ctx);
    FxSummary hs;
    HIPCHK(ctx, ctx->d2h(&hs, d_sum, sizeof hs, st));
    HIPCHK(ctx, ctx->d2h_sync(st));
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
    int rc;
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
    hipError_t e = hipSuccess;
    if (!(R->d_recs = (FxRec *)ctx->pool.alloc((size_t)n_rec * sizeof(FxRec), &e))) { LRGE_SET_ERR(ctx, "reads_open: record table: %s", hipGetErrorString(e)); return LRGE_ERR_DEVICE; }
    ALLOC_OR_FAIL(d_seq_len, sc, u32, n_rec);
    ALLOC_OR_FAIL(d_name_len, sc, u32, n_rec);
    ALLOC_OR_FAIL(d_flags, sc, u64, 2);                   // [0]: verdict bits (low word), [1]: identifier bytes
    HIPCHK(ctx, hipMemsetAsync(d_flags, 0, 16, st));
    const u32 rec_blocks = (u32)div_up(n_rec, FX_THREADS);
    hipLaunchKernelGGL(k_fx_records, dim3(rec_blocks), dim3(FX_THREADS), 0, st, t, n_use, fmt, n_rec, (const u64 *)ls, n_lf, n_lines, l0, (const u64 *)hpos, (const u32 *)hrem,
                       n_rem, R->d_recs, d_seq_len, d_name_len, (u32 *)d_flags, (unsigned long long *)(d_flags + 1));
    KCHK(ctx);
    u64 flags[2] = {0, 0};
    HIPCHK(ctx, ctx->d2h(flags, d_flags, sizeof flags, st));
    HIPCHK(ctx, ctx->d2h_sync(st));
    if ((u32)flags[0]) return fx_verdict_rc(ctx, (u32)flags[0], "a record outside the strict form");
    if (flags[1] >> 32) return fx_verdict_rc(ctx, FX_UNPROVEN, "4 GiB of identifiers or more");
    if ((rc = fx_tables_to_host(ctx, R, sc, n_rec, d_seq_len, d_name_len, flags[1])) || !w) return rc;
    return w->dev->store_window(sc, *R, d_seq_len, n_use);
}

#include "host_bam.inl"      // bam_parse_device: the same for unaligned BAM (needs the struct and the tail above)
#include "host_sam.inl"      // sam_parse_device: the same for unaligned SAM

// ---- text that stays in HBM ----
// any other gzip input: the rounds of gz_run with GzDev keeping every round's bytes on the device (host_gzip.inl: keep_*).
// LRGE_OK with the block in *d_text (the caller's now), LRGE_ERR_UNPROVEN, LRGE_ERR_DEVICE
// run: the call is windowed -- the block is flushed through run->win whenever a round has been appended (DevKeep::keep_flush)
static int gzip_inflate_to_device(lrge_hip_ctx *ctx, const uint8_t *comp, uint64_t comp_len, u64 max_bytes, u8 **d_text, u64 *n_text, FxWinRun *run) {
    const GzCfg cfg = gz_cfg(ctx);
    GzStats st;
    u64 bad = 0;
    GzDev dev(ctx, cfg);
    dev.keep_on = true; dev.keep_max = max_bytes; dev.keep_slack = FX_PAD;
    // a first size: the last member's ISIZE (the whole text of a single-member file below 4 GiB); later rounds grow the block
    if (comp_len >= 18) dev.keep_hint = std::min<u64>(max_bytes, bgzf_u32(comp + comp_len - 4));
    if (run) fx_win_attach(run, &dev);
    const int rc = dev.e == hipSuccess ? gz_run(dev, comp, comp_len, cfg, [&](const uint8_t *, uint64_t) { return true; }, st, &bad) : (int)GZ_RUN_DEVICE;
    (void)hipStreamSynchronize(ctx->stream);
    if (rc == GZ_RUN_OK) {
        if (!dev.keep && !dev.keep_reserve(0)) { LRGE_SET_ERR(ctx, "reads_open: device allocation failed"); return LRGE_ERR_DEVICE; }
        *d_text = dev.keep; *n_text = dev.keep_len; dev.keep = nullptr;
        return LRGE_OK;
    }
    if (run && fx_win_stopped(run)) return fx_win_stopped(run);
    if (dev.keep_over) return fx_over_cap_rc(ctx, max_bytes);
    if (rc == GZ_RUN_DEVICE) {
        LRGE_SET_ERR(ctx, "reads_open: gzip inflate: %s", hipGetErrorString(dev.e != hipSuccess ? dev.e : hipErrorUnknown));
        (void)hipGetLastError();
        return LRGE_ERR_DEVICE;
    }
    LRGE_SET_ERR(ctx, "reads_open: gzip data not proven on the device (status %d near file offset %llu)", rc, (unsigned long long)bad);
    return LRGE_ERR_UNPROVEN;
}

extern "C" void lrge_hip_reads_free(lrge_hip_reads *r) {
    if (!r) return;
    bool ctx_alive;
    { std::lock_guard<std::mutex> g(g_live_mu); ctx_alive = g_live_ctx.count(r->ctx) != 0; }
    if (ctx_alive) { r->ctx->pool.release(r->d_text); r->ctx->pool.release(r->d_recs); }     // (a destroyed context has already freed its pool)
    delete r;
}

extern "C" int lrge_hip_reads_open_mem(lrge_hip_ctx *ctx, const void *file_bytes, uint64_t len, int flags, lrge_hip_reads **out) {
    if (!ctx || !out || (!file_bytes && len)) return LRGE_ERR_INVALID;
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const double t0 = fx_now_ms();
    const u8 *d = (const u8 *)file_bytes;
    std::unique_ptr<lrge_hip_reads, void (*)(lrge_hip_reads *)> guard(new lrge_hip_reads(), lrge_hip_reads_free);
    lrge_hip_reads *R = guard.get();
    R->ctx = ctx;
    const u64 cap = ingest_cap(ctx);
    // LRGE_GPU_INGEST_WINDOWED: text larger than a window passes through the block in windows (fx_window.h)
    const u64 window = std::max<u64>(1, ctx->opt_u64("INGEST_WINDOW_BYTES", std::min<u64>((u64)1 << 30, cap / 4)));
    std::unique_ptr<FxWinRun> run;
    if (flags & LRGE_GPU_INGEST_WINDOWED) run.reset(new FxWinRun(ctx, R, flags, cap, window));
    // a source of the windowed call that appends to a block of the call's own: room for `more` bytes behind what it holds
    DevKeep blk(ctx);
    blk.keep_on = true; blk.keep_max = cap; blk.keep_slack = FX_PAD;
    auto blk_room = [&](u64 more) -> int {
        // (a block that moved was copied on the main stream, and its old bytes are the pool's again: other streams draw from it)
        if (blk.keep_reserve(more)) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); return LRGE_OK; }
        if (blk.keep_over) return fx_over_cap_rc(ctx, cap);
        LRGE_SET_ERR(ctx, "reads_open: device allocation of %llu bytes failed: %s", (unsigned long long)more, hipGetErrorString(blk.e));
        return LRGE_ERR_DEVICE;
    };
    hipError_t e = hipSuccess;
    auto text_block = [&](u64 bytes) -> bool {
        R->d_text = (u8 *)ctx->pool.alloc((size_t)bytes + FX_PAD, &e);
        if (!R->d_text) LRGE_SET_ERR(ctx, "reads_open: device allocation of %llu bytes failed: %s", (unsigned long long)bytes, hipGetErrorString(e));
        return R->d_text != nullptr;
    };
    const auto b = [&](u64 i) -> u32 { return i < len ? d[i] : 0x100u; };
    bool raw_text = false;                      // the file's bytes are the text
    if (b(0) == 0x1f && b(1) == 0x8b) {
        std::vector<BgzfBlock> t;
        uint64_t total = 0;
        if (bgzf_scan_blocks(d, len, &t, &total)) {
            if (!(flags & LRGE_GPU_INFLATE_BGZF)) { ctx->err = "reads_open: BGZF input without LRGE_GPU_INFLATE_BGZF"; return LRGE_ERR_UNPROVEN; }
            BgzfBad bad;                        // the chunk pipeline of host_inflate.inl, decoding into the block
            // BAM and SAM with their flags are not windowed without LRGE_GPU_INGEST_WINDOWED_ALN: the first blocks that hold four
            // bytes of text are decoded for the sniff, and such a file takes the resident branch below exactly as without the
            // windowed flag
            bool windowed = run && total > window;
            if (windowed && (flags & (LRGE_GPU_INGEST_BAM | LRGE_GPU_INGEST_SAM))) {
                std::vector<BgzfBlock> first;
                u64 bytes = 0;
                for (size_t i = 0; i < t.size() && bytes < 4; ++i) { first.push_back(t[i]); bytes += t[i].isize; }
                Scratch sc(ctx);
                ALLOC_OR_FAIL(d_first, sc, u8, bytes + FX_PAD);
                const int rc = bgzf_inflate_chunks(ctx, d, first, nullptr, d_first, "reads_open: bgzf inflate", &bad);
                if (rc) return rc;
                if (bad.status != INF_OK) { ctx->err = "reads_open: a BGZF block failed its checks"; return LRGE_ERR_UNPROVEN; }
                u8 head[4] = {0, 0, 0, 0};
                HIPCHK(ctx, hipMemcpyAsync(head, d_first, (size_t)std::min<u64>(4, bytes), hipMemcpyDeviceToHost, ctx->stream));
                HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
                bool is_bam, is_sam;
                fx_sniff_bam_sam(flags, head, total, &is_bam, &is_sam);
                windowed = !fx_stays_resident(flags, is_bam, is_sam);
            }
            if (windowed) {
                // runs of blocks of a window's size, each decoded behind the tail the window before it left
                run->attach(&blk);
                for (size_t i = 0, j; i < t.size(); i = j) {
                    std::vector<BgzfBlock> part;
                    u64 bytes = 0;
                    for (j = i; j < t.size() && (j == i || bytes < window); ++j) {
                        part.push_back(t[j]);
                        part.back().o_off = blk.keep_len + bytes;
                        bytes += t[j].isize;
                    }
                    int rc = blk_room(bytes);
                    if (rc) return rc;
                    if ((rc = bgzf_inflate_chunks(ctx, d, part, nullptr, blk.keep, "reads_open: bgzf inflate", &bad))) return rc;
                    if (bad.status != INF_OK) { ctx->err = "reads_open: a BGZF block failed its checks"; return LRGE_ERR_UNPROVEN; }
                    blk.keep_len += bytes;
                    if (!run->appended()) return run->stopped();
                }
                R->d_text = blk.keep; R->n_text = blk.keep_len; blk.keep = nullptr;
            } else {
                if (total > cap) return fx_over_cap_rc(ctx, cap);
                if (!text_block(total)) return LRGE_ERR_DEVICE;
                const int rc = bgzf_inflate_chunks(ctx, d, t, nullptr, R->d_text, "reads_open: bgzf inflate", &bad);
                if (rc) return rc;
                if (bad.status != INF_OK) { ctx->err = "reads_open: a BGZF block failed its checks"; return LRGE_ERR_UNPROVEN; }
                R->n_text = total;
            }
        } else {
            if (!(flags & LRGE_GPU_INFLATE_GZIP)) { ctx->err = "reads_open: gzip input without LRGE_GPU_INFLATE_GZIP"; return LRGE_ERR_UNPROVEN; }
            const int rc = gzip_inflate_to_device(ctx, d, len, cap, &R->d_text, &R->n_text, run.get());
            if (rc) return rc;
        }
    } else if (b(0) == 0x42 && b(1) == 0x5a && (flags & LRGE_GPU_INFLATE_BZIP2)) {
        const int rc = bzip2_inflate_to_device(ctx, d, len, cap, FX_PAD, &R->d_text, &R->n_text, run.get());
        if (rc) return rc;
    } else if ((b(0) == 0x42 && b(1) == 0x5a) || (b(0) == 0x28 && b(1) == 0xb5 && b(2) == 0x2f && b(3) == 0xfd) ||
               (b(0) == 0xfd && b(1) == 0x37 && b(2) == 0x7a && b(3) == 0x58 && b(4) == 0x5a)) {
        ctx->err = "reads_open: bzip2, zstd and xz input is decompressed on the host";
        return LRGE_ERR_UNPROVEN;
    } else if (run && len > window && [&] { bool is_bam, is_sam; fx_sniff_bam_sam(flags, d, len, &is_bam, &is_sam); return !fx_stays_resident(flags, is_bam, is_sam); }()) {
        run->attach(&blk);                      // copies of a window's size (BAM and SAM that stay resident: the branch below)
        for (u64 off = 0; off < len; off += window) {
            const u64 m = std::min<u64>(window, len - off);
            const int rc = blk_room(m);
            if (rc) return rc;
            HIPCHK(ctx, hipMemcpyAsync(blk.keep + blk.keep_len, d + off, (size_t)m, hipMemcpyHostToDevice, ctx->stream));
            blk.keep_len += m;
            if (!run->appended()) return run->stopped();
        }
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        R->d_text = blk.keep; R->n_text = blk.keep_len; blk.keep = nullptr; raw_text = !run->win.st.windows;
    } else {
        if (len > cap) return fx_over_cap_rc(ctx, cap);
        if (!text_block(len)) return LRGE_ERR_DEVICE;
        if (len) HIPCHK(ctx, hipMemcpyAsync(R->d_text, d, (size_t)len, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        R->n_text = len; raw_text = true;
    }
    if (run && run->win.st.windows) {           // windows were flushed: the rest of the block is the last, the store the handle's text
        u8 *rest = R->d_text;
        const u64 n_rest = R->n_text;
        R->d_text = nullptr; R->n_text = 0;
        const int rc = run->finish(rest, n_rest);
        if (rc) return rc;
        R->ms[3] = (float)(fx_now_ms() - t0); R->ms[0] = R->ms[3] - R->ms[1] - R->ms[2];
        if (ctx->opt("VERBOSE")) fprintf(stderr, "[lrge_hip] reads_open: %llu text bytes in %llu windows, %llu records, %llu store bytes; record scan %.2f ms, identifiers and lengths %.2f ms\n",
                                        (unsigned long long)R->text_bytes, (unsigned long long)R->win.windows, (unsigned long long)R->n, (unsigned long long)R->n_text, R->ms[1], R->ms[2]);
        *out = guard.release();
        return LRGE_OK;
    }
    R->text_bytes = R->n_text;
    const double t1 = fx_now_ms();
    // BAM and SAM by their magic, when the caller asked for them: the first text bytes are here already for raw input
    bool is_bam = false, is_sam = false;
    if ((flags & (LRGE_GPU_INGEST_BAM | LRGE_GPU_INGEST_SAM)) && R->n_text >= 3) {
        u8 head[4] = {0, 0, 0, 0};
        const size_t k = (size_t)std::min<u64>(4, R->n_text);
        if (raw_text) memcpy(head, d, k);
        else { HIPCHK(ctx, hipMemcpyAsync(head, R->d_text, k, hipMemcpyDeviceToHost, ctx->stream)); HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); }
        fx_sniff_bam_sam(flags, head, R->n_text, &is_bam, &is_sam);
    }
    const int rc = is_bam ? bam_parse_device(ctx, R) : is_sam ? sam_parse_device(ctx, R) : fx_parse_device(ctx, R);
    if (rc) return rc;
    const double t2 = fx_now_ms();
    R->ms[0] = (float)(t1 - t0); R->ms[1] = (float)(t2 - t1) - R->ms[2]; R->ms[3] = (float)(t2 - t0);
    if (ctx->opt("VERBOSE")) fprintf(stderr, "[lrge_hip] reads_open: %llu text bytes, %llu records; text to HBM %.2f ms, record scan %.2f ms, identifiers and lengths %.2f ms\n",
                                    (unsigned long long)R->n_text, (unsigned long long)R->n, R->ms[0], R->ms[1], R->ms[2]);
    *out = guard.release();
    return LRGE_OK;
}

extern "C" int lrge_hip_reads_open(lrge_hip_ctx *ctx, const char *path, int flags, lrge_hip_reads **out) {
    if (!ctx || !path || !out) return LRGE_ERR_INVALID;
    *out = nullptr;
    std::string raw;
    try { raw = lrge::io::slurp(path); } catch (const std::exception &e) { ctx->err = e.what(); return LRGE_ERR_IO; }
    return lrge_hip_reads_open_mem(ctx, raw.data(), raw.size(), flags, out);
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
