// host_sam.inl -- the record scan of unaligned SAM text in HBM (k_sam.h): the line table by the census and
// scatter passes of the FASTQ scan, a mark and a rank per line, then a wavefront per record line.  Included into host_fastx.inl,
// whose tail (fx_scan_tail) takes the table from there.

// the caller has seen the SAM magic at the start of R->d_text, or of the first window.
// w: the text is a window (fx_window.h).  One that is not the last is cut directly behind its last line feed
// (w->cut; 0: it has none yet) and the prefix is scanned as a complete text of that size with the window's own line table: all
// its line feeds lie in the prefix, whose last line is the empty one behind the cut.  The bases go to the store.  A run that does
// not keep all (the census and the selected open) brings neither the tables to the host nor the window to the
// store: the bases are counted behind k_sam_records, the seek map takes its points (a record starts at the first byte of its line),
// and FxWinDev::keep_window keeps the chosen records by its unpacked branch -- a SAM sequence is one line, seq_span == seq_len
static int sam_parse_device(lrge_hip_ctx *ctx, lrge_hip_reads *R, FxWinScan *w) {
    u64 n = R->n_text;
    const u8 *t = R->d_text;
    R->name_off.assign(1, 0);
    hipStream_t st = ctx->stream;
    Scratch sc(ctx);
    // the line starts, as for FASTQ
    FxTiles tl;
    int rc = fx_census_device(ctx, sc, t, n, &tl);
    if (rc) return rc;
    const auto &[n_tiles, c_lf, c_rem, c_hdr, hs] = tl;
    FxCensus c;
    memset(&c, 0, sizeof c);
    c.n_lf = hs.n_lf; c.first = hs.first; c.last = hs.last;
    u32 verdict = fx_limits(FX_FMT_FASTQ, c);
    if (!verdict && (c.n_lf + 1) >> 32) verdict = FX_UNPROVEN;
    if (verdict) return fx_verdict_rc(ctx, verdict, "line count");
    const u64 n_lines = c.n_lf + 1;                         // (the last one is empty when the text ends with a line feed)
    if ((rc = scan_exclusive_u32(ctx, sc, c_lf, c_lf, n_tiles, nullptr))) return rc;
    ALLOC_OR_FAIL(ls, sc, u64, n_lines);
    ALLOC_OR_FAIL(d_lines, sc, u64, 2);
    hipLaunchKernelGGL(k_fx_scatter, dim3((u32)n_tiles), dim3(FX_THREADS), 0, st, t, n, (int)FX_FMT_FASTQ, (const u32 *)c_lf, (const u32 *)c_rem, (const u32 *)c_hdr, c.first,
                       c.last, ls, d_lines, (u64 *)nullptr, (u32 *)nullptr);
    KCHK(ctx);
    if (w && !w->end) {
        if (!c.n_lf) { R->fmt = FX_FMT_SAM; return LRGE_OK; }
        HIPCHK(ctx, ctx->d2h(&n, ls + c.n_lf, 8, st));
        HIPCHK(ctx, ctx->d2h_sync(st));
        w->cut = n;
    }
    // which lines carry a record, and the rank of each
    ALLOC_OR_FAIL(d_mark, sc, u32, n_lines);
    ALLOC_OR_FAIL(d_rank, sc, u32, n_lines);
    ALLOC_OR_FAIL(d_flags, sc, u64, 3);                   // [0]: verdict bits (low word), [1]: identifier bytes, [2]: records (low word), later the bases
    HIPCHK(ctx, hipMemsetAsync(d_flags, 0, 24, st));
    hipLaunchKernelGGL(k_sam_mark, dim3((u32)div_up(n_lines, SAM_THREADS)), dim3(SAM_THREADS), 0, st, t, n, (const u64 *)ls, c.n_lf, n_lines, d_mark);
    KCHK(ctx);
    if ((rc = scan_exclusive_u32(ctx, sc, d_mark, d_rank, n_lines, (u32 *)(d_flags + 2)))) return rc;
    u64 n_rec = 0;
    HIPCHK(ctx, ctx->d2h(&n_rec, d_flags + 2, 8, st));
    HIPCHK(ctx, ctx->d2h_sync(st));
    if (!n_rec) { R->fmt = FX_FMT_SAM; return LRGE_OK; }    // header lines only: the host returns no record
    if ((rc = fx_alloc_recs(ctx, R, n_rec))) return rc;
    if (fx_scan_selects(w)) HIPCHK(ctx, hipMemsetAsync(d_flags + 2, 0, 8, st));      // (the record count is on the host: the word now sums the bases)
    ALLOC_OR_FAIL(d_seq_len, sc, u32, n_rec);
    ALLOC_OR_FAIL(d_name_len, sc, u32, n_rec);
    const u32 grid = (u32)std::min<u64>(div_up(n_lines, SAM_WAVES), (u64)ctx->n_cu * 8);
    hipLaunchKernelGGL(k_sam_records, dim3(grid), dim3(SAM_THREADS), 0, st, t, n, (const u64 *)ls, c.n_lf, n_lines, (const u32 *)d_mark, (const u32 *)d_rank, R->d_recs,
                       d_seq_len, d_name_len, (u32 *)d_flags, (unsigned long long *)(d_flags + 1));
    KCHK(ctx);
    u64 f[3];
    if ((rc = fx_flags_back(ctx, fx_scan_selects(w), d_flags, d_seq_len, n_rec, f))) return rc;
    R->fmt = FX_FMT_SAM;                                    // (a refused file leaves no read set: whoever called drops the handle with its format)
    return fx_scan_tail(ctx, R, sc, w, f, "a SAM record line outside the strict form", d_seq_len, d_name_len, n_rec, n);
}
