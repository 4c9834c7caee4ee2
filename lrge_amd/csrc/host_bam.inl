// host_bam.inl -- the record scan of unaligned BAM text in HBM (k_bam.h): the header, a candidate start per
// segment, the walks, the repair rounds that bam_chain_plan (bam_core.h) asks for, then the table.  Between the rounds only the
// segment summaries travel (24 B a segment).  Included into host_fastx.inl, whose tail (fx_tables_to_host) brings the
// identifiers and the lengths down.

static_assert(sizeof(lrge_hip_bam_stats) == sizeof(BamStats), "lrge_hip_bam_stats is BamStats");

static dim3 bam_walker_grid(lrge_hip_ctx *ctx, u64 n_items) {            // (k_bam.h: walker i is lane i / grid of workgroup i % grid)
    return dim3((u32)std::max<u64>(div_up(n_items, 64), std::min<u64>(n_items, (u64)ctx->n_cu * 8)));
}

static int bam_parse_device(lrge_hip_ctx *ctx, lrge_hip_reads *R) {
    const u64 n = R->n_text;
    const u8 *t = R->d_text;
    hipStream_t st = ctx->stream;
    Scratch sc(ctx);
    R->name_off.assign(1, 0);
    R->bam = BamStats{0, 0, 0, 0, 0, 0};
    ALLOC_OR_FAIL(d_hdr, sc, BamHeader, 1);
    hipLaunchKernelGGL(k_bam_header, dim3(1), dim3(64), 0, st, t, n, d_hdr);
    KCHK(ctx);
    BamHeader hdr;
    HIPCHK(ctx, hipMemcpyAsync(&hdr, d_hdr, sizeof hdr, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (hdr.verdict) return fx_verdict_rc(ctx, hdr.verdict, "BAM header");
    R->fmt = FX_FMT_BAM;
    const u64 hdr_end = hdr.hdr_end;
    if (hdr_end == n) return LRGE_OK;                                   // no record: an empty read set, as on the host
    const u64 S = std::max<u64>(64, ctx->opt_u64("BAM_SEGMENT_BYTES", (u64)256 << 10));
    const u64 n_seg = div_up(n - hdr_end, S);
    if (n_seg >> 31) return fx_verdict_rc(ctx, FX_UNPROVEN, "2^31 BAM segments or more");
    ALLOC_OR_FAIL(d_cand, sc, u64, n_seg);
    ALLOC_OR_FAIL(d_seg, sc, BamSeg, n_seg);
    ALLOC_OR_FAIL(d_list, sc, u32, n_seg);
    ALLOC_OR_FAIL(d_from, sc, u64, n_seg + 1);                          // (later: the table bases, one more than segments)
    std::vector<u64> cand((size_t)n_seg), from((size_t)n_seg + 1);
    std::vector<BamSeg> seg((size_t)n_seg), got((size_t)n_seg);
    std::vector<u32> list((size_t)n_seg);
    // round 0: every segment from its candidate
    hipLaunchKernelGGL(k_bam_find, dim3((u32)n_seg), dim3(64), 0, st, t, n, hdr_end, S, d_cand);
    KCHK(ctx);
    hipLaunchKernelGGL(k_bam_walk, bam_walker_grid(ctx, n_seg), dim3(64), 0, st, t, n, hdr_end, S, (const u32 *)nullptr, (const u64 *)nullptr, (const u64 *)d_cand, n_seg, d_seg);
    KCHK(ctx);
    HIPCHK(ctx, hipMemcpyAsync(cand.data(), d_cand, (size_t)n_seg * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(seg.data(), d_seg, (size_t)n_seg * sizeof(BamSeg), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    cand[0] = BAM_NONE;
    // repair rounds
    for (;;) {
        u32 verdict = 0;
        const u64 k = bam_chain_plan(seg.data(), n_seg, hdr_end, S, n, list.data(), from.data(), &verdict);
        if (verdict) return fx_verdict_rc(ctx, verdict, "the BAM record chain");
        if (!k) break;
        ++R->bam.repair_rounds; R->bam.rewalked_segments += k;
        HIPCHK(ctx, hipMemcpyAsync(d_list, list.data(), (size_t)k * 4, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(d_from, from.data(), (size_t)k * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_bam_walk, bam_walker_grid(ctx, k), dim3(64), 0, st, t, n, hdr_end, S, (const u32 *)d_list, (const u64 *)d_from, (const u64 *)nullptr, k, d_seg);
        KCHK(ctx);
        HIPCHK(ctx, hipMemcpyAsync(got.data(), d_seg, (size_t)k * sizeof(BamSeg), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        for (u64 i = 0; i < k; ++i) seg[list[i]] = got[i];
    }
    bam_chain_stats(seg.data(), cand.data(), n_seg, &R->bam);
    // the table: every segment again from its proven start, at the exclusive scan of the counts
    u64 n_rec = 0;
    for (u64 s = 0; s < n_seg; ++s) { from[s] = n_rec; n_rec += seg[s].count; cand[s] = seg[s].start; }
    from[n_seg] = n_rec;
    if (n_rec >> 32) return fx_verdict_rc(ctx, FX_TOO_MANY, "records");
    hipError_t e = hipSuccess;
    if (!(R->d_recs = (FxRec *)ctx->pool.alloc((size_t)std::max<u64>(1, n_rec) * sizeof(FxRec), &e))) {
        LRGE_SET_ERR(ctx, "reads_open: record table: %s", hipGetErrorString(e));
        return LRGE_ERR_DEVICE;
    }
    ALLOC_OR_FAIL(d_seq_len, sc, u32, std::max<u64>(1, n_rec));
    ALLOC_OR_FAIL(d_name_len, sc, u32, std::max<u64>(1, n_rec));
    ALLOC_OR_FAIL(d_flags, sc, u64, 2);                   // [0]: verdict bits (low word), [1]: identifier bytes
    HIPCHK(ctx, hipMemsetAsync(d_flags, 0, 16, st));
    HIPCHK(ctx, hipMemcpyAsync(d_cand, cand.data(), (size_t)n_seg * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_from, from.data(), ((size_t)n_seg + 1) * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bam_records, bam_walker_grid(ctx, n_seg), dim3(64), 0, st, t, n, hdr_end, S, (const u64 *)d_cand, (const u64 *)d_from, n_seg, R->d_recs, d_seq_len,
                       d_name_len, (u32 *)d_flags, (unsigned long long *)(d_flags + 1));
    KCHK(ctx);
    u64 flags[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(flags, d_flags, sizeof flags, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));                 // (cand and from are pageable: their copies are done)
    if ((u32)flags[0]) return fx_verdict_rc(ctx, (u32)flags[0], "a BAM record changed between the walks");
    if (flags[1] >> 32) return fx_verdict_rc(ctx, FX_UNPROVEN, "4 GiB of identifiers or more");
    return fx_tables_to_host(ctx, R, sc, n_rec, d_seq_len, d_name_len, flags[1]);
}

extern "C" int lrge_hip_reads_bam_stats(const lrge_hip_reads *r, lrge_hip_bam_stats *out) {
    if (!r || !out || r->fmt != FX_FMT_BAM) return LRGE_ERR_INVALID;
    memcpy(out, &r->bam, sizeof *out);
    return LRGE_OK;
}
