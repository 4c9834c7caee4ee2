// host_bam.inl -- the record scan of unaligned BAM text in HBM (k_bam.h): the device backend of bam_run
// (bam_round.h), which drives the header, a candidate start per segment, the walks, the repair rounds and then the table, here
// and in the host twin alike.  Between the rounds only the segment summaries travel (24 B a segment).  Included into
// host_fastx.inl, whose tail (fx_scan_tail) takes the table from there.

#include "bam_round.h"

static_assert(sizeof(lrge_hip_bam_stats) == sizeof(BamStats), "lrge_hip_bam_stats is BamStats");

static dim3 bam_walker_grid(lrge_hip_ctx *ctx, u64 n_items) {            // (k_bam.h: walker i is lane i / grid of workgroup i % grid)
    return dim3((u32)std::max<u64>(div_up(n_items, 64), std::min<u64>(n_items, (u64)ctx->n_cu * 8)));
}

// the backend of bam_run: the text in HBM, every pass a kernel; between the passes only what the driver reads or gives travels
namespace {
struct BamDev {
    lrge_hip_ctx *ctx; lrge_hip_reads *R; Scratch &sc;
    const u8 *t; u64 n; hipStream_t st;                                 // the text, the stream of every step
    u64 hdr_end = 0, S = 0;                                             // (round0 sets them)
    u64 *d_cand = nullptr, *d_from = nullptr;                           // (d_from: later the table bases, one more than segments)
    BamSeg *d_seg = nullptr;
    u32 *d_list = nullptr, *d_seq_len = nullptr, *d_name_len = nullptr;
    bool count_bases = false;                                           // a run that does not keep all: f[2] is the sum of the lengths
    u64 f[3] = {0, 0, 0};                                               // the flag words records() brought back (fx_flags_back)

    int header(u64 *he, u32 *verdict) {
        ALLOC_OR_FAIL(d_hdr, sc, BamHeader, 1);
        hipLaunchKernelGGL(k_bam_header, dim3(1), dim3(64), 0, st, t, n, d_hdr);
        KCHK(ctx);
        BamHeader hdr;
        HIPCHK(ctx, hipMemcpyAsync(&hdr, d_hdr, sizeof hdr, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        *he = hdr.hdr_end; *verdict = hdr.verdict;
        return LRGE_OK;
    }
    u32 tail = 0;                                                       // (round0 sets it: a window's walks, bam_core.h)
    int round0(u64 he, u64 seg_bytes, u64 n_seg, bool tail_mode, u64 *cand, BamSeg *seg) {
        hdr_end = he; S = seg_bytes; tail = tail_mode;
        if (!(d_cand = sc.get<u64>(n_seg)) || !(d_seg = sc.get<BamSeg>(n_seg)) || !(d_list = sc.get<u32>(n_seg)) || !(d_from = sc.get<u64>(n_seg + 1))) return LRGE_ERR_DEVICE;
        hipLaunchKernelGGL(k_bam_find, dim3((u32)n_seg), dim3(64), 0, st, t, n, hdr_end, S, d_cand);
        KCHK(ctx);
        hipLaunchKernelGGL(k_bam_walk, bam_walker_grid(ctx, n_seg), dim3(64), 0, st, t, n, hdr_end, S, (const u32 *)nullptr, (const u64 *)nullptr, (const u64 *)d_cand, n_seg, tail, d_seg);
        KCHK(ctx);
        HIPCHK(ctx, hipMemcpyAsync(cand, d_cand, (size_t)n_seg * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(seg, d_seg, (size_t)n_seg * sizeof(BamSeg), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        return LRGE_OK;
    }
    int rewalk(const u32 *list, const u64 *from, u64 k, BamSeg *got) {
        HIPCHK(ctx, hipMemcpyAsync(d_list, list, (size_t)k * 4, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(d_from, from, (size_t)k * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_bam_walk, bam_walker_grid(ctx, k), dim3(64), 0, st, t, n, hdr_end, S, (const u32 *)d_list, (const u64 *)d_from, (const u64 *)nullptr, k, tail, d_seg);
        KCHK(ctx);
        HIPCHK(ctx, hipMemcpyAsync(got, d_seg, (size_t)k * sizeof(BamSeg), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        return LRGE_OK;
    }
    int records(const u64 *start, const u64 *base, u64 n_seg, u64 n_rec, u64 cut, u32 *flags, u64 *name_bytes) {
        const int rc = fx_alloc_recs(ctx, R, std::max<u64>(1, n_rec));
        if (rc) return rc;
        if (!(d_seq_len = sc.get<u32>(std::max<u64>(1, n_rec))) || !(d_name_len = sc.get<u32>(std::max<u64>(1, n_rec)))) return LRGE_ERR_DEVICE;
        ALLOC_OR_FAIL(d_flags, sc, u64, 3);                   // [0]: verdict bits (low word), [1]: identifier bytes, [2]: bases (count_bases)
        HIPCHK(ctx, hipMemsetAsync(d_flags, 0, 24, st));
        HIPCHK(ctx, hipMemcpyAsync(d_cand, start, (size_t)n_seg * 8, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(d_from, base, ((size_t)n_seg + 1) * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_bam_records, bam_walker_grid(ctx, n_seg), dim3(64), 0, st, t, n, hdr_end, S, (const u64 *)d_cand, (const u64 *)d_from, n_seg, cut, R->d_recs, d_seq_len,
                           d_name_len, (u32 *)d_flags, (unsigned long long *)(d_flags + 1));
        KCHK(ctx);
        const int frc = fx_flags_back(ctx, count_bases, d_flags, d_seq_len, n_rec, f);      // (the stream is synchronised: start and base are pageable, their copies are done)
        *flags = (u32)f[0]; *name_bytes = f[1];
        return frc;
    }
};
}  // namespace

// w: the text is a window (fx_window.h) -- only the first has a header, one that is not the last is scanned
// up to its cut (w->cut; 0: there is none yet), and the packed bases of its records go to the store.  A run that does not keep all
// (the census and the selected open) brings neither the tables to the host nor the window to the store: the bases
// are counted behind k_bam_records, the seek map takes its points, and FxWinDev::keep_window keeps the chosen records
static int bam_parse_device(lrge_hip_ctx *ctx, lrge_hip_reads *R, FxWinScan *w) {
    Scratch sc(ctx);
    R->name_off.assign(1, 0);
    BamDev dev{ctx, R, sc, R->d_text, R->n_text, ctx->stream};
    dev.count_bases = fx_scan_selects(w);
    const u64 S = std::max<u64>(64, ctx->opt_u64("BAM_SEGMENT_BYTES", (u64)256 << 10));
    u64 n_rec = 0, name_bytes = 0;
    const char *refused = nullptr;
    const int v = bam_run(dev, R->n_text, S, &R->bam, &n_rec, &name_bytes, &refused, !w || w->first, w && !w->end ? &w->cut : nullptr);
    if (v == BAM_RUN_DEVICE) return LRGE_ERR_DEVICE;                   // (the step that failed has left its message)
    if (v) return fx_verdict_rc(ctx, (u32)v, refused);
    R->fmt = FX_FMT_BAM;                                                // (a refused file leaves no read set, so no format either)
    if (!n_rec) return LRGE_OK;                                         // the header ends the text, or the window has no whole record yet
    // (bam_run has judged the verdict word, with its own message; the prefix's end is for the seek map: the packed copies take whole records)
    return fx_scan_tail(ctx, R, sc, w, dev.f, nullptr, dev.d_seq_len, dev.d_name_len, n_rec, w && !w->end ? w->cut : R->n_text);
}

extern "C" int lrge_hip_reads_bam_stats(const lrge_hip_reads *r, lrge_hip_bam_stats *out) {
    if (!r || !out || r->fmt != FX_FMT_BAM) return LRGE_ERR_INVALID;
    memcpy(out, &r->bam, sizeof *out);
    return LRGE_OK;
}
