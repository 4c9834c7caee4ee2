// host_fastx.inl -- read sets built on the device from FASTA / FASTQ text (k_fastx.h), from unaligned BAM
// (k_bam.h, host_bam.inl) and from unaligned SAM (k_sam.h, host_sam.inl): the text reaches HBM
// decompressed (BGZF chunks decoded into one block by the pipeline of host_inflate.inl, the gzip and bzip2 rounds appended device-to-device, plain input copied once), the
// record scan runs there, only identifiers and lengths come back, and lrge_hip_seqset_from_reads gathers the selected reads
// into dense ASCII for the device-source pack of host_seqset.inl.  Whatever the scan cannot prove is LRGE_ERR_UNPROVEN: the
// caller takes lrge_hip_read_records*, which parses the file or reports it with the reference's messages.  Included into
// lrge_hip.hip.

struct lrge_hip_reads {
    lrge_hip_ctx *ctx = nullptr;
    u8 *d_text = nullptr; u64 n_text = 0;       // the decompressed text (FX_PAD bytes of slack behind it)
    FxRec *d_recs = nullptr; u64 n = 0;
    int fmt = FX_FMT_EMPTY;
    std::vector<u32> seq_len;
    std::vector<u64> name_off;                  // [n + 1]
    std::string names;
    float ms[4] = {0, 0, 0, 0};                 // text to HBM, record scan, identifiers and lengths to the host, the whole call
    BamStats bam = {0, 0, 0, 0, 0, 0};          // fmt == FX_FMT_BAM: the counts of the record scan (lrge_hip_reads_bam_stats)
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

// the record scan over R->d_text: fills the table, the lengths and the identifiers
static int fx_parse_device(lrge_hip_ctx *ctx, lrge_hip_reads *R) {
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
    u32 verdict = 0;
    const int fmt = fx_format(n, c, &verdict);
    if (verdict) return fx_verdict_rc(ctx, verdict, "neither FASTA nor FASTQ by its first line");
    R->fmt = fmt;
    if (fmt == FX_FMT_EMPTY) return LRGE_OK;
    if ((verdict = fx_limits(fmt, c))) return fx_verdict_rc(ctx, verdict, "line or header count");
    u64 *ls = nullptr, *d_lines = nullptr, *hpos = nullptr;
    u32 *hrem = nullptr;
    u64 n_rec = 0, n_lines = 0, l0 = 0;
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
    }
    if (n_rec >> 32) return fx_verdict_rc(ctx, FX_TOO_MANY, "records");
    hipError_t e = hipSuccess;
    if (!(R->d_recs = (FxRec *)ctx->pool.alloc((size_t)n_rec * sizeof(FxRec), &e))) { LRGE_SET_ERR(ctx, "reads_open: record table: %s", hipGetErrorString(e)); return LRGE_ERR_DEVICE; }
    ALLOC_OR_FAIL(d_seq_len, sc, u32, n_rec);
    ALLOC_OR_FAIL(d_name_len, sc, u32, n_rec);
    ALLOC_OR_FAIL(d_flags, sc, u64, 2);                   // [0]: verdict bits (low word), [1]: identifier bytes
    HIPCHK(ctx, hipMemsetAsync(d_flags, 0, 16, st));
    const u32 rec_blocks = (u32)div_up(n_rec, FX_THREADS);
    hipLaunchKernelGGL(k_fx_records, dim3(rec_blocks), dim3(FX_THREADS), 0, st, t, n, fmt, n_rec, (const u64 *)ls, c.n_lf, n_lines, l0, (const u64 *)hpos, (const u32 *)hrem,
                       c.n_rem, R->d_recs, d_seq_len, d_name_len, (u32 *)d_flags, (unsigned long long *)(d_flags + 1));
    KCHK(ctx);
    u64 flags[2] = {0, 0};
    HIPCHK(ctx, ctx->d2h(flags, d_flags, sizeof flags, st));
    HIPCHK(ctx, ctx->d2h_sync(st));
    if ((u32)flags[0]) return fx_verdict_rc(ctx, (u32)flags[0], "a record outside the strict form");
    if (flags[1] >> 32) return fx_verdict_rc(ctx, FX_UNPROVEN, "4 GiB of identifiers or more");
    return fx_tables_to_host(ctx, R, sc, n_rec, d_seq_len, d_name_len, flags[1]);
}

#include "host_bam.inl"      // bam_parse_device: the same for unaligned BAM (needs the struct and the tail above)
#include "host_sam.inl"      // sam_parse_device: the same for unaligned SAM

// ---- text that stays in HBM ----
// any other gzip input: the rounds of gz_run with GzDev keeping every round's bytes on the device (host_gzip.inl: keep_*).
// LRGE_OK with the block in *d_text (the caller's now), LRGE_ERR_UNPROVEN, LRGE_ERR_DEVICE
static int gzip_inflate_to_device(lrge_hip_ctx *ctx, const uint8_t *comp, uint64_t comp_len, u64 max_bytes, u8 **d_text, u64 *n_text) {
    const GzCfg cfg = gz_cfg(ctx);
    GzStats st;
    u64 bad = 0;
    GzDev dev(ctx, cfg);
    dev.keep_on = true; dev.keep_max = max_bytes; dev.keep_slack = FX_PAD;
    // a first size: the last member's ISIZE (the whole text of a single-member file below 4 GiB); later rounds grow the block
    if (comp_len >= 18) dev.keep_hint = std::min<u64>(max_bytes, bgzf_u32(comp + comp_len - 4));
    const int rc = dev.e == hipSuccess ? gz_run(dev, comp, comp_len, cfg, [&](const uint8_t *, uint64_t) { return true; }, st, &bad) : (int)GZ_RUN_DEVICE;
    (void)hipStreamSynchronize(ctx->stream);
    if (rc == GZ_RUN_OK) {
        if (!dev.keep && !dev.keep_reserve(0)) { LRGE_SET_ERR(ctx, "reads_open: device allocation failed"); return LRGE_ERR_DEVICE; }
        *d_text = dev.keep; *n_text = dev.keep_len; dev.keep = nullptr;
        return LRGE_OK;
    }
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
            if (total > cap) return fx_over_cap_rc(ctx, cap);
            if (!text_block(total)) return LRGE_ERR_DEVICE;
            BgzfBad bad;                        // the chunk pipeline of host_inflate.inl, decoding into the block
            const int rc = bgzf_inflate_chunks(ctx, d, t, nullptr, R->d_text, "reads_open: bgzf inflate", &bad);
            if (rc) return rc;
            if (bad.status != INF_OK) { ctx->err = "reads_open: a BGZF block failed its checks"; return LRGE_ERR_UNPROVEN; }
            R->n_text = total;
        } else {
            if (!(flags & LRGE_GPU_INFLATE_GZIP)) { ctx->err = "reads_open: gzip input without LRGE_GPU_INFLATE_GZIP"; return LRGE_ERR_UNPROVEN; }
            const int rc = gzip_inflate_to_device(ctx, d, len, cap, &R->d_text, &R->n_text);
            if (rc) return rc;
        }
    } else if (b(0) == 0x42 && b(1) == 0x5a && (flags & LRGE_GPU_INFLATE_BZIP2)) {
        const int rc = bzip2_inflate_to_device(ctx, d, len, cap, FX_PAD, &R->d_text, &R->n_text);
        if (rc) return rc;
    } else if ((b(0) == 0x42 && b(1) == 0x5a) || (b(0) == 0x28 && b(1) == 0xb5 && b(2) == 0x2f && b(3) == 0xfd) ||
               (b(0) == 0xfd && b(1) == 0x37 && b(2) == 0x7a && b(3) == 0x58 && b(4) == 0x5a)) {
        ctx->err = "reads_open: bzip2, zstd and xz input is decompressed on the host";
        return LRGE_ERR_UNPROVEN;
    } else {
        if (len > cap) return fx_over_cap_rc(ctx, cap);
        if (!text_block(len)) return LRGE_ERR_DEVICE;
        if (len) HIPCHK(ctx, hipMemcpyAsync(R->d_text, d, (size_t)len, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        R->n_text = len; raw_text = true;
    }
    const double t1 = fx_now_ms();
    // BAM and SAM by their magic, when the caller asked for them: the first text bytes are here already for raw input
    bool is_bam = false, is_sam = false;
    if ((flags & (LRGE_GPU_INGEST_BAM | LRGE_GPU_INGEST_SAM)) && R->n_text >= 3) {
        u8 head[4] = {0, 0, 0, 0};
        const size_t k = (size_t)std::min<u64>(4, R->n_text);
        if (raw_text) memcpy(head, d, k);
        else { HIPCHK(ctx, hipMemcpyAsync(head, R->d_text, k, hipMemcpyDeviceToHost, ctx->stream)); HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); }
        is_bam = (flags & LRGE_GPU_INGEST_BAM) && R->n_text >= 4 && head[0] == 'B' && head[1] == 'A' && head[2] == 'M' && head[3] == 1;
        is_sam = (flags & LRGE_GPU_INGEST_SAM) && sam_sniff(head, R->n_text);
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
extern "C" uint64_t lrge_hip_reads_text_bytes(const lrge_hip_reads *r) { return r ? r->n_text : 0; }

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
