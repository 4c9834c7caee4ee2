// host_paf.inl -- part of lrge_hip.hip: overlaps.paf written on the device.  lrge_hip_paf_text runs the
// statistics and the chains job with the records kept in HBM, measures every line (k_paf_measure: dv code, its proof, the length),
// and writes the text slice by slice (scan_exclusive_u32, k_paf_write) into two pinned pieces that reach the caller's sink as whole
// lines.  The bytes are those of lrge::paf_lines / paf.paf_lines, or the call is LRGE_ERR_UNPROVEN and nothing was delivered.

enum { PAF_S_LINES = 0, PAF_S_BYTES, PAF_S_CHAIN_RUNS, PAF_S_SLICES, PAF_S_PIECES, PAF_S_RECORDS, PAF_S_UNPROVEN, PAF_S_FORMAT_US };
enum { PAF_P_STATS = 0, PAF_P_CHAINS, PAF_P_MEASURE, PAF_P_WRITE, PAF_P_COPY, PAF_P_SINK, PAF_P_TOTAL, PAF_P_SETUP };

static u64 paf_now_us() { return (u64)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// one name table: offsets ascend (else LRGE_ERR_INVALID); *longest: the longest identifier
static int paf_check_names(lrge_hip_ctx *ctx, const char *what, const char *names, const uint64_t *off, u32 n, u64 *longest) {
    *longest = 0;
    if (!off || (!names && n && off[n] > off[0])) { LRGE_SET_ERR(ctx, "paf_text: no %s name table", what); return LRGE_ERR_INVALID; }
    for (u32 r = 0; r < n; ++r) {
        if (off[r + 1] < off[r]) { LRGE_SET_ERR(ctx, "paf_text: %s name offsets do not ascend at read %u", what, r); return LRGE_ERR_INVALID; }
        *longest = std::max<u64>(*longest, off[r + 1] - off[r]);
    }
    return LRGE_OK;
}

// The two pinned pieces, the events behind their copies, and the order in which they may go: both streams are drained first.
struct PafPieces {
    lrge_hip_ctx *ctx;
    u8 *pin[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    explicit PafPieces(lrge_hip_ctx *c) : ctx(c) {}
    ~PafPieces() {
        (void)hipStreamSynchronize(ctx->stream); (void)hipStreamSynchronize(ctx->stream2);
        for (int b = 0; b < 2; ++b) { if (pin[b]) (void)hipHostFree(pin[b]); if (ev[b]) (void)hipEventDestroy(ev[b]); }
        (void)hipGetLastError();
    }
};

// One chains run of the whole call into the caller's device buffer: the index, or its parts one after the other (records carry the
// read's index in the whole set, the counter goes on counting).  *found: the chains there are, also beyond `cap`.
static int paf_chain_run(lrge_hip_ctx *ctx, const lrge_hip_index *ix, const lrge_hip_seqset *queries, int dual, lrge_hip_chain *d_rec, u64 cap,
                         unsigned long long *d_cnt, const u32 *d_hc_global, u64 *found) {
    HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, 8, ctx->stream));
    OverlapJob job; job.mode = MODE_TWOSET; job.dual = dual ? 1 : 0;
    job.prm = lrge_hip_params{0, 0.2f};
    job.d_chain_buf = d_rec; job.d_chain_cnt = d_cnt; job.chain_cap = cap; job.n_chains = found;
    if (ix->parts.empty()) return run_overlap(ctx, ix, queries, job);
    StageAcc acc;
    acc.parts = ix->parts.size();
    for (size_t pi = 0; pi < ix->parts.size(); ++pi) {
        OverlapJob j = job;
        j.d_hc_global = d_hc_global; j.rid_base = ix->part_r0[pi];
        const int rc = run_overlap(ctx, ix->parts[pi], queries, j);
        acc.add(ctx);
        if (rc) return rc;
    }
    acc.store(ctx);
    return LRGE_OK;
}

extern "C" int lrge_hip_paf_text(lrge_hip_ctx *ctx, const lrge_hip_index *ix, const lrge_hip_seqset *queries, int dual, const char *q_names,
                                 const uint64_t *q_name_off, const char *t_names, const uint64_t *t_name_off, uint64_t chain_hint,
                                 int (*sink)(void *user, const void *bytes, uint64_t n), void *user) {
    int rc = check_common(ctx, ix, queries, /*parts_ok=*/true);
    if (rc) return rc;
    memset(ctx->paf_stats, 0, sizeof ctx->paf_stats); memset(ctx->paf_phase_us, 0, sizeof ctx->paf_phase_us);
    if (!sink) { LRGE_SET_ERR(ctx, "paf_text: no sink"); return LRGE_ERR_INVALID; }
    const u32 nq = queries->n, nt = ix->seqs->n;
    // ---- the refusals in front of any device work ----
    u64 q_longest = 0, t_longest = 0;
    rc = paf_check_names(ctx, "query", q_names, q_name_off, nq, &q_longest);
    if (!rc) rc = paf_check_names(ctx, "target", t_names, t_name_off, nt, &t_longest);
    if (rc) return rc;
    const u64 name_max = ctx->opt_u64("PAF_NAME_MAX_BYTES", 1024);
    if (q_longest > name_max || t_longest > name_max) {
        LRGE_SET_ERR(ctx, "paf_text: an identifier of %llu bytes (PAF_NAME_MAX_BYTES %llu)", (unsigned long long)std::max(q_longest, t_longest), (unsigned long long)name_max);
        return LRGE_ERR_UNPROVEN;
    }
    if (nq == 0 || nt == 0) return LRGE_OK;
    if (!queries->d_len || !ix->seqs->d_len) { LRGE_SET_ERR(ctx, "paf_text: a read set without device lengths"); return LRGE_ERR_INVALID; }
    const bool parts = !ix->parts.empty();
    if (parts && queries->total_bases + 1 >= (1ULL << 32)) { LRGE_SET_ERR(ctx, "chains against a partitioned index: query set too large"); return LRGE_ERR_TOO_MANY; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool serial = ctx->opt_u64("PAF_SERIAL", 0) != 0;      // (bench only, tools/paf_bench.py: every slice is written, copied and delivered before the next begins, so the host clock splits the phases)
    const u64 t_begin = paf_now_us();
    u64 *ph = ctx->paf_phase_us;
    Scratch sc(ctx);

    // ---- 1. statistics: rl, sum_span, n_kept per query, as lrge_hip_paf_stats gets them; a partitioned index leaves the global occurrence counts too ----
    std::vector<i32> h_rl((size_t)nq + 1); std::vector<u64> h_ss((size_t)nq + 1); std::vector<u32> h_nk((size_t)nq + 1);
    u32 *d_acc = nullptr;
    {
        OverlapJob job; job.mode = MODE_TWOSET; job.dual = 1;
        job.prm = lrge_hip_params{0, 0.2f};
        job.paf_stats = true; job.rep_len = h_rl.data(); job.sum_span = h_ss.data(); job.n_kept = h_nk.data();
        if (!parts) { rc = run_overlap(ctx, ix, queries, job); if (rc) return rc; }
        else {
            d_acc = sc.get<u32>((size_t)queries->total_bases + 1);      // (one minimizer per base at most)
            if (!d_acc) return LRGE_ERR_DEVICE;
            HIPCHK(ctx, hipMemsetAsync(d_acc, 0, ((size_t)queries->total_bases + 1) * 4, ctx->stream));
            for (size_t pi = 0; pi < ix->parts.size(); ++pi) {
                OverlapJob j = job;
                j.d_hc_acc = d_acc; j.hc_last = pi + 1 == ix->parts.size();
                rc = run_overlap(ctx, ix->parts[pi], queries, j);
                if (rc) return rc;
            }
        }
    }
    ph[PAF_P_STATS] = paf_now_us() - t_begin;

    // ---- 2. chains, the records kept on the device: one run as a rule, a second one with the exact count when the buffer was too small ----
    u64 t0 = paf_now_us();
    u64 cap = chain_hint ? chain_hint : std::max<u64>(1024, (u64)nq * ctx->opt_u64("PAF_CHAINS_FIRST", 64));
    ALLOC_OR_FAIL(d_cnt, sc, unsigned long long, 1);
    lrge_hip_chain *d_rec = sc.get<lrge_hip_chain>(cap);
    if (!d_rec) return LRGE_ERR_DEVICE;
    u64 n = 0, runs = 1;
    rc = paf_chain_run(ctx, ix, queries, dual, d_rec, cap, d_cnt, d_acc, &n);
    if (rc) return rc;
    if (n > cap) {
        sc.drop(d_rec);
        cap = n;
        d_rec = sc.get<lrge_hip_chain>(cap);
        if (!d_rec) return LRGE_ERR_DEVICE;
        const u64 first = n;
        rc = paf_chain_run(ctx, ix, queries, dual, d_rec, cap, d_cnt, d_acc, &n);
        if (rc) return rc;
        ++runs;
        if (n != first) { LRGE_SET_ERR(ctx, "paf_text: %llu chains in the second run, %llu in the first", (unsigned long long)n, (unsigned long long)first); return LRGE_ERR_DEVICE; }
    }
    if (d_acc) { sc.drop(d_acc); d_acc = nullptr; }
    ctx->paf_stats[PAF_S_CHAIN_RUNS] = runs; ctx->paf_stats[PAF_S_RECORDS] = n;
    ph[PAF_P_CHAINS] = paf_now_us() - t0;
    if (n == 0) { ph[PAF_P_TOTAL] = paf_now_us() - t_begin; return LRGE_OK; }

    // ---- 3. measure: every line's dv code, proof and length, before the first delivery ----
    t0 = paf_now_us();
    PafPieces pc(ctx);      // (from here on copies out of locals and of the caller's tables may be queued: whichever way the call ends, this drains both streams first)
    const bool same_names = t_names == q_names && t_name_off == q_name_off && nt == nq;      // (all-vs-all: one table)
    const u64 q_bytes = q_name_off[nq] - q_name_off[0], t_bytes = t_name_off[nt] - t_name_off[0];
    ALLOC_OR_FAIL(d_rl, sc, i32, nq); ALLOC_OR_FAIL(d_ss, sc, u64, nq); ALLOC_OR_FAIL(d_nk, sc, u32, nq);
    ALLOC_OR_FAIL(d_qoff, sc, u64, (size_t)nq + 1); ALLOC_OR_FAIL(d_qn, sc, u8, q_bytes + 1);
    u64 *d_toff = d_qoff; u8 *d_tn = d_qn;
    if (!same_names) {
        d_toff = sc.get<u64>((size_t)nt + 1); d_tn = sc.get<u8>(t_bytes + 1);
        if (!d_toff || !d_tn) return LRGE_ERR_DEVICE;
    }
    ALLOC_OR_FAIL(d_code, sc, u32, n); ALLOC_OR_FAIL(d_len, sc, u32, n); ALLOC_OR_FAIL(d_tot, sc, PafTotals, 1);
    HIPCHK(ctx, hipMemcpyAsync(d_rl, h_rl.data(), (size_t)nq * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_ss, h_ss.data(), (size_t)nq * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_nk, h_nk.data(), (size_t)nq * 4, hipMemcpyHostToDevice, ctx->stream));
    // (the tables are uploaded as they are: the kernels index the blob by the offsets themselves, so the blob travels from its byte 0)
    HIPCHK(ctx, hipMemcpyAsync(d_qoff, q_name_off, ((size_t)nq + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (q_bytes) HIPCHK(ctx, hipMemcpyAsync(d_qn, q_names + q_name_off[0], q_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (!same_names) {
        HIPCHK(ctx, hipMemcpyAsync(d_toff, t_name_off, ((size_t)nt + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        if (t_bytes) HIPCHK(ctx, hipMemcpyAsync(d_tn, t_names + t_name_off[0], t_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipMemsetAsync(d_tot, 0, sizeof(PafTotals), ctx->stream));
    PafIn in;
    in.rec = reinterpret_cast<const u32 *>(d_rec); in.q_len = queries->d_len; in.t_len = ix->seqs->d_len;
    in.q_name_off = d_qoff; in.t_name_off = d_toff;
    in.q_names = d_qn - q_name_off[0]; in.t_names = d_tn - t_name_off[0];      // (offsets count from the caller's blob start)
    in.rl = d_rl; in.sum_span = d_ss; in.n_kept = d_nk;
    hipLaunchKernelGGL(k_paf_measure, dim3((u32)div_up(n, PAF_MEASURE_THREADS)), dim3(PAF_MEASURE_THREADS), 0, ctx->stream, in, n, d_code, d_len, d_tot);
    KCHK(ctx);
    PafTotals tot;
    HIPCHK(ctx, ctx->d2h(&tot, d_tot, sizeof tot, ctx->stream));
    HIPCHK(ctx, ctx->d2h_sync(ctx->stream));
    ph[PAF_P_MEASURE] = paf_now_us() - t0;
    ctx->paf_stats[PAF_S_UNPROVEN] = tot.unproven;
    if (tot.unproven) {
        LRGE_SET_ERR(ctx, "dv of %u lines not proven on the device", tot.unproven);
        ph[PAF_P_TOTAL] = paf_now_us() - t_begin;
        return LRGE_ERR_UNPROVEN;
    }

    // ---- 4. slices: at most floor(PAF_PIECE_BYTES / bound) chains each, so every slice fits a piece by construction ----
    const u64 t_format = paf_now_us();
    const u64 bound = q_longest + t_longest + PAF_FIXED_BOUND;
    const u64 piece_opt = std::min<u64>(std::max<u64>(ctx->opt_u64("PAF_PIECE_BYTES", 64ull << 20), 1), 1ull << 31);
    const u64 per_slice = std::min<u64>(std::max<u64>(piece_opt / bound, 1), n);
    const u64 piece_cap = std::max<u64>(1, std::min<u64>(per_slice * bound, tot.bytes));      // (no slice is longer than the whole text)
    const u64 n_slices = div_up(n, per_slice);
    ALLOC_OR_FAIL(d_off, sc, u32, per_slice + 1);
    u8 *d_text[2];
    d_text[0] = sc.get<u8>(piece_cap); d_text[1] = n_slices > 1 ? sc.get<u8>(piece_cap) : d_text[0];
    if (!d_text[0] || !d_text[1]) return LRGE_ERR_DEVICE;
    for (int b = 0; b < (n_slices > 1 ? 2 : 1); ++b) {
        HIPCHK(ctx, hipHostMalloc((void **)&pc.pin[b], piece_cap, hipHostMallocDefault));
        HIPCHK(ctx, hipEventCreateWithFlags(&pc.ev[b], hipEventDisableTiming));
    }
    ph[PAF_P_SETUP] = paf_now_us() - t_format;      // the slice offsets, the two device text blocks and the two pinned pieces taken
    u32 slice_bytes[2] = {0, 0};
    u64 delivered = 0, pieces = 0;
    auto deliver = [&](u64 k) -> int {          // slice k: wait for its copy, hand its lines to the sink
        const int b = (int)(k & 1);
        u64 t1 = paf_now_us();
        HIPCHK(ctx, hipEventSynchronize(pc.ev[b]));
        ph[PAF_P_COPY] += paf_now_us() - t1;
        t1 = paf_now_us();
        const int src = sink(user, pc.pin[b], slice_bytes[b]);
        ph[PAF_P_SINK] += paf_now_us() - t1;
        if (src) { LRGE_SET_ERR(ctx, "Error writing PAF file: the sink returned %d at byte %llu", src, (unsigned long long)delivered); return LRGE_ERR_PAF_WRITE; }
        delivered += slice_bytes[b]; ++pieces;
        return LRGE_OK;
    };
    for (u64 k = 0; k < n_slices; ++k) {
        const int b = (int)(k & 1);
        const u64 i0 = k * per_slice;
        const u32 m = (u32)std::min<u64>(per_slice, n - i0);
        u64 t1 = paf_now_us();
        // (d_text[b] and pin[b] are free: slice k - 2 was delivered in the round before)
        rc = scan_exclusive_u32(ctx, sc, d_len + i0, d_off, m, d_off + m);
        if (rc) return rc;
        hipLaunchKernelGGL(k_paf_write, dim3((u32)div_up(m, PAF_WRITE_WAVES)), dim3(PAF_WRITE_WAVES * 64), 0, ctx->stream, in, i0, m, d_code, d_off, d_text[b]);
        KCHK(ctx);
        HIPCHK(ctx, ctx->d2h(&slice_bytes[b], d_off + m, 4, ctx->stream));
        if (k > 0 && !serial) { rc = deliver(k - 1); if (rc) return rc; }      // beside the write of slice k
        const u64 t2 = paf_now_us();
        HIPCHK(ctx, ctx->d2h_sync(ctx->stream));
        ph[PAF_P_WRITE] += paf_now_us() - (serial ? t1 : t2);
        if (slice_bytes[b] > piece_cap) { LRGE_SET_ERR(ctx, "paf_text: a slice of %u bytes above its piece of %llu", slice_bytes[b], (unsigned long long)piece_cap); return LRGE_ERR_DEVICE; }
        // the copy down on the side stream: it runs beside the write of slice k + 1
        HIPCHK(ctx, hipMemcpyAsync(pc.pin[b], d_text[b], slice_bytes[b], hipMemcpyDeviceToHost, ctx->stream2));
        HIPCHK(ctx, hipEventRecord(pc.ev[b], ctx->stream2));
        if (serial) { rc = deliver(k); if (rc) return rc; }
    }
    if (!serial) { rc = deliver(n_slices - 1); if (rc) return rc; }
    if (delivered != tot.bytes) { LRGE_SET_ERR(ctx, "paf_text: %llu bytes delivered, %llu measured", (unsigned long long)delivered, (unsigned long long)tot.bytes); return LRGE_ERR_DEVICE; }
    ctx->paf_stats[PAF_S_LINES] = n; ctx->paf_stats[PAF_S_BYTES] = delivered; ctx->paf_stats[PAF_S_SLICES] = n_slices; ctx->paf_stats[PAF_S_PIECES] = pieces;
    ctx->paf_stats[PAF_S_FORMAT_US] = paf_now_us() - t_format + ph[PAF_P_MEASURE];
    ph[PAF_P_TOTAL] = paf_now_us() - t_begin;
    return LRGE_OK;
}

extern "C" int lrge_hip_last_paf_stats(const lrge_hip_ctx *ctx, uint64_t out[8]) {
    if (!ctx || !out) return LRGE_ERR_INVALID;
    memcpy(out, ctx->paf_stats, sizeof ctx->paf_stats);
    return LRGE_OK;
}
extern "C" int lrge_hip_last_paf_phases(const lrge_hip_ctx *ctx, uint64_t out[8]) {
    if (!ctx || !out) return LRGE_ERR_INVALID;
    memcpy(out, ctx->paf_phase_us, sizeof ctx->paf_phase_us);
    return LRGE_OK;
}
