// host_cram.inl -- read sets built on the device from unaligned CRAM (k_cram.h): the backend that
// cram_round.h's cram_run drives, the CRAM source of lrge_hip_reads_open_mem and the two C entry points.  Included into
// host_fastx.inl (lrge_hip_reads, FxSink, ingest_cap).
//
// The host walks the containers (cram_walk: the host reader's record loop, no base read) and parses the head of every BA block;
// only the BA byte ranges go up, a round at a time (option CRAM_ROUND_BYTES, default 256 MiB of compressed bytes), with their
// descriptors, table words, run-symbol flags, PACK maps and run lengths.  k_rans_decode leaves every block's bases at its
// precomputed offset in the handle's dense store, the form a windowed FASTA handle has, so the gather, the identifier ranks and
// every other consumer work unchanged.  Option CRAM_MIN_BLOCKS (default CRAM_MIN_BLOCKS_DEFAULT = 32, the measured break-even rounded up to a power of two: DESIGN section 22): a file with
// fewer BA blocks stays with the host.
// The sampled ingest (fx_cram_sampled below): the same walk and rounds with a second backend, CramKeepDev, which
// decodes a round into a scratch of the round's size and keeps the chosen reads only.

#define CRAM_MIN_BLOCKS_DEFAULT 32

namespace {
struct CramDev {
    lrge_hip_ctx *ctx;
    hipError_t e = hipSuccess;
    u8 *out = nullptr;
    GzBuf in, blks, tabs, aux, runs, tmp, status;
    explicit CramDev(lrge_hip_ctx *c) : ctx(c) { for (GzBuf *b : {&in, &blks, &tabs, &aux, &runs, &tmp, &status}) b->ctx = c; }
    ~CramDev() { (void)hipStreamSynchronize(ctx->stream); }
    bool ok(hipError_t x) { if (x != hipSuccess && e == hipSuccess) e = x; return e == hipSuccess; }
    bool up(GzBuf &b, const void *src, size_t bytes) {
        if (!b.need(bytes + 16, &e)) return false;
        return !bytes || ok(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    bool round(const uint8_t *h_in, size_t in_bytes, const RansBlk *blk, uint32_t m, const RansTables &t, uint64_t tmp_bytes, uint32_t *st_h) {
        hipStream_t st = ctx->stream;
        if (!up(in, h_in, in_bytes) || !up(blks, blk, (size_t)m * sizeof(RansBlk)) || !up(tabs, t.tabs.data(), t.tabs.size() * 2) || !up(aux, t.aux.data(), t.aux.size()) ||
            !up(runs, t.runs.data(), t.runs.size() * 4) || !tmp.need((size_t)tmp_bytes + 16, &e) || !status.need((size_t)m * 4, &e))
            return false;
        if (!ok(hipMemsetAsync(status.p, 0xFF, (size_t)m * 4, st))) return false;
        u32 lds_words = 0;                                         // the largest model of the round that fits LDS
        for (uint32_t a = 0; a < m; ++a)
            if (blk[a].codec && blk[a].n_sym && rans_model_words(blk[a]) <= RANS_LDS_U16) lds_words = std::max<u32>(lds_words, rans_model_words(blk[a]));
        hipLaunchKernelGGL(k_rans_decode, dim3(m), dim3(64), (size_t)lds_words * 2, st, in.as<const u8>(), blks.as<const RansBlk>(), m, tabs.as<const uint16_t>(),
                           aux.as<const u8>(), runs.as<const u32>(), lds_words, tmp.as<u8>(), out, status.as<u32>());
        if (!ok(hipGetLastError())) return false;
        return ok(hipMemcpyAsync(st_h, status.p, (size_t)m * 4, hipMemcpyDeviceToHost, st)) && ok(hipStreamSynchronize(st));
    }
};

static void cram_stats_out(const CramStats &s, lrge_hip_cram_stats *o) {
    static_assert(sizeof(lrge_hip_cram_stats) == CRAM_STAT_WORDS * 8, "one word a field");
    if (o) cram_stats_words(s, (uint64_t *)o);
}
static_assert(sizeof(lrge_hip_rans_stream) == 24, "the stream record of the header");

static int cram_device_error(lrge_hip_ctx *ctx, const CramDev &dev, const char *what) {
    LRGE_SET_ERR(ctx, "%s: %s", what, hipGetErrorString(dev.e != hipSuccess ? dev.e : hipErrorUnknown));
    (void)hipGetLastError();
    return LRGE_ERR_DEVICE;
}
}  // namespace

// input that starts with "CRAM", under LRGE_GPU_INGEST_CRAM: the whole call
static int fx_open_cram(lrge_hip_ctx *ctx, lrge_hip_reads *R, const u8 *d, u64 len, double t0) {
    CramWalk cw;
    std::string why;
    const uint64_t w0 = cram_now_us();
    if (!cram_walk(d, len, cw, why)) return fx_unproven(ctx, why.c_str());
    CramStats &st = R->cram;
    st.walk_us = cram_now_us() - w0;
    st.containers = cw.w.containers; st.slices = cw.w.ba.size(); st.records = cw.w.recs.size();
    const u64 n = cw.w.recs.size(), total = cw.ba_out.back();
    if (n >> 32) return fx_verdict_rc(ctx, FX_TOO_MANY, "CRAM records");
    if (cw.names.size() >> 32) return fx_unproven(ctx, "4 GiB of identifiers or more");
    const std::vector<RansStream> s = cram_streams(cw);
    if (s.size() < ctx->opt_u64("CRAM_MIN_BLOCKS", CRAM_MIN_BLOCKS_DEFAULT)) return fx_unproven(ctx, "fewer BA blocks than CRAM_MIN_BLOCKS");
    const u64 round_bytes = std::max<u64>(1, ctx->opt_u64("CRAM_ROUND_BYTES", (u64)256 << 20)), cap = ingest_cap(ctx);
    u64 comp = 0, largest = 0;
    for (const RansStream &k : s) { comp += k.n; largest = std::max<u64>(largest, k.n); }
    if (total + std::max<u64>(largest, std::min<u64>(round_bytes, comp)) > cap) {
        LRGE_SET_ERR(ctx, "reads_open: bases and one round above INGEST_MAX_BYTES (%llu)", (unsigned long long)cap);
        return LRGE_ERR_UNPROVEN;
    }
    int rc = fx_alloc_text(ctx, R, total);
    if (rc) return rc;
    {
        CramDev dev(ctx);
        dev.out = R->d_text;
        const int64_t bad = cram_run(dev, s, round_bytes, true, st, nullptr, why);
        if (bad < 0) return cram_device_error(ctx, dev, "reads_open: CRAM base blocks");
        if (bad) return fx_unproven(ctx, why.c_str());
    }
    const double t1 = fx_now_ms();
    // the record table of a base store: a record's bases are where the walk found them
    std::vector<FxRec> tab((size_t)n);
    R->seq_len.resize((size_t)n);
    for (u64 i = 0; i < n; ++i) {
        const auto &r = cw.w.recs[(size_t)i];
        R->seq_len[(size_t)i] = r.len;
        tab[(size_t)i] = FxRec{0, cw.ba_out[r.slice] + r.off, r.len, (u32)(cw.name_off[(size_t)i + 1] - cw.name_off[(size_t)i]), r.len};
    }
    if ((rc = fx_upload_recs(ctx, R, tab))) return rc;
    R->n = n; R->names.swap(cw.names); R->name_off.swap(cw.name_off);
    R->fmt = n ? FX_FMT_FASTA : FX_FMT_EMPTY;
    R->text_bytes = total; R->is_cram = true;
    const double t2 = fx_now_ms();
    R->ms[0] = (float)(t1 - t0); R->ms[1] = 0; R->ms[2] = (float)(t2 - t1); R->ms[3] = (float)(t2 - t0);
    if (ctx->opt("VERBOSE")) fprintf(stderr, "[lrge_hip] reads_open: CRAM, %llu records in %llu slices, %llu bases from %llu compressed bytes in %llu rounds; walk %.2f ms, decode %.2f ms\n",
                                    (unsigned long long)n, (unsigned long long)st.slices, (unsigned long long)total, (unsigned long long)st.comp_bytes, (unsigned long long)st.rounds,
                                    st.walk_us / 1000.0, st.decode_us / 1000.0);
    return LRGE_OK;
}

// ---- the sampled ingest of CRAM: census, selected open, census with a map, mapped open ----
namespace {
static_assert(sizeof(CramCopy) == sizeof(FxRunCopy), "k_fx_runs takes the copy table of cram_round_copies as it is");

// The second backend of cram_run: a round is decoded by CramDev into a scratch block of the round's raw size -- the descriptors
// rebased on a copy, cram_run and k_rans_decode as they are -- and k_fx_runs copies the chosen reads' ranges from there to the dense
// store, which is allocated once at the chosen bases.  A census has no store and no copy
struct CramKeepDev {
    lrge_hip_ctx *ctx;
    CramDev dev;
    GzBuf scratch, copies, first;
    const CramWalk *cw = nullptr;
    const CramKeepPlan *plan = nullptr;
    const u32 *sel = nullptr;
    u8 *store = nullptr;
    u64 at = 0;
    explicit CramKeepDev(lrge_hip_ctx *c) : ctx(c), dev(c) { for (GzBuf *b : {&scratch, &copies, &first}) b->ctx = c; }
    ~CramKeepDev() { ctx->pool.release(store); }
    bool begin(const CramWalk &w, const CramKeepPlan &p, const uint32_t *s, uint64_t) {
        cw = &w; plan = &p; sel = s; at = 0;
        return (store = (u8 *)ctx->pool.alloc((size_t)p.dst.back() + FX_PAD, &dev.e)) != nullptr;
    }
    bool round(const uint8_t *h_in, size_t in_bytes, const RansBlk *blk, uint32_t m, const RansTables &t, uint64_t tmp_bytes, uint32_t *st_h) {
        std::vector<RansBlk> b(blk, blk + m);
        std::vector<uint64_t> scr(m);
        const u64 raw = cram_rebase(b.data(), m, scr.data());
        if (!scratch.need((size_t)raw + FX_PAD, &dev.e)) return false;          // (FX_PAD: fx_copy_span may load the word behind a range's last byte)
        dev.out = scratch.as<u8>();
        if (!dev.round(h_in, in_bytes, b.data(), m, t, tmp_bytes, st_h)) return false;
        bool good = true;
        for (uint32_t a = 0; a < m; ++a) good = good && st_h[a] == RANS_OK;
        std::vector<CramCopy> c;
        if (good) cram_round_copies(*cw, *plan, sel, (size_t)at, m, scr.data(), c);
        at += m;
        if (c.empty()) return true;
        std::vector<u64> f(c.size() + 1, 0);
        for (size_t i = 0; i < c.size(); ++i) {
            if (c[i].src + c[i].len > raw || c[i].dst + c[i].len > plan->dst.back()) return dev.ok(hipErrorInvalidValue);      // (never: the walk proved the lengths)
            f[i + 1] = f[i] + div_up(c[i].len, (u64)FX_RUN_TILE);
        }
        if (f.back() >> 31 || c.size() >> 32) return dev.ok(hipErrorInvalidValue);                                             // (never: a round is below 2^31 tiles)
        hipStream_t st = ctx->stream;
        if (!dev.up(copies, c.data(), c.size() * sizeof(CramCopy)) || !dev.up(first, f.data(), f.size() * 8)) return false;
        hipLaunchKernelGGL(k_fx_runs, dim3((u32)f.back()), dim3(64), 0, st, scratch.as<const u8>(), store, copies.as<const FxRunCopy>(), first.as<const u64>(), (u32)c.size());
        return dev.ok(hipGetLastError()) && dev.ok(hipStreamSynchronize(st));      // (the tables are pageable, and the scratch is decoded into again)
    }
};
}  // namespace

static bool cram_select_flags(int flags) { return (flags & LRGE_GPU_INGEST_CRAM) && (flags & LRGE_GPU_INGEST_SELECT_CRAM); }

// One sampled call on input that starts with "CRAM", under LRGE_GPU_INGEST_SELECT_CRAM beside LRGE_GPU_INGEST_CRAM.  mode
// FX_KEEP_NONE: the census (map: filled when given); FX_KEEP_SEL: the selected open, or -- mapped -- the mapped open on `map`
static int fx_cram_sampled(lrge_hip_ctx *ctx, lrge_hip_reads *R, const u8 *d, u64 len, FxKeepMode mode, const u32 *sel, u64 k, bool mapped, FxSeekMap *map, double t0) {
    if (mode != FX_KEEP_SEL) k = 0;
    const u64 cap = ingest_cap(ctx);
    CramSampled o;
    CramKeepDev sink(ctx);
    std::string why;
    const int rc = cram_sampled(sink, d, len, sel, k, mapped, map, ctx->opt_u64("CRAM_MIN_BLOCKS", CRAM_MIN_BLOCKS_DEFAULT), std::max<u64>(1, ctx->opt_u64("CRAM_ROUND_BYTES", (u64)256 << 20)),
                                cap, o, why);
    switch (rc) {
    case CRAM_S_OK: break;
    case CRAM_S_UNPROVEN: return fx_unproven(ctx, why.c_str());
    case CRAM_S_ORDINAL: return fx_ordinal_rc(ctx, o.bad_ordinal, o.cw.w.recs.size());
    case CRAM_S_OTHER_INPUT: return fx_map_other(ctx);
    case CRAM_S_MISFIT: return fx_map_misfit(ctx, why.c_str());
    case CRAM_S_OVER_CAP: LRGE_SET_ERR(ctx, "reads_open_selected: chosen bases and one round of CRAM blocks above INGEST_MAX_BYTES (%llu)", (unsigned long long)cap); return LRGE_ERR_UNPROVEN;
    default: return cram_device_error(ctx, sink.dev, "reads_open_selected: CRAM base blocks");
    }
    const double t1 = fx_now_ms();
    const u64 n = o.cw.w.recs.size(), total = o.cw.ba_out.back(), kept = o.plan.dst.back();
    std::vector<FxRec> tab((size_t)k);
    R->seq_len.resize((size_t)k);
    for (u64 j = 0; j < k; ++j) {
        const u32 l = o.cw.w.recs[sel[j]].len;
        R->seq_len[(size_t)j] = l;
        tab[(size_t)j] = FxRec{0, o.plan.dst[(size_t)j], l, (u32)(o.cw.name_off[(size_t)j + 1] - o.cw.name_off[(size_t)j]), l};
    }
    int arc;
    if ((arc = fx_upload_recs(ctx, R, tab))) return arc;
    R->d_text = sink.store; sink.store = nullptr; R->n_text = kept;
    R->n = k; R->names.swap(o.cw.names); R->name_off.swap(o.cw.name_off);
    R->fmt = k ? FX_FMT_FASTA : FX_FMT_EMPTY;
    R->text_bytes = total; R->is_cram = true;
    R->cram = o.st;
    R->sel = FxSelStats{n, k, total, kept};
    R->win.bases = kept;                                              // (window_stats out[1]: the bytes of the dense store; no window was flushed)
    memcpy(R->seek, o.seek, sizeof R->seek);
    const double t2 = fx_now_ms();
    R->ms[0] = (float)(t1 - t0); R->ms[1] = 0; R->ms[2] = (float)(t2 - t1); R->ms[3] = (float)(t2 - t0);
    if (ctx->opt("VERBOSE")) fprintf(stderr, "[lrge_hip] reads_open_selected: CRAM, %llu of %llu records, %llu of %llu bases kept; %llu of %llu slices decoded in %llu rounds of at most %llu compressed bytes; walk %.2f ms, decode %.2f ms\n",
                                    (unsigned long long)k, (unsigned long long)n, (unsigned long long)kept, (unsigned long long)total, (unsigned long long)o.plan.streams.size(),
                                    (unsigned long long)o.st.slices, (unsigned long long)o.st.rounds, (unsigned long long)o.round_bytes, o.st.walk_us / 1000.0, o.st.decode_us / 1000.0);
    return LRGE_OK;
}

extern "C" int lrge_hip_reads_cram_stats(const lrge_hip_reads *r, lrge_hip_cram_stats *out) {
    if (!r || !out || !r->is_cram) return LRGE_ERR_INVALID;
    cram_stats_out(r->cram, out);
    return LRGE_OK;
}

extern "C" int lrge_hip_rans_decode(lrge_hip_ctx *ctx, const void *comp, uint64_t comp_len, lrge_hip_rans_stream *streams, uint32_t n, void *out, uint64_t out_cap,
                                    lrge_hip_cram_stats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (!ctx || (!comp && comp_len) || (!streams && n)) return LRGE_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<RansStream> v;
    u64 total = 0;
    for (u32 i = 0; i < n; ++i) {
        const lrge_hip_rans_stream &k = streams[i];
        if (k.offset > comp_len || k.length > comp_len - k.offset || (k.raw_size >> 31)) { LRGE_SET_ERR(ctx, "rans_decode: stream %u lies outside the input or is 2^31 bytes or more", i); return LRGE_ERR_INVALID; }
        v.push_back(RansStream{(const uint8_t *)comp + k.offset, k.length, (int)k.method, (int64_t)k.raw_size, total});
        total += k.raw_size;
    }
    if (total > out_cap || (!out && total)) { LRGE_SET_ERR(ctx, "rans_decode: the output needs %llu bytes", (unsigned long long)total); return LRGE_ERR_INVALID; }
    Scratch sc(ctx);
    ALLOC_OR_FAIL(d_out, sc, u8, total + FX_PAD);
    HIPCHK(ctx, hipMemsetAsync(d_out, 0, (size_t)total + FX_PAD, ctx->stream));
    CramStats st;
    std::string why;
    std::vector<u32> status(n, 0);
    {
        CramDev dev(ctx);
        dev.out = d_out;
        if (cram_run(dev, v, std::max<u64>(1, ctx->opt_u64("CRAM_ROUND_BYTES", (u64)256 << 20)), false, st, status.data(), why) < 0) return cram_device_error(ctx, dev, "rans_decode");
    }
    for (u32 i = 0; i < n; ++i) streams[i].status = status[i];
    if (total) HIPCHK(ctx, hipMemcpyAsync(out, d_out, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (!why.empty()) ctx->err = "rans_decode: " + why;
    cram_stats_out(st, stats);
    return LRGE_OK;
}
