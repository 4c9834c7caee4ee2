// host_names.inl -- identifier ranks on the device by a fixed number of LSD sort passes: the device backend of
// name_lsd_round.h over the kernels of k_names.h, radix_sort_pairs and scan_exclusive_u32, and the entry points
// lrge_hip_name_ranks / lrge_hip_reads_name_ranks.  The host gathers only the selected identifiers into one padded blob; the
// number and shape of all launches follow from n and the longest identifier; the only read-back is the ranks and one status /
// statistics word at the end.  Included into lrge_hip.hip (behind host_fastx.inl: lrge_hip_reads).

#include "k_names.h"
#include "name_lsd_round.h"

struct NlDev {
    lrge_hip_ctx *ctx;
    Scratch sc;
    NlArgs A = {nullptr, 0, nullptr, nullptr, 0, 0, nullptr};
    u64 *kb[2] = {nullptr, nullptr}, *vb[2] = {nullptr, nullptr};
    u32 *d_flag = nullptr, *d_excl = nullptr, *d_start = nullptr, *d_rank = nullptr, *d_stat = nullptr;
    u64 n = 0;
    u32 stat[2] = {0, 0};
    explicit NlDev(lrge_hip_ctx *c) : ctx(c), sc(c) {}
    dim3 grid() const { return dim3((u32)div_up(n, NL_THREADS)); }

    // every block of the call is taken here, before the first launch; the copies read pageable memory that outlives the call
    int upload(const NlBlob &B, uint64_t n_) {
        n = n_;
        ALLOC_OR_FAIL(d_w8, sc, u64, B.words.size());
        ALLOC_OR_FAIL(d_off, sc, u64, n);
        ALLOC_OR_FAIL(d_len, sc, u32, n);
        for (int s = 0; s < 2; ++s) {
            if (!(kb[s] = sc.get<u64>(n)) || !(vb[s] = sc.get<u64>(n))) return LRGE_ERR_DEVICE;
        }
        if (!(d_flag = sc.get<u32>(n)) || !(d_excl = sc.get<u32>(n)) || !(d_start = sc.get<u32>(n)) || !(d_rank = sc.get<u32>(n)) || !(d_stat = sc.get<u32>(2)))
            return LRGE_ERR_DEVICE;
        HIPCHK(ctx, hipMemcpyAsync(d_w8, B.words.data(), B.words.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_off, B.off.data(), (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_len, B.len.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(d_stat, 0, 8, ctx->stream));
        A = NlArgs{d_w8, B.bytes, d_off, d_len, (u32)n, nl_words(B.lmax), d_stat};
        return LRGE_OK;
    }
    uint64_t *key_buf(int s) { return kb[s]; }
    uint64_t *val_buf(int s) { return vb[s]; }
    int keys(uint32_t pass, uint32_t, bool first, uint64_t *val, uint64_t *key) {
        hipLaunchKernelGGL(k_nl_key, grid(), dim3(NL_THREADS), 0, ctx->stream, A, (u64 *)val, (u64 *)key, pass, first ? 1u : 0u);
        KCHK(ctx);
        return LRGE_OK;
    }
    int sort(uint64_t *k0, uint64_t *v0, uint64_t *k1, uint64_t *v1, uint64_t n_, int nbits, uint64_t **rk, uint64_t **rv) {
        u64 *a = nullptr, *b = nullptr;
        const int rc = radix_sort_pairs(ctx, sc, (u64 *)k0, (u64 *)v0, (u64 *)k1, (u64 *)v1, n_, 0, nbits, &a, &b);
        *rk = a; *rv = b;
        return rc;
    }
    int heads(const uint64_t *val, uint32_t) {
        hipLaunchKernelGGL(k_nl_heads, grid(), dim3(NL_THREADS), 0, ctx->stream, A, (const u64 *)val, d_flag);
        KCHK(ctx);
        return LRGE_OK;
    }
    int ranks(const uint64_t *val) {
        const int rc = scan_exclusive_u32(ctx, sc, d_flag, d_excl, n, d_stat);
        if (rc) return rc;
        hipLaunchKernelGGL(k_nl_starts, grid(), dim3(NL_THREADS), 0, ctx->stream, A, (const u32 *)d_flag, (const u32 *)d_excl, d_start);
        KCHK(ctx);
        hipLaunchKernelGGL(k_nl_rank, grid(), dim3(NL_THREADS), 0, ctx->stream, A, (const u64 *)val, (const u32 *)d_flag, (const u32 *)d_excl, (const u32 *)d_start, d_rank);
        KCHK(ctx);
        return LRGE_OK;
    }
    int finish(uint32_t *rank_out, uint64_t *word) {
        HIPCHK(ctx, ctx->d2h(rank_out, d_rank, (size_t)n * 4, ctx->stream));
        HIPCHK(ctx, ctx->d2h(stat, d_stat, 8, ctx->stream));
        HIPCHK(ctx, ctx->d2h_sync(ctx->stream));
        ctx->resolve_timers();
        *word = (u64)stat[1] << 32 | stat[0];
        return LRGE_OK;
    }
};

static int name_ranks_impl(lrge_hip_ctx *ctx, const char *names, const uint64_t *name_off, uint64_t n_names, const uint32_t *idx, uint64_t n, uint32_t *rank_out,
                           uint64_t stats[4]) {
    const double t0 = DevPool::now_ms();
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n && !rank_out) { ctx->err = "name_ranks: no rank_out"; return LRGE_ERR_INVALID; }
    NlBlob B;
    const char *why = "";
    int rc = nl_gather(names, name_off, n_names, idx, n, ctx->opt_u64("NAME_RANK_MAX_BYTES", NL_MAX_BYTES_DEFAULT), B, &why);
    if (rc) { LRGE_SET_ERR(ctx, "name_ranks: %s", why); return rc; }
    NlStats st = {0, nl_words(B.lmax), 0};
    if (n >= 2) HIPCHK(ctx, hipSetDevice(ctx->device));
    {
        NlDev dev(ctx);
        rc = nl_run(dev, B, n, rank_out, st, &why);
        // a step that failed after launches were queued: nothing of the call may still run when its memory goes back to the arena
        if (rc && n >= 2) { (void)hipStreamSynchronize(ctx->stream); ctx->pin_items.clear(); ctx->pin_used = 0; }
    }
    if (rc && *why) LRGE_SET_ERR(ctx, "name_ranks: %s", why);
    if (stats) { stats[0] = st.sorts; stats[1] = st.words; stats[2] = st.distinct; stats[3] = (uint64_t)((DevPool::now_ms() - t0) * 1000.0); }
    return rc;
}

extern "C" int lrge_hip_name_ranks(lrge_hip_ctx *ctx, const char *names, const uint64_t *name_off, uint64_t n_names, const uint32_t *idx, uint64_t n,
                                   uint32_t *rank_out, uint64_t stats[4]) {
    if (!ctx) return LRGE_ERR_INVALID;
    return name_ranks_impl(ctx, names, name_off, n_names, idx, n, rank_out, stats);
}

extern "C" int lrge_hip_reads_name_ranks(const lrge_hip_reads *r, const uint32_t *idx, uint64_t n, uint32_t *rank_out, uint64_t stats[4]) {
    if (!r || !r->ctx) return LRGE_ERR_INVALID;
    static const uint64_t none[1] = {0};
    const bool empty = r->n == 0 || r->name_off.size() < r->n + 1;
    return name_ranks_impl(r->ctx, r->names.data(), empty ? none : r->name_off.data(), empty ? 0 : r->n, idx, n, rank_out, stats);
}
