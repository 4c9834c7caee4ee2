// host_zstd.inl -- Zstandard decompressed on the device (k_zstd.h): the backend that zs_round.h's zs_run drives
// and the C entry point.  Included into lrge_hip.hip behind host_gzip.inl (DevKeep, GzBuf).
//
// The compressed bytes go up once and stay for the call.  The text of the whole call stays in the backend's DevKeep block: a match
// reaches back through every earlier block of its frame, and a later round reads the bytes of the rounds before.  Option
// ZSTD_ROUND_BLOCKS: the blocks decoded per round; its default is what half of the arena's idle bytes plus the device's free bytes
// hold at zs_block_bytes plus the text per block, at most ZS_ROUND_MAX.  Option ZSTD_CHECKSUM (default 1): 0 skips XXH64.  Option
// ZSTD_TIMING: the stages are separated by synchronisations and their times are printed to stderr when the call ends
// (tools/zstd_bench.py); the checksum's time is always measured, its launch is followed by the read of its word anyway.
//
// The sliding mode (the windowed and the sampled ingest under LRGE_GPU_INGEST_WINDOWED_ZSTD): the rounds are
// decoded in a work block [history | round] of their own, sized once from the block headers.  A finished round is appended
// device-to-device to the DevKeep block and flushed through the ingest's windows, as a gzip round is; the history the next round
// needs moves to the front of the work block.  Everything is ordered on the context's main stream.

static const char *zs_status_name(int s) {
    switch (s) {
    case ZS_E_MAGIC: return "no frame magic where a frame must start";
    case ZS_E_INPUT: return "unexpected end of compressed data";
    case ZS_E_RESERVED: return "a reserved bit is set";
    case ZS_E_DICT: return "a dictionary ID other than 0";
    case ZS_E_WINDOW: return "a window above 2^27 bytes";
    case ZS_E_BLOCK_TYPE: return "block type 3";
    case ZS_E_BLOCK_SIZE: return "a block above Block_Maximum_Size";
    case ZS_E_LIT_HEADER: return "a literals section that does not fit its block";
    case ZS_E_ACCURACY: return "an accuracy log above the format's limit";
    case ZS_E_FSE: return "an invalid FSE table description";
    case ZS_E_WEIGHTS: return "invalid Huffman weights";
    case ZS_E_BITSTREAM: return "a bitstream not consumed exactly";
    case ZS_E_NO_TABLE: return "treeless literals or a repeat mode with no table in front";
    case ZS_E_SYMBOL: return "a symbol above its alphabet";
    case ZS_E_LITERALS: return "more literals asked for than the block has";
    case ZS_E_OFFSET: return "an offset of 0, beyond the frame's bytes or beyond the window";
    case ZS_E_CONTENT_SIZE: return "Frame_Content_Size mismatch";
    case ZS_E_CHECKSUM: return "content checksum mismatch";
    case ZS_E_SEQ_HEADER: return "a sequences section that does not fit its block";
    case ZS_E_TOO_BIG: return "the text does not fit the device budget";
    default: return "unknown status";
    }
}

namespace {
struct ZsDev : DevKeep {
    GzBuf in, blocks, hbuf, lit, seq, res, status, org, groups, hash, work, xstate;
    u64 n = 0;
    // the sliding mode: work holds work_len bytes, the round behind `hist` bytes of history; retire() left keep_hist bytes to carry
    bool sliding = false;
    u64 slide_window = 0;                                        // the ingest's window: a round's text stays below it (default_round)
    u64 work_text = 0, work_len = 0, hist = 0, keep_hist = 0;
    std::function<bool(u64)> work_budget;                        // the work block's bytes, taken from the budget the caller shares out (false: above it)
    bool timing = false;
    double ms[6] = {0, 0, 0, 0, 0, 0};                           // heads, literals, sequences, execute, resolve, checksum
    explicit ZsDev(lrge_hip_ctx *c) : DevKeep(c) {
        for (GzBuf *b : {&in, &blocks, &hbuf, &lit, &seq, &res, &status, &org, &groups, &hash, &work, &xstate}) b->ctx = c;
        timing = c->opt("ZSTD_TIMING") != nullptr;
    }
    ~ZsDev() { (void)hipStreamSynchronize(ctx->stream); }
    bool over() const { return keep_over; }
    bool load(const uint8_t *d, uint64_t len) {
        n = len;
        if (!in.need((size_t)len + ZS_PAD, &e)) return false;
        if (!ok(hipMemsetAsync(in.as<u8>() + len, 0, ZS_PAD, ctx->stream))) return false;
        if (len && !ok(hipMemcpyAsync(in.p, d, (size_t)len, hipMemcpyHostToDevice, ctx->stream))) return false;
        return sync();
    }
    uint32_t default_round() {
        const u64 k = std::min<u64>(ZS_ROUND_MAX, std::max<u64>(1, dev_budget(ctx) / (zs_block_bytes() + ZS_BLOCK_MAX)));
        return (uint32_t)(sliding ? std::min<u64>(k, std::max<u64>(1, slide_window / ZS_BLOCK_MAX)) : k);
    }
    bool slides() const { return sliding; }
    bool plan(uint64_t work_bytes) {
        const u64 bytes = work_bytes + ZS_PAD;
        if (work_budget && !work_budget(bytes)) { keep_over = true; return false; }
        work_text = work_bytes;
        return work.need((size_t)bytes, &e) && xstate.need(2 * sizeof(ZsXxh), &e);
    }
    // the history to the front: one copy when source and destination are apart, else the forward copy of k_zs_slide
    bool slide(uint64_t history, uint64_t bytes) {
        if (history != keep_hist || history > work_len || history + bytes > work_text) return false;      // (never: zs_run's own plan)
        const u64 from = work_len - history;
        if (history && from >= history) { if (!ok(hipMemcpyAsync(work.p, work.as<u8>() + from, (size_t)history, hipMemcpyDeviceToDevice, ctx->stream))) return false; }
        else if (history && from) {
            hipLaunchKernelGGL(k_zs_slide, dim3(1), dim3(ZS_SLIDE_THREADS), 0, ctx->stream, work.as<u8>(), from, history);
            if (!ok(hipGetLastError())) return false;
        }
        hist = history; work_len = history + bytes;
        return true;
    }
    // the checked round behind the text kept so far, through the caller's windows; the next round's history is noted
    bool retire(uint64_t keep_bytes) {
        const u64 bytes = work_len - hist;
        if (keep_bytes > work_len || !keep_reserve(bytes)) return false;
        if (bytes && !ok(hipMemcpyAsync(keep + keep_len, work.as<const u8>() + hist, (size_t)bytes, hipMemcpyDeviceToDevice, ctx->stream))) return false;
        keep_len += bytes; keep_hist = keep_bytes;
        return !keep_flush || keep_flush();
    }
    bool xxh64_part(const ZsXxhJob *job, uint32_t m, uint64_t *h) {
        Lap lap(*this, ms[5], true);
        for (uint32_t i = 0; i < m; ++i) if (job[i].at + job[i].len > work_len) return false;                 // (never)
        if (!hash.need((size_t)m * (sizeof(ZsXxhJob) + 8), &e)) return false;
        u64 *out = (u64 *)(hash.as<ZsXxhJob>() + m);
        if (!ok(hipMemcpyAsync(hash.p, job, (size_t)m * sizeof(ZsXxhJob), hipMemcpyHostToDevice, ctx->stream))) return false;
        hipLaunchKernelGGL(k_zs_xxh64_part, dim3(m), dim3(64), 0, ctx->stream, work.as<const u8>(), hash.as<const ZsXxhJob>(), xstate.as<ZsXxh>(), out);
        if (!ok(hipGetLastError())) return false;
        if (!ok(hipMemcpyAsync(h, out, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream)) || !sync()) return false;
        return lap.end();
    }
    bool put_blocks(const ZsBlock *b, uint32_t k) {
        return blocks.need((size_t)k * sizeof(ZsBlock), &e) && ok(hipMemcpyAsync(blocks.p, b, (size_t)k * sizeof(ZsBlock), hipMemcpyHostToDevice, ctx->stream));
    }
    bool heads(ZsBlock *b, uint32_t k) {
        Lap lap(*this, ms[0], timing);
        if (!put_blocks(b, k) || !hbuf.need((size_t)k * sizeof(ZsHead), &e)) return false;
        hipLaunchKernelGGL(k_zs_heads, dim3((u32)div_up(k, 64)), dim3(64), 0, ctx->stream, in.as<const u8>(), blocks.as<const ZsBlock>(), k, hbuf.as<ZsHead>());
        if (!ok(hipGetLastError())) return false;
        std::vector<ZsHead> h(k);
        if (!ok(hipMemcpyAsync(h.data(), hbuf.p, (size_t)k * sizeof(ZsHead), hipMemcpyDeviceToHost, ctx->stream)) || !sync()) return false;
        for (uint32_t j = 0; j < k; ++j) if (b[j].type == 2) b[j].h = h[j];
        return lap.end();
    }
    bool entropy(const ZsBlock *b, uint32_t k, uint64_t lit_bytes, uint64_t n_seq, uint32_t *lit_status, ZsSeqRes *r) {
        hipStream_t st = ctx->stream;
        if (!put_blocks(b, k) || !lit.need((size_t)lit_bytes + 16, &e) || !seq.need((size_t)(n_seq + 1) * sizeof(ZsSeq), &e) || !res.need((size_t)k * sizeof(ZsSeqRes), &e) ||
            !status.need((size_t)k * 4, &e))
            return false;
        if (!ok(hipMemsetAsync(status.p, 0, (size_t)k * 4, st)) || !ok(hipMemsetAsync(res.p, 0, (size_t)k * sizeof(ZsSeqRes), st))) return false;
        {
            Lap lap(*this, ms[1], timing);
            hipLaunchKernelGGL(k_zs_literals, dim3(k), dim3(64), 0, st, in.as<const u8>(), n, blocks.as<const ZsBlock>(), k, lit.as<u8>(), status.as<u32>());
            if (!ok(hipGetLastError()) || !lap.end()) return false;
        }
        Lap lap(*this, ms[2], timing);
        hipLaunchKernelGGL(k_zs_sequences, dim3(k), dim3(64), 0, st, in.as<const u8>(), n, blocks.as<const ZsBlock>(), k, seq.as<ZsSeq>(), res.as<ZsSeqRes>());
        if (!ok(hipGetLastError())) return false;
        if (!ok(hipMemcpyAsync(lit_status, status.p, (size_t)k * 4, hipMemcpyDeviceToHost, st)) || !ok(hipMemcpyAsync(r, res.p, (size_t)k * sizeof(ZsSeqRes), hipMemcpyDeviceToHost, st)) ||
            !sync())
            return false;
        return lap.end();
    }
    bool reserve(uint64_t bytes) { return keep_reserve(bytes); }
    bool execute(const ZsBlock *b, uint32_t k, const uint32_t *group, uint32_t n_groups, uint64_t bytes, uint32_t *st_h) {
        hipStream_t st = ctx->stream;
        if (!put_blocks(b, k) || !org.need((size_t)(bytes + 1) * 4, &e) || !groups.need((size_t)(n_groups + 1) * 4, &e) || !status.need((size_t)k * 4, &e)) return false;
        if (!ok(hipMemcpyAsync(groups.p, group, (size_t)(n_groups + 1) * 4, hipMemcpyHostToDevice, st)) || !ok(hipMemsetAsync(status.p, 0, (size_t)k * 4, st))) return false;
        u8 *const text = sliding ? work.as<u8>() : keep;
        const u64 base = sliding ? hist : keep_len;
        {
            Lap lap(*this, ms[3], timing);
            hipLaunchKernelGGL(k_zs_execute, dim3(k), dim3(64), 0, st, in.as<const u8>(), blocks.as<const ZsBlock>(), k, lit.as<const u8>(), seq.as<const ZsSeq>(), text, org.as<u32>(),
                               base, status.as<u32>());
            if (!ok(hipGetLastError())) return false;
            if (!ok(hipMemcpyAsync(st_h, status.p, (size_t)k * 4, hipMemcpyDeviceToHost, st)) || !sync() || !lap.end()) return false;
        }
        for (uint32_t j = 0; j < k; ++j) if (st_h[j]) return true;         // (no block's origins are resolved when one of them is damaged)
        Lap lap(*this, ms[4], timing);
        hipLaunchKernelGGL(k_zs_resolve, dim3(n_groups), dim3(ZS_RESOLVE_THREADS), 0, st, blocks.as<const ZsBlock>(), groups.as<const u32>(), text, org.as<const u32>(), base);
        if (!ok(hipGetLastError()) || !lap.end()) return false;
        if (!sliding) keep_len += bytes;                             // (sliding: retire() appends the round)
        return true;
    }
    bool xxh64(const uint64_t *at, const uint64_t *len, uint32_t m, uint64_t *h) {
        Lap lap(*this, ms[5], true);
        std::vector<u64> span(2 * (size_t)m);
        for (uint32_t i = 0; i < m; ++i) { span[2 * i] = at[i]; span[2 * i + 1] = len[i]; }
        if (!hash.need((size_t)m * 24, &e)) return false;
        if (!ok(hipMemcpyAsync(hash.p, span.data(), (size_t)m * 16, hipMemcpyHostToDevice, ctx->stream))) return false;
        hipLaunchKernelGGL(k_zs_xxh64, dim3(m), dim3(64), 0, ctx->stream, sliding ? work.as<const u8>() : (const u8 *)keep, hash.as<const u64>(), hash.as<u64>() + 2 * (size_t)m);
        if (!ok(hipGetLastError())) return false;
        if (!ok(hipMemcpyAsync(h, hash.as<u64>() + 2 * (size_t)m, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream)) || !sync()) return false;
        return lap.end();
    }
    // (the text that stays has been flushed by retire(), where it slides; else nothing flushes it)
    const uint8_t *bytes(uint64_t at, uint64_t len) { return deliver((sliding ? work.as<const u8>() : keep) + at, len, false); }
};

static bool zs_checksum_on(lrge_hip_ctx *ctx) { return ctx->opt_u64("ZSTD_CHECKSUM", 1) != 0; }
static void zs_stats_out(const ZsStats &st, const ZsDev &dev, lrge_hip_zstd_stats *o) {
    if (!o) return;
    o->frames = st.frames; o->skippable_frames = st.skippable; o->blocks = st.blocks; o->raw_blocks = st.raw_blocks; o->rle_blocks = st.rle_blocks;
    o->sequences = st.sequences; o->checksums_checked = st.checksums_checked; o->rounds = st.rounds; o->bytes_out = st.bytes_out;
    o->checksum_us = (uint64_t)(dev.ms[5] * 1000.0);
}
}  // namespace

// the whole zstd buffer through `sink`; LRGE_ERR_PARSE / TOO_MANY / DEVICE as lrge_hip_zstd_inflate
static int zstd_inflate_impl(lrge_hip_ctx *ctx, const uint8_t *comp, uint64_t comp_len, int (*sink)(void *, const void *, uint64_t), void *user,
                             lrge_hip_zstd_stats *stats) {
    (void)hipSetDevice(ctx->device);
    static const CodecText text = {"zstd", zs_status_name, ZS_E_TOO_BIG, "the text does not fit the device budget"};
    ZsStats st;
    ZsDev dev(ctx);
    dev.keep_max = dev_budget(ctx);                                   // (the ingest cap's default: host_fastx.inl)
    return codec_inflate(dev, text, sink, user, [&](auto &to_sink, u64 *bad) {
        return zs_run(dev, comp, comp_len, ctx->opt_u64("ZSTD_ROUND_BLOCKS", 0), zs_checksum_on(ctx), to_sink, st, bad);
    }, [&] {
        if (dev.timing) fprintf(stderr, "[lrge_hip] zstd stages ms: heads %.3f literals %.3f sequences %.3f execute %.3f resolve %.3f checksum %.3f\n", dev.ms[0], dev.ms[1],
                                dev.ms[2], dev.ms[3], dev.ms[4], dev.ms[5]);
        zs_stats_out(st, dev, stats);
    });
}

extern "C" int lrge_hip_zstd_inflate(lrge_hip_ctx *ctx, const void *comp, uint64_t comp_len, int (*sink)(void *user, const void *bytes, uint64_t n),
                                     void *user, lrge_hip_zstd_stats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (!ctx || !sink || (!comp && comp_len)) return LRGE_ERR_INVALID;
    return zstd_inflate_impl(ctx, (const uint8_t *)comp, comp_len, sink, user, stats);
}
