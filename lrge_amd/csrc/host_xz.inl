// host_xz.inl -- xz decompressed on the device (k_xz.h): the backend that xz_round.h's xz_run drives and the C
// entry point.  Included into lrge_hip.hip behind host_gzip.inl (DevKeep, GzBuf).
//
// The compressed bytes and the chunk table go up once and stay for the call.  A round's text is reserved behind the text so far in
// the backend's DevKeep block; a block never reads another block's text, so lrge_hip_xz_inflate hands a finished round to the
// sink and uses the room again, and the windowed ingest flushes it (keep_flush).  Options XZ_ROUND_BLOCKS: the blocks decoded per
// round; its default is what half of the arena's idle bytes plus the device's free bytes hold at the largest block's text plus a
// state slot per block, at most XZ_ROUND_MAX.  XZ_LAUNCH_BYTES: the text a block may produce per launch, whole chunks, one at
// least (default 2 MiB, the format's largest chunk).  XZ_CHECK (default 1): 0 skips the block checks.  XZ_MIN_BLOCKS (default 64,
// measured: BASELINE section 13): a file with fewer blocks is refused -- one wavefront decodes about 1 MB/s, liblzma 60 MB/s.  XZ_TIMING: the stage times are printed to stderr when the call ends (tools/xz_bench.py);
// every launch is followed by the read of its status words anyway, so the times are always measured.

static const char *xz_status_name(int s) {
    switch (s) {
    case XZ_E_MAGIC: return "no stream header where a stream must start";
    case XZ_E_INPUT: return "unexpected end of compressed data";
    case XZ_E_FOOTER: return "no stream footer where a stream must end";
    case XZ_E_RESERVED: return "a reserved bit is set";
    case XZ_E_CHECK_ID: return "a check other than none, CRC32 or CRC64";
    case XZ_E_HEADER_CRC: return "header, footer or index CRC32 mismatch";
    case XZ_E_FLAGS: return "stream header and footer flags differ";
    case XZ_E_INDEX: return "an invalid index";
    case XZ_E_FILTER: return "a filter chain other than LZMA2 alone";
    case XZ_E_PADDING: return "padding that is not zero bytes in multiples of four";
    case XZ_E_SIZES: return "sizes of a block that do not agree";
    case XZ_E_CONTROL: return "an invalid LZMA2 control byte";
    case XZ_E_PROPS: return "invalid LZMA properties";
    case XZ_E_DICT_SIZE: return "an invalid dictionary size";
    case XZ_E_DIST: return "a distance beyond the dictionary";
    case XZ_E_END_MARKER: return "an end marker";
    case XZ_E_MATCH_CROSS: return "a match that crosses its chunk";
    case XZ_E_RC: return "a range decoder that does not start or end as its chunk states";
    case XZ_E_CHECK: return "block check mismatch";
    case XZ_E_FEW_BLOCKS: return "fewer blocks than XZ_MIN_BLOCKS";
    case XZ_E_TOO_BIG: return "the text does not fit the device budget";
    default: return "unknown status";
    }
}

namespace {
struct XzDev : DevKeep {
    GzBuf in, table, tasks, slots, status, spans, crc;
    bool timing = false;
    double ms[3] = {0, 0, 0};                                      // upload, decode, check
    explicit XzDev(lrge_hip_ctx *c) : DevKeep(c) {
        for (GzBuf *b : {&in, &table, &tasks, &slots, &status, &spans, &crc}) b->ctx = c;
        timing = c->opt("XZ_TIMING") != nullptr;
    }
    ~XzDev() { (void)hipStreamSynchronize(ctx->stream); }
    bool over() const { return keep_over; }
    bool load(const uint8_t *d, uint64_t len, const XzChunk *c, uint64_t n_chunks) {
        Lap lap(*this, ms[0], true);                               // (always: the stream is drained here whether the time is wanted or not)
        if (!in.need((size_t)len + 16, &e) || !table.need((size_t)(n_chunks + 1) * sizeof(XzChunk), &e)) return false;
        if (len && !ok(hipMemcpyAsync(in.p, d, (size_t)len, hipMemcpyHostToDevice, ctx->stream))) return false;
        if (n_chunks && !ok(hipMemcpyAsync(table.p, c, (size_t)n_chunks * sizeof(XzChunk), hipMemcpyHostToDevice, ctx->stream))) return false;
        return lap.end();
    }
    uint32_t default_round(uint64_t block_bytes) { return (uint32_t)std::min<u64>(XZ_ROUND_MAX, std::max<u64>(1, dev_budget(ctx) / (block_bytes + XZ_SLOT_BYTES))); }
    bool reserve(uint64_t bytes, uint32_t k) {
        if (!keep_reserve(bytes)) return false;
        if (!slots.need((size_t)k * XZ_SLOT_BYTES, &e)) return false;
        return ok(hipMemsetAsync(slots.p, 0, (size_t)k * XZ_SLOT_BYTES, ctx->stream));
    }
    bool decode(const XzTask *t, uint32_t m, uint32_t *st_h, uint32_t *bad_h) {
        Lap lap(*this, ms[1], true);
        hipStream_t st = ctx->stream;
        if (!tasks.need((size_t)m * sizeof(XzTask), &e) || !status.need((size_t)m * 8, &e)) return false;
        if (!ok(hipMemcpyAsync(tasks.p, t, (size_t)m * sizeof(XzTask), hipMemcpyHostToDevice, st)) || !ok(hipMemsetAsync(status.p, 0, (size_t)m * 8, st))) return false;
        hipLaunchKernelGGL(k_xz_decode, dim3(m), dim3(64), 0, st, in.as<const u8>(), table.as<const XzChunk>(), tasks.as<const XzTask>(), m, keep + keep_len, slots.as<u8>(),
                           status.as<u32>(), status.as<u32>() + m);
        if (!ok(hipGetLastError())) return false;
        if (!ok(hipMemcpyAsync(st_h, status.p, (size_t)m * 4, hipMemcpyDeviceToHost, st)) ||
            !ok(hipMemcpyAsync(bad_h, status.as<u32>() + m, (size_t)m * 4, hipMemcpyDeviceToHost, st)))
            return false;
        return lap.end();
    }
    bool check(const XzSpan *s, uint32_t m, uint64_t *c) {
        Lap lap(*this, ms[2], true);
        if (!spans.need((size_t)m * sizeof(XzSpan), &e) || !crc.need((size_t)m * 8, &e)) return false;
        if (!ok(hipMemcpyAsync(spans.p, s, (size_t)m * sizeof(XzSpan), hipMemcpyHostToDevice, ctx->stream))) return false;
        hipLaunchKernelGGL(k_xz_check, dim3(m), dim3(64), 0, ctx->stream, (const u8 *)(keep + keep_len), spans.as<const XzSpan>(), m, crc.as<u64>());
        if (!ok(hipGetLastError())) return false;
        if (!ok(hipMemcpyAsync(c, crc.p, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream))) return false;
        return lap.end();
    }
    const uint8_t *commit(uint64_t bytes) {
        const u8 *round = keep + keep_len;
        if (!to_host) keep_len += bytes;                           // (to the host keep_len stays: the next round takes the same room)
        return deliver(round, bytes);
    }
};

static XzCfg xz_cfg(lrge_hip_ctx *ctx) {
    return XzCfg{ctx->opt_u64("XZ_ROUND_BLOCKS", 0), ctx->opt_u64("XZ_LAUNCH_BYTES", 0), ctx->opt_u64("XZ_MIN_BLOCKS", XZ_MIN_BLOCKS_DEFAULT), ctx->opt_u64("XZ_CHECK", 1) != 0};
}
static void xz_stats_out(const XzStats &st, const XzDev &dev, lrge_hip_xz_stats *o) {
    if (!o) return;
    o->streams = st.streams; o->blocks = st.blocks; o->chunks = st.chunks; o->raw_chunks = st.raw_chunks; o->checks_checked = st.checks_checked;
    o->rounds = st.rounds; o->launches = st.launches; o->bytes_out = st.bytes_out;
    o->check_us = (uint64_t)(dev.ms[2] * 1000.0); o->decode_us = (uint64_t)(dev.ms[1] * 1000.0); o->walk_us = st.walk_us;
}
}  // namespace

// the whole xz buffer through `sink`; LRGE_ERR_PARSE / TOO_MANY / DEVICE as lrge_hip_xz_inflate
static int xz_inflate_impl(lrge_hip_ctx *ctx, const uint8_t *comp, uint64_t comp_len, int (*sink)(void *, const void *, uint64_t), void *user,
                           lrge_hip_xz_stats *stats) {
    (void)hipSetDevice(ctx->device);
    static const CodecText text = {"xz", xz_status_name, XZ_E_TOO_BIG, "the text does not fit the device budget"};
    XzStats st;
    XzDev dev(ctx);
    dev.keep_max = dev_budget(ctx);                                     // (a round's text; the ingest cap's default: host_fastx.inl)
    return codec_inflate(dev, text, sink, user, [&](auto &to_sink, u64 *bad) { return xz_run(dev, comp, comp_len, xz_cfg(ctx), to_sink, st, bad); }, [&] {
        if (dev.timing) fprintf(stderr, "[lrge_hip] xz stages ms: walk %.3f upload %.3f decode %.3f check %.3f\n", st.walk_us / 1000.0, dev.ms[0], dev.ms[1], dev.ms[2]);
        xz_stats_out(st, dev, stats);
    });
}

extern "C" int lrge_hip_xz_inflate(lrge_hip_ctx *ctx, const void *comp, uint64_t comp_len, int (*sink)(void *user, const void *bytes, uint64_t n),
                                   void *user, lrge_hip_xz_stats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (!ctx || !sink || (!comp && comp_len)) return LRGE_ERR_INVALID;
    return xz_inflate_impl(ctx, (const uint8_t *)comp, comp_len, sink, user, stats);
}
