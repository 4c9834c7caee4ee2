// host_gzip.inl -- plain and multi-member gzip decompressed on the device (k_gzip.h): the backend that
// gzip_round.h's gz_run drives, the C entry point and the record reader with both device paths.  Included into lrge_hip.hip.
//
// Options: GZIP_CHUNK_BYTES (nominal chunk, default 512 KiB), GZIP_ROUND_BYTES (compressed bytes per round, default 256 MiB:
// device memory stays bounded whatever the file size), GZIP_SLOT_RATIO (symbols per compressed byte of a chunk's slot,
// default 8; an overflowing chunk is decoded again once with 4x, then the call gives LRGE_ERR_TOO_MANY).  Rounds overlap: the
// next round's bytes go up through pinned memory on the copy stream and the last round's come down on the side stream while
// a round decodes; the pinned buffers are kept in the context across calls.

#include "dev_keep.h"
#include "fx_input.h"

static const char *gz_status_name(u32 s) {
    switch (s) {
    case GZ_E_HEADER: return "invalid gzip member header or trailing bytes";
    case GZ_E_CRC: return "member CRC32 or ISIZE mismatch";
    case GZ_E_MARKER: return "invalid distance too far back";
    case INF_E_INPUT: return "unexpected end of compressed data";
    default: return inf_status_name(s);
    }
}

namespace {
// a device buffer of the context's pool that grows on demand (contents are not kept)
struct GzBuf {
    lrge_hip_ctx *ctx = nullptr;
    void *p = nullptr;
    size_t cap = 0;
    bool need(size_t bytes, hipError_t *e) {
        if (bytes <= cap && p) return true;
        ctx->pool.release(p); p = nullptr; cap = 0;
        if (!(p = ctx->pool.alloc(std::max<size_t>(bytes, 256), e))) return false;
        cap = std::max<size_t>(bytes, 256);
        return true;
    }
    template <class T> T *as() const { return (T *)p; }
    ~GzBuf() { if (ctx) ctx->pool.release(p); }
};

struct GzDev : DevKeep {
    GzBuf cand, tasks, res, sym, seg, links, tiles, windows, fsegs, seg_crc, err, out, carry, bigtab;
    std::vector<GzBuf *> big_sym, big_seg;
    std::vector<const u16 *> big_ptr;
    uint32_t n = 0;
    u64 S = 0; u32 SG = 0;
    explicit GzDev(lrge_hip_ctx *c, const GzCfg &cfg) : DevKeep(c) {
        for (GzBuf *b : {&cand, &tasks, &res, &sym, &seg, &links, &tiles, &windows, &fsegs, &seg_crc, &err, &out, &carry, &bigtab}) b->ctx = c;
        in2[0].ctx = c; in2[1].ctx = c;
        S = gz_slot_symbols(cfg); SG = gz_slot_segs(cfg);
        if (carry.need(GZ_WIN, &e)) ok(hipMemsetAsync(carry.p, 0, GZ_WIN, ctx->stream));
        ok(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
        ok(hipEventCreateWithFlags(&ev_out, hipEventDisableTiming));
    }
    ~GzDev() {
        (void)hipStreamSynchronize(ctx->copy_stream); (void)hipStreamSynchronize(ctx->stream2); (void)hipStreamSynchronize(ctx->stream);
        drop_big();
        if (ev_in) (void)hipEventDestroy(ev_in);
        if (ev_out) (void)hipEventDestroy(ev_out);
    }
    void drop_big() {
        for (GzBuf *b : big_sym) delete b;
        for (GzBuf *b : big_seg) delete b;
        big_sym.clear(); big_seg.clear(); big_ptr.clear();
    }

    // the round's input: two device slots, the next round staged through pinned memory on the copy stream while this one decodes
    GzBuf in2[2];
    int cur = 0;
    u64 pf_off = 0; u32 pf_len = 0; bool pf = false;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    // src: the streamed first pass -- the round's bytes are read from the file into the pinned buffer, `d` is a
    // null base; a read that fails stops the run (io_failed: the caller reports an IO error, not a device failure)
    const FxInput *src = nullptr;
    bool io_failed = false;
    bool stage(const uint8_t *d, u64 off, u32 len, int slot, hipStream_t st) {
        u8 *h = ctx_pin(0, len);
        if (!h || !in2[slot].need(len, &e)) return false;
        if (!src) memcpy(h, d + off, len);
        else if (!src->read(off, len, h)) { io_failed = true; return false; }
        return ok(hipMemcpyAsync(in2[slot].p, h, len, hipMemcpyHostToDevice, st));
    }
    void prefetch(const uint8_t *d, uint64_t off, uint32_t len) {
        if (e != hipSuccess) return;
        pf = stage(d, off, len, cur ^ 1, ctx->copy_stream) && ok(hipEventRecord(ev_in, ctx->copy_stream));
        pf_off = off; pf_len = len;
    }
    bool load(const uint8_t *d, uint64_t off, uint32_t len) {
        n = len;
        if (pf) {
            pf = false;
            if (!ok(hipStreamWaitEvent(ctx->stream, ev_in, 0))) return false;
            if (off >= pf_off && off + len <= pf_off + pf_len) { cur ^= 1; in_ptr = in2[cur].as<const u8>() + (off - pf_off); return true; }
            if (!ok(hipEventSynchronize(ev_in))) return false;        // (the pinned buffer is free again)
        }
        if (!stage(d, off, len, cur ^ 1, ctx->stream) || !sync()) return false;   // (the pinned buffer is free again)
        cur ^= 1; in_ptr = in2[cur].as<const u8>();
        return true;
    }
    const u8 *in_ptr = nullptr;
    uint32_t pend_nt = 0;
    bool wait(GzRes *r) {
        if (!ok(hipMemcpyAsync(r, res.p, (size_t)pend_nt * sizeof(GzRes), hipMemcpyDeviceToHost, ctx->stream))) return false;
        return sync();
    }
    bool bytes_ready() { return ok(hipEventSynchronize(ev_out)); }
    bool find(uint32_t chunk, uint32_t nc, uint32_t lim, uint32_t *c) {
        if (!cand.need((size_t)nc * 4, &e)) return false;
        hipLaunchKernelGGL(k_gz_find, dim3(nc - 1), dim3(GZ_FIND_THREADS), 0, ctx->stream, in_ptr, n, chunk, lim, cand.as<u32>());
        if (!ok(hipGetLastError())) return false;
        if (!ok(hipMemcpyAsync(c + 1, cand.as<u32>() + 1, (size_t)(nc - 1) * 4, hipMemcpyDeviceToHost, ctx->stream))) return false;
        return sync();
    }
    bool launch(const GzTask *t, uint32_t nt, bool eof) {
        u64 need_s = 0, need_g = 0;
        for (uint32_t i = 0; i < nt; ++i) { need_s = std::max<u64>(need_s, t[i].sym_off + t[i].cap); need_g = std::max<u64>(need_g, (u64)t[i].seg_off + t[i].seg_cap); }
        GzBuf *a = &sym, *b = &seg;
        if (t[0].big) {                                          // (every task of the call in one extra buffer of its own)
            a = new GzBuf; b = new GzBuf;
            a->ctx = ctx; b->ctx = ctx;
            big_sym.push_back(a); big_seg.push_back(b);
        }
        if (!a->need((size_t)need_s * 2, &e) || !b->need((size_t)need_g * sizeof(GzSeg), &e)) return false;
        if (t[0].big) big_ptr.push_back(a->as<const u16>());
        u16 *sy = a->as<u16>(); GzSeg *sg = b->as<GzSeg>();
        if (!tasks.need((size_t)nt * sizeof(GzTask), &e) || !res.need((size_t)nt * sizeof(GzRes), &e)) return false;
        if (!ok(hipMemcpyAsync(tasks.p, t, (size_t)nt * sizeof(GzTask), hipMemcpyHostToDevice, ctx->stream))) return false;
        hipLaunchKernelGGL(k_gz_decode, dim3(nt), dim3(64), 0, ctx->stream, in_ptr, n, (u32)eof, tasks.as<const GzTask>(), nt, sy, sg, res.as<GzRes>());
        pend_nt = nt;
        return ok(hipGetLastError());
    }
    bool decode(const GzTask *t, uint32_t nt, bool eof, GzRes *r) { return launch(t, nt, eof) && wait(r); }
    bool segs(const GzTask &t, uint32_t k, GzSeg *o) {
        const GzSeg *src = (t.big ? big_seg[t.big - 1]->as<const GzSeg>() : seg.as<const GzSeg>()) + t.seg_off;
        return ok(hipMemcpy(o, src, (size_t)k * sizeof(GzSeg), hipMemcpyDeviceToHost));
    }
    bool finish(const GzLink *l, uint32_t nl, const GzSeg *s, uint32_t ns, uint64_t out_bytes, uint32_t *seg_crc_h, uint32_t *marker_err,
                const uint8_t **bytes) {
        std::vector<GzTile> tl;
        for (uint32_t k = 0; k < nl; ++k) for (u32 s0 = 0; s0 < l[k].n_sym; s0 += GZ_TILE) tl.push_back(GzTile{k, s0});
        if (!links.need((size_t)nl * sizeof(GzLink), &e) || !tiles.need(std::max<size_t>(1, tl.size()) * sizeof(GzTile), &e) ||
            !windows.need((size_t)nl * GZ_WIN, &e) || !fsegs.need(std::max<size_t>(1, ns) * sizeof(GzSeg), &e) ||
            !seg_crc.need(std::max<size_t>(1, ns) * 4, &e) || !err.need(4, &e) || !out.need(std::max<u64>(1, out_bytes), &e) ||
            !bigtab.need(std::max<size_t>(1, big_ptr.size()) * sizeof(void *), &e))
            return false;
        u8 *h_out = to_host ? ctx_pin(1, std::max<u64>(1, out_bytes)) : nullptr;
        if (!h_out && to_host) return false;
        hipStream_t st = ctx->stream;
        if (!ok(hipMemcpyAsync(links.p, l, (size_t)nl * sizeof(GzLink), hipMemcpyHostToDevice, st))) return false;
        if (!tl.empty() && !ok(hipMemcpyAsync(tiles.p, tl.data(), tl.size() * sizeof(GzTile), hipMemcpyHostToDevice, st))) return false;
        if (ns && !ok(hipMemcpyAsync(fsegs.p, s, (size_t)ns * sizeof(GzSeg), hipMemcpyHostToDevice, st))) return false;
        if (!big_ptr.empty() && !ok(hipMemcpyAsync(bigtab.p, big_ptr.data(), big_ptr.size() * sizeof(void *), hipMemcpyHostToDevice, st))) return false;
        if (!ok(hipMemsetAsync(seg_crc.p, 0, std::max<size_t>(1, ns) * 4, st)) || !ok(hipMemsetAsync(err.p, 0xFF, 4, st))) return false;
        hipLaunchKernelGGL(k_gz_window, dim3(1), dim3(1024), 0, st, links.as<const GzLink>(), nl, sym.as<const u16>(), bigtab.as<const u16 *const>(),
                           carry.as<u8>(), windows.as<u8>());
        if (!ok(hipGetLastError())) return false;
        if (!tl.empty()) {
            hipLaunchKernelGGL(k_gz_resolve, dim3((u32)tl.size()), dim3(GZ_RESOLVE_THREADS), 0, st, links.as<const GzLink>(), tiles.as<const GzTile>(),
                               sym.as<const u16>(), bigtab.as<const u16 *const>(), windows.as<const u8>(), fsegs.as<const GzSeg>(), out.as<u8>(),
                               seg_crc.as<u32>(), err.as<u32>());
            if (!ok(hipGetLastError())) return false;
        }
        if (ns && !ok(hipMemcpyAsync(seg_crc_h, seg_crc.p, (size_t)ns * 4, hipMemcpyDeviceToHost, st))) return false;
        if (!ok(hipMemcpyAsync(marker_err, err.p, 4, hipMemcpyDeviceToHost, st))) return false;
        if (!to_host) {                                          // the round's bytes stay in HBM, behind what the earlier rounds left
            if (!keep_reserve(out_bytes)) return false;
            if (out_bytes && !ok(hipMemcpyAsync(keep + keep_len, out.p, out_bytes, hipMemcpyDeviceToDevice, st))) return false;
            keep_len += out_bytes;
            if (keep_flush && !keep_flush()) return false;
        }
        // the bytes travel on the side stream while the next round is staged and decoded (bytes_ready waits for them)
        if (!ok(hipEventRecord(ev_out, st)) || !ok(hipStreamWaitEvent(ctx->stream2, ev_out, 0))) return false;
        if (to_host && out_bytes && !ok(hipMemcpyAsync(h_out, out.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream2))) return false;
        if (!ok(hipEventRecord(ev_out, ctx->stream2))) return false;
        if (!sync()) return false;
        if (*marker_err == 0xFFFFFFFFu) *marker_err = 0;
        drop_big();
        *bytes = to_host ? h_out : keep;
        return true;
    }
    // the recorder of a seek map (gzip_round.h GzSeekRec) takes the windows of the links it keeps as entries: `windows` still holds the
    // round's; one gather, one copy down
    GzBuf pick_idx, pick;
    bool windows_out(const uint32_t *link, uint32_t k, uint8_t *dst) {
        pick_idx.ctx = ctx; pick.ctx = ctx;
        if (!pick_idx.need((size_t)k * 4, &e) || !pick.need((size_t)k * GZ_WIN, &e)) return false;
        if (!ok(hipMemcpyAsync(pick_idx.p, link, (size_t)k * 4, hipMemcpyHostToDevice, ctx->stream))) return false;
        hipLaunchKernelGGL(k_gz_win_pick, dim3(k), dim3(256), 0, ctx->stream, windows.as<const u8>(), pick_idx.as<const u32>(), pick.as<u8>());
        if (!ok(hipGetLastError())) return false;
        return ok(hipMemcpyAsync(dst, pick.p, (size_t)k * GZ_WIN, hipMemcpyDeviceToHost, ctx->stream)) && sync();
    }
};
}  // namespace

static GzCfg gz_cfg(lrge_hip_ctx *ctx) {
    return GzCfg{ctx->opt_u64("GZIP_CHUNK_BYTES", (u64)512 << 10), ctx->opt_u64("GZIP_ROUND_BYTES", (u64)256 << 20), ctx->opt_u64("GZIP_SLOT_RATIO", 8)};
}

// ---- the common entry of the four round decoders (gzip, bzip2, Zstandard, xz) ----
// What differs between them behind the driver: the name in the messages, the text of a driver status, and the status that means
// "too big" (LRGE_ERR_TOO_MANY, with its message; 0: the codec has none)
struct CodecText { const char *name; const char *(*status_name)(int); int too_big; const char *too_big_msg; };
static_assert((int)GZ_RUN_OK == (int)BZ_RUN_OK && (int)GZ_RUN_DEVICE == (int)BZ_RUN_DEVICE && (int)GZ_RUN_OK == (int)ZS_RUN_OK && (int)GZ_RUN_DEVICE == (int)ZS_RUN_DEVICE &&
              (int)GZ_RUN_OK == (int)XZ_RUN_OK && (int)GZ_RUN_DEVICE == (int)XZ_RUN_DEVICE, "one set of driver codes");
// run(to_sink, &bad) drives the backend `dev` (gz_run, bz_run, zs_run, xz_run) with the C sink behind to_sink; done() copies the
// stats out and prints the stage line while the backend still holds its times.  OK, a sink that stopped, a device failure, too
// big and any other status become LRGE_OK, LRGE_ERR_IO, LRGE_ERR_DEVICE, LRGE_ERR_TOO_MANY and LRGE_ERR_PARSE
template <class Dev, class Run, class Done>
static int codec_inflate(Dev &dev, const CodecText &c, int (*sink)(void *, const void *, uint64_t), void *user, Run run, Done done) {
    lrge_hip_ctx *ctx = dev.ctx;
    u64 bad = 0;
    bool sink_stop = false;
    auto to_sink = [&](const uint8_t *b, uint64_t k) {
        if (sink(user, b, k) != 0) { sink_stop = true; return false; }
        return true;
    };
    const int rc = dev.e == hipSuccess ? run(to_sink, &bad) : (int)GZ_RUN_DEVICE;
    if (rc == GZ_RUN_DEVICE && !sink_stop) {
        LRGE_SET_ERR(ctx, "%s inflate: %s", c.name, hipGetErrorString(dev.e != hipSuccess ? dev.e : hipErrorUnknown));
        (void)hipGetLastError();
    }
    (void)hipStreamSynchronize(ctx->stream);
    done();
    if (rc == GZ_RUN_OK) return LRGE_OK;
    if (sink_stop) { LRGE_SET_ERR(ctx, "%s inflate: the sink stopped the call", c.name); return LRGE_ERR_IO; }
    if (rc == GZ_RUN_DEVICE) return LRGE_ERR_DEVICE;
    if (c.too_big && rc == c.too_big) { LRGE_SET_ERR(ctx, "%s inflate: %s", c.name, c.too_big_msg); return LRGE_ERR_TOO_MANY; }
    LRGE_SET_ERR(ctx, "%s data at file offset %llu: %s", c.name, (unsigned long long)bad, c.status_name(rc));
    return LRGE_ERR_PARSE;
}

// the whole gzip buffer through `sink`; LRGE_ERR_PARSE / TOO_MANY / DEVICE as lrge_hip_gzip_inflate
static int gzip_inflate_impl(lrge_hip_ctx *ctx, const uint8_t *comp, uint64_t comp_len, int (*sink)(void *, const void *, uint64_t), void *user,
                             lrge_hip_gzip_stats *stats) {
    (void)hipSetDevice(ctx->device);
    static const CodecText text = {"gzip", [](int s) { return gz_status_name((u32)s); }, GZ_RUN_TOO_MANY, "a chunk decodes to more symbols than its slot holds"};
    const GzCfg cfg = gz_cfg(ctx);
    GzStats st;
    GzDev dev(ctx, cfg);
    return codec_inflate(dev, text, sink, user, [&](auto &to_sink, u64 *bad) { return gz_run(dev, comp, comp_len, cfg, to_sink, st, bad); }, [&] {
        if (!stats) return;
        stats->members = st.members; stats->chunks = st.chunks; stats->speculative_starts = st.speculative; stats->rejected_starts = st.rejected;
        stats->redecoded_chunks = st.redecoded; stats->overflow_retries = st.overflow_retries; stats->bytes_out = st.bytes_out;
    });
}

extern "C" int lrge_hip_gzip_inflate(lrge_hip_ctx *ctx, const void *comp, uint64_t comp_len, int (*sink)(void *user, const void *bytes, uint64_t n),
                                     void *user, lrge_hip_gzip_stats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (!ctx || !sink || (!comp && comp_len)) return LRGE_ERR_INVALID;
    return gzip_inflate_impl(ctx, (const uint8_t *)comp, comp_len, sink, user, stats);
}

// (host_bzip2.inl)
static int bzip2_inflate_impl(lrge_hip_ctx *ctx, const uint8_t *comp, uint64_t comp_len, int (*sink)(void *, const void *, uint64_t), void *user,
                              lrge_hip_bzip2_stats *stats);
// (host_zstd.inl)
static int zstd_inflate_impl(lrge_hip_ctx *ctx, const uint8_t *comp, uint64_t comp_len, int (*sink)(void *, const void *, uint64_t), void *user,
                             lrge_hip_zstd_stats *stats);
// (host_xz.inl)
static int xz_inflate_impl(lrge_hip_ctx *ctx, const uint8_t *comp, uint64_t comp_len, int (*sink)(void *, const void *, uint64_t), void *user,
                           lrge_hip_xz_stats *stats);

extern "C" int lrge_hip_read_records_gpu_ex(lrge_hip_ctx *ctx, const char *path, int flags,
                                            void (*cb)(void *, const char *, uint64_t, const char *, uint64_t), void *user, int *used_device) {
    if (!ctx || !path || !cb) return LRGE_ERR_INVALID;
    if (used_device) *used_device = 0;
    struct DeviceFail { int rc; };
    int used = 0;
    // a round decoder behind the hook, when the caller's flags name it: false for input the device does not accept or cannot prove
    // (the host path, with its messages)
    const auto through = [&](int flag, auto impl, const std::string &raw, std::string &data) -> bool {
        if (!(flags & flag)) return false;
        data.clear();
        const int rc = impl(ctx, (const uint8_t *)raw.data(), raw.size(), [](void *u, const void *b, uint64_t k) {
            ((std::string *)u)->append((const char *)b, (size_t)k);
            return 0;
        }, &data, nullptr);
        if (rc == LRGE_ERR_DEVICE) throw DeviceFail{rc};
        if (rc != LRGE_OK) { data.clear(); return false; }
        used = 1;
        return true;
    };
    try {
        lrge::io::iter_records(path, [&](const std::string &n, const std::string &s) { cb(user, n.data(), (uint64_t)n.size(), s.data(), (uint64_t)s.size()); },
                               [&](const std::string &raw, std::string &data) -> bool {
            const lrge::io::CompressionFormat fmt = lrge::io::detect_compression_format(raw);
            if (fmt == lrge::io::CompressionFormat::Bzip2) return through(LRGE_GPU_INFLATE_BZIP2, bzip2_inflate_impl, raw, data);
            if (fmt == lrge::io::CompressionFormat::Zstd) return through(LRGE_GPU_INFLATE_ZSTD, zstd_inflate_impl, raw, data);
            if (fmt == lrge::io::CompressionFormat::Xz) return through(LRGE_GPU_INFLATE_XZ, xz_inflate_impl, raw, data);
            std::vector<BgzfBlock> t;
            uint64_t total = 0;
            if (bgzf_scan_blocks((const uint8_t *)raw.data(), raw.size(), &t, &total)) {
                if (!(flags & LRGE_GPU_INFLATE_BGZF)) return false;
                data.resize((size_t)total);
                const int rc = bgzf_inflate_table(ctx, (const uint8_t *)raw.data(), t, (uint8_t *)&data[0]);
                if (rc == LRGE_ERR_DEVICE) throw DeviceFail{rc};
                if (rc != LRGE_OK) { data.clear(); return false; }
                used = 1;
                return true;
            }
            return through(LRGE_GPU_INFLATE_GZIP, gzip_inflate_impl, raw, data);
        });
    } catch (const DeviceFail &) {
        return LRGE_ERR_DEVICE;
    } catch (const std::exception &e) {
        ctx->err = e.what();
        if (used_device) *used_device = used;
        return strncmp(e.what(), "cannot open", 11) == 0 ? LRGE_ERR_IO : LRGE_ERR_PARSE;
    }
    if (used_device) *used_device = used;
    return LRGE_OK;
}
