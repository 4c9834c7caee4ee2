// host_inflate.inl -- BGZF decompression on the device (k_inflate.h): the block scan and the chunked pipeline, for the bytes on
// the host and for text that stays in HBM (host_fastx.inl) alike; the record reader is the one of host_gzip.inl with the BGZF
// path alone.  Included into lrge_hip.hip.
//
// The block table of a BGZF buffer (bgzf_scan.h) is cut into chunks that end on block boundaries and hold at most
// INFLATE_CHUNK_BYTES (option; compressed + decompressed bytes, default 256 MiB, at least one block).  Two slots of pinned
// host and device buffers, each sized for the largest chunk, keep HBM use bounded whatever the file size: the upload of
// chunk i+1 (copy stream), the decode of chunk i (main stream) and the download of chunk i-1 (side stream) overlap, and the
// host reads the status words of a chunk once, when its download has finished.  With a resident destination the slots hold no
// output: the decode writes into the block and the status words alone come down.

static const char *inf_status_name(u32 s) {
    switch (s) {
    case INF_E_BTYPE: return "invalid block type";
    case INF_E_STORED: return "invalid stored block lengths";
    case INF_E_CODES: return "invalid code lengths";
    case INF_E_SYMBOL: return "invalid code";
    case INF_E_DIST: return "invalid distance too far back";
    case INF_E_INPUT: return "compressed data does not end with the block";
    case INF_E_OUTPUT: return "more output than ISIZE";
    case INF_E_SIZE: return "less output than ISIZE";
    case INF_E_CRC: return "CRC32 mismatch";
    default: return "block not decoded";
    }
}

extern "C" int lrge_hip_bgzf_scan(const void *comp, uint64_t comp_len, uint64_t *n_blocks, uint64_t *out_len) {
    if (!comp && comp_len) return LRGE_ERR_INVALID;
    std::vector<BgzfBlock> t;
    uint64_t total = 0;
    if (!bgzf_scan_blocks((const uint8_t *)comp, comp_len, &t, &total)) { g_last_error = "not a BGZF buffer"; return LRGE_ERR_PARSE; }
    if (n_blocks) *n_blocks = t.size();
    if (out_len) *out_len = total;
    return LRGE_OK;
}

struct BgzfBad { u32 status; u64 c_off; };      // the first block that failed its checks (INF_OK: none did), its file offset

// Every block of `t` (a table of `comp`) decoded into [0, sum of ISIZE) of d_out, a block resident in HBM, or, when d_out is
// null, of h_out, a host buffer (null only where no block has output).  LRGE_OK with *bad the first block that failed (the
// destination is not to be used then), or LRGE_ERR_DEVICE with "<what>: <the runtime's text>".
// comp_pinned: `comp` is pinned host memory already (the slots of the streamed source, host_fastx.inl): a chunk's bytes go up from
// where they lie, and the pipeline's own pinned slots hold the block tables alone.
static int bgzf_inflate_chunks(lrge_hip_ctx *ctx, const uint8_t *comp, const std::vector<BgzfBlock> &t, uint8_t *h_out, u8 *d_out, const char *what, BgzfBad *bad,
                               bool comp_pinned = false) {
    struct Chunk { size_t b0, b1; u64 c0, cn, o0, on; };
    const u64 limit = std::max<u64>(1, ctx->opt_u64("INFLATE_CHUNK_BYTES", (u64)256 << 20));
    std::vector<Chunk> ch;
    u64 max_c = 0, max_o = 0; size_t max_n = 0;
    for (size_t i = 0; i < t.size();) {
        Chunk c{i, i, t[i].c_off, 0, t[i].o_off, 0};
        while (c.b1 < t.size() && (c.b1 == i || c.cn + c.on + t[c.b1].c_len + t[c.b1].isize <= limit) &&
               c.cn + t[c.b1].c_len < ((u64)1 << 31) && c.on + t[c.b1].isize < ((u64)1 << 31)) {
            c.cn += t[c.b1].c_len; c.on += t[c.b1].isize; ++c.b1;
        }
        max_c = std::max(max_c, c.cn); max_o = std::max(max_o, c.on); max_n = std::max(max_n, c.b1 - c.b0);
        ch.push_back(c);
        i = c.b1;
    }
    *bad = BgzfBad{INF_OK, 0};
    if (ch.empty()) return LRGE_OK;
    (void)hipSetDevice(ctx->device);
    const size_t a16 = 16;
    auto up16 = [&](u64 x) { return (size_t)((x + a16 - 1) & ~(u64)(a16 - 1)); };
    // slot layout, the same on both sides: [input | block table] up, [output (host destination only) | status words] down
    const size_t tab_off = up16(max_c), up_bytes = tab_off + up16(max_n * sizeof(InfBlk));
    const size_t st_off = d_out ? 0 : up16(max_o), dn_bytes = st_off + up16(max_n * 4);
    u8 *d_up[2] = {nullptr, nullptr}, *d_dn[2] = {nullptr, nullptr}, *h_up[2] = {nullptr, nullptr}, *h_dn[2] = {nullptr, nullptr};
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_k[2] = {nullptr, nullptr}, ev_dn[2] = {nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int s = 0; s < 2 && e == hipSuccess; ++s) {
        if (!(d_up[s] = (u8 *)ctx->pool.alloc(up_bytes, &e)) || !(d_dn[s] = (u8 *)ctx->pool.alloc(dn_bytes, &e))) break;
        if ((e = hipHostMalloc((void **)&h_up[s], comp_pinned ? up_bytes - tab_off : up_bytes, hipHostMallocDefault)) != hipSuccess) break;
        if ((e = hipHostMalloc((void **)&h_dn[s], dn_bytes, hipHostMallocDefault)) != hipSuccess) break;
        if ((e = hipEventCreateWithFlags(&ev_up[s], hipEventDisableTiming)) != hipSuccess) break;
        if ((e = hipEventCreateWithFlags(&ev_k[s], hipEventDisableTiming)) != hipSuccess) break;
        e = hipEventCreateWithFlags(&ev_dn[s], hipEventDisableTiming);
    }
    // the host's share of chunk k: status words, then (host destination) the bytes
    auto finish = [&](size_t k) -> hipError_t {
        const int s = (int)(k & 1);
        const Chunk &c = ch[k];
        hipError_t he = hipEventSynchronize(ev_dn[s]);
        if (he != hipSuccess) return he;
        const u32 *st = (const u32 *)(h_dn[s] + st_off);
        for (size_t i = 0; i < c.b1 - c.b0; ++i)
            if (st[i] != INF_OK && bad->status == INF_OK) *bad = BgzfBad{st[i], t[c.b0 + i].c_off};
        if (!d_out && c.on && bad->status == INF_OK) memcpy(h_out + c.o0, h_dn[s], (size_t)c.on);
        return hipSuccess;
    };
    for (size_t k = 0; k <= ch.size() && e == hipSuccess && bad->status == INF_OK; ++k) {
        if (k < ch.size()) {
            const int s = (int)(k & 1);
            const Chunk &c = ch[k];
            const u32 n = (u32)(c.b1 - c.b0);
            // k_inflate stores 4-byte words aligned relative to its output pointer: in the resident block, where a chunk starts
            // at any offset, the pointer is the chunk's start rounded down (a slot's buffer holds its chunk from byte 0)
            const u32 lead = d_out ? (u32)(c.o0 & 3) : 0;
            u8 *dst = d_out ? d_out + (c.o0 - lead) : d_dn[s];
            if (!comp_pinned) memcpy(h_up[s], comp + c.c0, (size_t)c.cn);
            InfBlk *tb = (InfBlk *)(h_up[s] + (comp_pinned ? 0 : tab_off));
            for (u32 i = 0; i < n; ++i) {
                const BgzfBlock &b = t[c.b0 + i];
                tb[i] = InfBlk{(u32)(b.c_off - c.c0) + b.d_off, b.d_len, (u32)(b.o_off - c.o0) + lead, b.isize, b.crc};
            }
            if (comp_pinned) {
                if (c.cn && (e = hipMemcpyAsync(d_up[s], comp + c.c0, (size_t)c.cn, hipMemcpyHostToDevice, ctx->copy_stream)) != hipSuccess) break;
                if ((e = hipMemcpyAsync(d_up[s] + tab_off, tb, (size_t)n * sizeof(InfBlk), hipMemcpyHostToDevice, ctx->copy_stream)) != hipSuccess) break;
            } else if ((e = hipMemcpyAsync(d_up[s], h_up[s], tab_off + (size_t)n * sizeof(InfBlk), hipMemcpyHostToDevice, ctx->copy_stream)) != hipSuccess) break;
            if ((e = hipEventRecord(ev_up[s], ctx->copy_stream)) != hipSuccess) break;
            if ((e = hipStreamWaitEvent(ctx->stream, ev_up[s], 0)) != hipSuccess) break;
            hipLaunchKernelGGL(k_inflate, dim3(n), dim3(64), 0, ctx->stream, d_up[s], (const InfBlk *)(d_up[s] + tab_off), n, dst, (u32 *)(d_dn[s] + st_off));
            if ((e = hipGetLastError()) != hipSuccess) break;
            if ((e = hipEventRecord(ev_k[s], ctx->stream)) != hipSuccess) break;
            if ((e = hipStreamWaitEvent(ctx->stream2, ev_k[s], 0)) != hipSuccess) break;
            if (!d_out && c.on && (e = hipMemcpyAsync(h_dn[s], d_dn[s], (size_t)c.on, hipMemcpyDeviceToHost, ctx->stream2)) != hipSuccess) break;
            if ((e = hipMemcpyAsync(h_dn[s] + st_off, d_dn[s] + st_off, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream2)) != hipSuccess) break;
            if ((e = hipEventRecord(ev_dn[s], ctx->stream2)) != hipSuccess) break;
        }
        if (k >= 1) e = finish(k - 1);
    }
    (void)hipStreamSynchronize(ctx->copy_stream); (void)hipStreamSynchronize(ctx->stream); (void)hipStreamSynchronize(ctx->stream2);
    int rc = LRGE_OK;
    if (e != hipSuccess) { LRGE_SET_ERR(ctx, "%s: %s", what, hipGetErrorString(e)); (void)hipGetLastError(); rc = LRGE_ERR_DEVICE; }
    for (int s = 0; s < 2; ++s) {
        ctx->pool.release(d_up[s]); ctx->pool.release(d_dn[s]);
        if (h_up[s]) (void)hipHostFree(h_up[s]);
        if (h_dn[s]) (void)hipHostFree(h_dn[s]);
        if (ev_up[s]) (void)hipEventDestroy(ev_up[s]);
        if (ev_k[s]) (void)hipEventDestroy(ev_k[s]);
        if (ev_dn[s]) (void)hipEventDestroy(ev_dn[s]);
    }
    return rc;
}

// the same into a host buffer, for the callers that hand the bytes on: LRGE_ERR_PARSE names the first bad block's file offset
static int bgzf_inflate_table(lrge_hip_ctx *ctx, const uint8_t *comp, const std::vector<BgzfBlock> &t, uint8_t *out) {
    BgzfBad bad;
    const int rc = bgzf_inflate_chunks(ctx, comp, t, out, nullptr, "bgzf inflate", &bad);
    if (rc || bad.status == INF_OK) return rc;
    LRGE_SET_ERR(ctx, "BGZF block at file offset %llu: %s", (unsigned long long)bad.c_off, inf_status_name(bad.status));
    return LRGE_ERR_PARSE;
}

extern "C" int lrge_hip_bgzf_inflate(lrge_hip_ctx *ctx, const void *comp, uint64_t comp_len, void *out, uint64_t out_len) {
    if (!ctx || (!comp && comp_len)) return LRGE_ERR_INVALID;
    std::vector<BgzfBlock> t;
    uint64_t total = 0;
    if (!bgzf_scan_blocks((const uint8_t *)comp, comp_len, &t, &total)) { ctx->err = "not a BGZF buffer"; return LRGE_ERR_PARSE; }
    if (out_len < total || (!out && total)) { LRGE_SET_ERR(ctx, "bgzf inflate: output buffer of %llu bytes, %llu needed", (unsigned long long)out_len, (unsigned long long)total); return LRGE_ERR_INVALID; }
    return bgzf_inflate_table(ctx, (const uint8_t *)comp, t, (uint8_t *)out);
}

extern "C" int lrge_hip_read_records_gpu(lrge_hip_ctx *ctx, const char *path, void (*cb)(void *, const char *, uint64_t, const char *, uint64_t),
                                         void *user, int *used_device) {
    return lrge_hip_read_records_gpu_ex(ctx, path, LRGE_GPU_INFLATE_BGZF, cb, user, used_device);      // (host_gzip.inl)
}
