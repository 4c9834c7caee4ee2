// dev_keep.h -- DevKeep: a growable block of the context's pool that holds text in HBM.  The four round decoders derive from it
// (GzDev of host_gzip.inl, BzDev of host_bzip2.inl, ZsDev of host_zstd.inl, XzDev of host_xz.inl: a round's bytes are appended to
// it, or pass through it on their way to the host), and the device ingest of host_fastx.inl uses it as the block its windows pass
// through and as the store of the bases.  What a decoder inherits: the budget (dev_budget), where a round's text goes (to_host,
// deliver) and the stage timer (Lap).  Included into lrge_hip.hip through host_gzip.inl.
#pragma once
#include <functional>

namespace {
// what a call may hold on the device when no option says otherwise: half of the device's free bytes plus the arena's idle bytes
// (the batch planner's accounting: idle arena bytes are reusable)
static u64 dev_budget(lrge_hip_ctx *ctx) {
    size_t mfree = 0, mtot = 0;
    if (hipMemGetInfo(&mfree, &mtot) != hipSuccess) { (void)hipGetLastError(); mfree = 0; }
    return ((u64)mfree + ctx->pool.idle()) / 2;
}

// what the device decoders share: the first runtime error, the text that stays in HBM and the context's pinned buffers
struct DevKeep {
    lrge_hip_ctx *ctx;
    hipError_t e = hipSuccess;
    explicit DevKeep(lrge_hip_ctx *c) : ctx(c) {}
    ~DevKeep() { ctx->pool.release(keep); }
    bool ok(hipError_t x) { if (x != hipSuccess && e == hipSuccess) e = x; return e == hipSuccess; }
    // to_host: a round's bytes travel to the host through the pinned output buffer, for a sink that reads them.  Cleared
    // (host_fastx.inl): they are appended to one pool block on the device instead, and the sink does not read them.
    // The block grows geometrically (a device-to-device copy on the main stream; the pool recycles in that stream's order); more than
    // keep_max bytes stops the call with keep_over set.  The bytes count only when the call as a whole returns OK.
    bool to_host = true, keep_over = false;
    u8 *keep = nullptr;
    u64 keep_len = 0, keep_cap = 0, keep_max = 0, keep_hint = 0, keep_slack = 0, keep_floor = (u64)1 << 20, keep_grow = 2;
    // called wherever keep_len has grown, ordered on the main stream like the append itself: the windowed ingest (host_fastx.inl)
    // takes whole records off the front of the block here.  false stops the call
    std::function<bool()> keep_flush;
    bool keep_reserve(u64 more) {
        const u64 need = keep_len + more;
        if (need > keep_max) { keep_over = true; return false; }
        if (keep && need <= keep_cap) return true;
        const u64 cap = std::min<u64>(keep_max, std::max<u64>(std::max<u64>(need, keep_hint), std::max<u64>(keep_grow * keep_cap, keep_floor)));
        u8 *p = (u8 *)ctx->pool.alloc((size_t)(cap + keep_slack), &e);
        if (!p) return false;
        if (keep_len && !ok(hipMemcpyAsync(p, keep, (size_t)keep_len, hipMemcpyDeviceToDevice, ctx->stream))) { ctx->pool.release(p); return false; }
        ctx->pool.release(keep);
        keep = p; keep_cap = cap;
        return true;
    }
    bool sync() { return ok(hipStreamSynchronize(ctx->stream)); }
    // pinned host buffers of the context, kept across calls (0: input staging, 1: output)
    u8 *ctx_pin(int i, size_t bytes) {
        if (ctx->gz_pin_cap[i] >= bytes && ctx->gz_pin[i]) return ctx->gz_pin[i];
        if (ctx->gz_pin[i]) (void)hipHostFree(ctx->gz_pin[i]);
        ctx->gz_pin[i] = nullptr; ctx->gz_pin_cap[i] = 0;
        if (!ok(hipHostMalloc((void **)&ctx->gz_pin[i], bytes, hipHostMallocDefault))) { ctx->gz_pin[i] = nullptr; return nullptr; }
        ctx->gz_pin_cap[i] = bytes;
        return ctx->gz_pin[i];
    }
    // A round's `len` final bytes at d_src, for the sink (nullptr: failure).  To the host: copied to the pinned output buffer on the
    // main stream, which is drained.  Staying: they are in the block and counted in keep_len already; the windows take their turn
    // (unless `flush` says that they have had it), and the pointer only has to differ from nullptr -- the sink does not read it,
    // and a block that is still empty has no address to give
    const u8 *deliver(const u8 *d_src, u64 len, bool flush = true) {
        if (!to_host) return flush && keep_flush && !keep_flush() ? nullptr : keep ? keep : (const uint8_t *)this;
        u8 *h = ctx_pin(1, std::max<u64>(1, len));
        if (!h) return nullptr;
        return ok(hipMemcpyAsync(h, d_src, (size_t)len, hipMemcpyDeviceToHost, ctx->stream)) && sync() ? h : nullptr;
    }
    // a stage's time added to `slot` when `on`: the stream is drained at its end
    struct Lap {
        DevKeep &d; double &slot; bool on; double t0;
        Lap(DevKeep &dev, double &s, bool on_) : d(dev), slot(s), on(on_), t0(on ? DevPool::now_ms() : 0) {}
        bool end() { if (!on) return true; const bool r = d.sync(); slot += DevPool::now_ms() - t0; return r; }
    };
};
}  // namespace
