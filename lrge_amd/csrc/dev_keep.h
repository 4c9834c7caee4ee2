// dev_keep.h -- DevKeep: a growable block of the context's pool that holds text in HBM.  The device decoders derive from it (GzDev
// of host_gzip.inl, BzDev of host_bzip2.inl: every round's bytes are appended to it), and the device ingest of host_fastx.inl uses
// it as the block its windows pass through and as the store of the bases.  Included into lrge_hip.hip through those three files.
#pragma once
#include <functional>

namespace {
// what the device decoders share: the first runtime error, the text that stays in HBM and the context's pinned buffers
struct DevKeep {
    lrge_hip_ctx *ctx;
    hipError_t e = hipSuccess;
    explicit DevKeep(lrge_hip_ctx *c) : ctx(c) {}
    ~DevKeep() { ctx->pool.release(keep); }
    bool ok(hipError_t x) { if (x != hipSuccess && e == hipSuccess) e = x; return e == hipSuccess; }
    // keep_on (host_fastx.inl): every round's bytes are appended to one pool block on the device instead of travelling to the host.
    // The block grows geometrically (a device-to-device copy on the main stream; the pool recycles in that stream's order); more than
    // keep_max bytes stops the call with keep_over set.  The bytes count only when the call as a whole returns OK.
    bool keep_on = false, keep_over = false;
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
};
}  // namespace
