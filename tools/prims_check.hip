// prims_check.hip -- the primitives of lrge_amd/csrc/k_prims.h, one call each, for tests/test_gpu_prims.py: the device-wide exclusive scan,
// the stable LSD radix sorts, the segment-local LDS sort, the segment-packed index sort and the run-head compaction.  The header is included
// as the product includes it: this file holds no kernel, every launch below is the product's own code.  Each pc_ function takes host arrays, copies them into device
// buffers that carry a guard band in front and behind (a byte pattern), calls ONE primitive on one stream, copies the result back and
// returns the primitive's return code; *guard_ok says whether every band still holds its pattern.  Word offsets shift a buffer off its
// 16-byte alignment (the scan's scalar branches).  Not part of the ABI: include/lrge_hip.h does not declare these.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -o lrge_amd/_lib/libprims_check.so tools/prims_check.hip   (lrge_amd/build.py: build_prims_check)
#include "../lrge_amd/csrc/k_prims.h"

namespace {

const int PC_ERR_HARNESS = -1000;       // the harness's own failures (allocation, copy, synchronise), never a primitive's code
const size_t PC_GUARD = 4096;           // bytes of band on either side (a multiple of 256: the payload keeps the allocation's alignment)
const int PC_PATTERN = 0xA5;

lrge_hip_ctx *g_ctx = nullptr;
int g_lsort_mask = 0;

// one device buffer: [band | off_bytes more band | payload | band]
struct GBuf {
    u8 *raw = nullptr;
    size_t total = 0, off = 0, bytes = 0;
    ~GBuf() { if (raw) (void)hipFree(raw); }
    bool alloc(size_t off_bytes, size_t nbytes) {
        off = PC_GUARD + off_bytes; bytes = nbytes;
        total = (off + bytes + PC_GUARD + 15) & ~(size_t)15;
        if (hipMalloc((void **)&raw, total) != hipSuccess) { raw = nullptr; return false; }
        return hipMemsetAsync(raw, PC_PATTERN, total, g_ctx->stream) == hipSuccess;
    }
    template <typename T> T *p() { return (T *)(raw + off); }
    bool put(const void *h, size_t nbytes) { return nbytes == 0 || hipMemcpyAsync(raw + off, h, nbytes, hipMemcpyHostToDevice, g_ctx->stream) == hipSuccess; }
    bool get(void *h, size_t nbytes, size_t from = 0) {
        if (nbytes == 0) return true;
        return hipMemcpyAsync(h, raw + off + from, nbytes, hipMemcpyDeviceToHost, g_ctx->stream) == hipSuccess && hipStreamSynchronize(g_ctx->stream) == hipSuccess;
    }
    bool intact() {
        std::vector<u8> f(off), b(total - off - bytes);
        if (hipMemcpyAsync(f.data(), raw, f.size(), hipMemcpyDeviceToHost, g_ctx->stream) != hipSuccess) return false;
        if (hipMemcpyAsync(b.data(), raw + off + bytes, b.size(), hipMemcpyDeviceToHost, g_ctx->stream) != hipSuccess) return false;
        if (hipStreamSynchronize(g_ctx->stream) != hipSuccess) return false;
        for (u8 x : f) if (x != PC_PATTERN) return false;
        for (u8 x : b) if (x != PC_PATTERN) return false;
        return true;
    }
};

void set_opts(const char *opts) {
    g_ctx->opts.clear();
    if (opts && *opts) g_ctx->opts[opts] = "1";
    g_ctx->err.clear();
}
// the stream has to be idle and clean before the result counts
int finish(int rc) {
    if (hipStreamSynchronize(g_ctx->stream) != hipSuccess) { LRGE_SET_ERR(g_ctx, "synchronise: %s", hipGetErrorString(hipGetLastError())); return LRGE_ERR_DEVICE; }
    return rc;
}
#define PC_NEED(x) do { if (!(x)) { LRGE_SET_ERR(g_ctx, "harness: %s failed (%s)", #x, hipGetErrorString(hipGetLastError())); return PC_ERR_HARNESS; } } while (0)

}   // namespace

extern "C" {

// A bare context on one stream.  *lsort_mask: bit c set = the device accepts the LDS sort variant of class c (256 / 512 / 1024 threads).
int pc_init(int *lsort_mask) {
    if (!g_ctx) {
        lrge_hip_ctx *c = new lrge_hip_ctx();
        memset(c->ms, 0, sizeof c->ms); memset(c->counters, 0, sizeof c->counters);
        c->timer_level = 0;
        if (hipStreamCreate(&c->stream) != hipSuccess) { delete c; return LRGE_ERR_DEVICE; }
        c->lsort_ok[0] = true;
        c->lsort_ok[1] = hipFuncSetAttribute((const void *)k_seg_sort_local<512, 16, LSORT_DB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LSORT_BYTES(512, 16, LSORT_DB)) == hipSuccess;
        c->lsort_ok[2] = hipFuncSetAttribute((const void *)k_seg_sort_local<1024, 16, LSORT_DB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LSORT_BYTES(1024, 16, LSORT_DB)) == hipSuccess;
        (void)hipGetLastError();
        g_lsort_mask = (c->lsort_ok[0] ? 1 : 0) | (c->lsort_ok[1] ? 2 : 0) | (c->lsort_ok[2] ? 4 : 0);
        g_ctx = c;
    }
    *lsort_mask = g_lsort_mask;
    return LRGE_OK;
}
void pc_shutdown() {
    if (!g_ctx) return;
    (void)hipStreamSynchronize(g_ctx->stream);
    g_ctx->pool.destroy();
    (void)hipStreamDestroy(g_ctx->stream);
    delete g_ctx; g_ctx = nullptr;
}
const char *pc_last_error() { return g_ctx ? g_ctx->err.c_str() : "no context"; }

u64 pc_hash_to_sig(u64 h, u32 nbits) { return hash_to_sig(h, nbits); }
u64 pc_sig_to_hash(u64 s, u32 nbits) { return sig_to_hash(s, nbits); }

// scan_exclusive_u32.  in_off / out_off: words the arrays are shifted off their alignment.  inplace: out == in (out_off is ignored).
// total_mode 0: d_total null; 1: a word of its own; 2: the word directly behind the output.  bs_mode 1: the caller's block sums
// (n / SCAN_TILE + 2 words).  h_out always receives the n output words as they stand afterwards (the band's pattern where nothing wrote).
int pc_scan(const u32 *h_in, u64 n, u32 in_off, u32 out_off, int inplace, int total_mode, int bs_mode, u32 *h_out, u32 *h_total, int *guard_ok) {
    set_opts(nullptr);
    *guard_ok = 0;
    const size_t tail = total_mode == 2 ? 4 : 0;
    GBuf in, out, tot, bs;
    PC_NEED(in.alloc((size_t)in_off * 4, n * 4 + (inplace ? tail : 0)));
    if (!inplace) PC_NEED(out.alloc((size_t)out_off * 4, n * 4 + tail));
    PC_NEED(tot.alloc(0, 4));
    if (bs_mode) PC_NEED(bs.alloc(0, (n / SCAN_TILE + 2) * 4));
    PC_NEED(in.put(h_in, n * 4));
    GBuf &o = inplace ? in : out;
    u32 *d_total = total_mode == 0 ? nullptr : total_mode == 1 ? tot.p<u32>() : o.p<u32>() + n;
    int rc;
    {
        Scratch sc(g_ctx);
        rc = finish(scan_exclusive_u32(g_ctx, sc, in.p<u32>(), o.p<u32>(), n, d_total, nullptr, false, bs_mode ? bs.p<u32>() : nullptr));
    }
    PC_NEED(o.get(h_out, n * 4));
    if (total_mode == 1) PC_NEED(tot.get(h_total, 4));
    if (total_mode == 2) PC_NEED(o.get(h_total, 4, n * 4));
    *guard_ok = in.intact() && (inplace || out.intact()) && tot.intact() && (!bs_mode || bs.intact());
    return rc;
}

// k_scan_small launched as scan_exclusive_u32 launches it (one block), on n words in place
int pc_scan_small(u32 *h_data, u32 n, int with_total, u32 *h_total, int *guard_ok) {
    set_opts(nullptr);
    *guard_ok = 0;
    GBuf d, tot;
    PC_NEED(d.alloc(0, (size_t)n * 4));
    PC_NEED(tot.alloc(0, 4));
    PC_NEED(d.put(h_data, (size_t)n * 4));
    hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(SS_THREADS), 0, g_ctx->stream, d.p<u32>(), n, with_total ? tot.p<u32>() : (u32 *)nullptr);
    int rc = hipGetLastError() == hipSuccess ? LRGE_OK : LRGE_ERR_DEVICE;
    rc = finish(rc);
    PC_NEED(d.get(h_data, (size_t)n * 4));
    PC_NEED(tot.get(h_total, 4));
    *guard_ok = d.intact() && tot.intact();
    return rc;
}

// radix_sort_pairs (unsegmented).  off0 / off1: u64 words the (k0, v0) / (k1, v1) buffers are shifted by.
int pc_sort_pairs(const u64 *h_k, const u64 *h_v, u64 n, int begin_bit, int nbits, int reverse_digits, int pass_begin, int pass_end, u32 off0, u32 off1,
                  u64 *h_ok, u64 *h_ov, int *guard_ok) {
    set_opts(nullptr);
    *guard_ok = 0;
    GBuf k0, v0, k1, v1;
    PC_NEED(k0.alloc((size_t)off0 * 8, n * 8)); PC_NEED(v0.alloc((size_t)off0 * 8, n * 8));
    PC_NEED(k1.alloc((size_t)off1 * 8, n * 8)); PC_NEED(v1.alloc((size_t)off1 * 8, n * 8));
    PC_NEED(k0.put(h_k, n * 8)); PC_NEED(v0.put(h_v, n * 8));
    u64 *rk = nullptr, *rv = nullptr;
    int rc;
    {
        Scratch sc(g_ctx);
        rc = finish(radix_sort_pairs(g_ctx, sc, k0.p<u64>(), v0.p<u64>(), k1.p<u64>(), v1.p<u64>(), n, begin_bit, nbits, &rk, &rv, reverse_digits != 0, nullptr, 0, pass_begin, pass_end));
    }
    PC_NEED((rk == k0.p<u64>() && rv == v0.p<u64>()) || (rk == k1.p<u64>() && rv == v1.p<u64>()));
    PC_NEED((rk == k0.p<u64>() ? k0 : k1).get(h_ok, n * 8));
    PC_NEED((rv == v0.p<u64>() ? v0 : v1).get(h_ov, n * 8));
    *guard_ok = k0.intact() && v0.intact() && k1.intact() && v1.intact();
    return rc;
}

// radix_sort_keys.  opts: an option of the context ("NO_DIGIT_BYTES") or null.
int pc_sort_keys(const u64 *h_k, u64 n, int begin_bit, int nbits, int reverse_digits, int pass_begin, int pass_end, const char *opts, u32 off0, u32 off1,
                 u64 *h_out, int *guard_ok) {
    set_opts(opts);
    *guard_ok = 0;
    GBuf k0, k1;
    PC_NEED(k0.alloc((size_t)off0 * 8, n * 8)); PC_NEED(k1.alloc((size_t)off1 * 8, n * 8));
    PC_NEED(k0.put(h_k, n * 8));
    u64 *res = nullptr;
    int rc;
    {
        Scratch sc(g_ctx);
        rc = finish(radix_sort_keys(g_ctx, sc, k0.p<u64>(), k1.p<u64>(), n, begin_bit, nbits, &res, reverse_digits != 0, pass_begin, pass_end));
    }
    PC_NEED(res == k0.p<u64>() || res == k1.p<u64>());
    PC_NEED((res == k0.p<u64>() ? k0 : k1).get(h_out, n * 8));
    *guard_ok = k0.intact() && k1.intact();
    return rc;
}

// radix_sort_keys_first_pass_from_slots over n_chunks slots of `cap` words (h_slots: n_chunks * cap words, h_offs: the exclusive scan of the
// per-chunk counts, n_chunks words).  rest != 0: the remaining passes follow through radix_sort_keys(pass_begin = 1).
int pc_sort_keys_from_slots(const u64 *h_slots, const u32 *h_offs, u32 n_chunks, u32 cap, u64 n, int begin_bit, int nbits, int reverse_digits, int rest,
                            const char *opts, u64 *h_out, int *guard_ok) {
    set_opts(opts);
    *guard_ok = 0;
    GBuf slots, offs, k0, k1;
    PC_NEED(slots.alloc(0, (size_t)n_chunks * cap * 8)); PC_NEED(offs.alloc(0, (size_t)n_chunks * 4));
    PC_NEED(k0.alloc(0, n * 8)); PC_NEED(k1.alloc(0, n * 8));
    PC_NEED(slots.put(h_slots, (size_t)n_chunks * cap * 8)); PC_NEED(offs.put(h_offs, (size_t)n_chunks * 4));
    u64 *res = k0.p<u64>();
    int rc;
    {
        Scratch sc(g_ctx);
        rc = radix_sort_keys_first_pass_from_slots(g_ctx, sc, slots.p<u64>(), offs.p<u32>(), n_chunks, cap, k0.p<u64>(), n, begin_bit, nbits, reverse_digits != 0);
        if (!rc && rest) rc = radix_sort_keys(g_ctx, sc, k0.p<u64>(), k1.p<u64>(), n, begin_bit, nbits, &res, reverse_digits != 0, 1);
        rc = finish(rc);
    }
    PC_NEED(res == k0.p<u64>() || res == k1.p<u64>());
    PC_NEED((res == k0.p<u64>() ? k0 : k1).get(h_out, n * 8));
    *guard_ok = slots.intact() && offs.intact() && k0.intact() && k1.intact();
    return rc;
}

// The anchor sort of one batch as OverlapRun::batch queues it: the segments of every LDS class through k_seg_sort_local, the tiles through
// radix_sort_packed_seg, all into (out_k, out_v) of n_out entries.  h_pk: n_in packed words (n_in > n_out: a sparse layout, read through
// SegDesc::src / SegTile::src).  h_segs: the SegDesc of class 0, 1, 2 back to back (n_segs[c] of each); h_tiles: n_tiles SegTile.
// A class the device refused is an error here (-(100 + class)), not a silent skip.
int pc_anchor_sort(const u64 *h_pk, u64 n_in, u64 n_out, int nbits, u32 sb, u32 bits_qy, u32 sh_q, const u32 *h_segs, const u32 *n_segs,
                   const u32 *h_tiles, u32 n_tiles, u64 n_items, int src_first, const char *opts, u64 *h_ok, u64 *h_ov, int *guard_ok) {
    set_opts(opts);
    *guard_ok = 0;
    static_assert(sizeof(SegDesc) == 16 && sizeof(SegTile) == 32, "the descriptors travel as plain words");
    const u64 n0 = n_in > n_out ? n_in : n_out;
    const u32 n_seg_all = n_segs[0] + n_segs[1] + n_segs[2];
    for (int c = 0; c < 3; ++c) if (n_segs[c] && !g_ctx->lsort_ok[c]) { LRGE_SET_ERR(g_ctx, "the device refused LDS sort class %d", c); return -(100 + c); }
    GBuf pk0, pk1, ok, ov, segs, tiles;
    PC_NEED(pk0.alloc(0, n0 * 8)); PC_NEED(pk1.alloc(0, n_out * 8)); PC_NEED(ok.alloc(0, n_out * 8)); PC_NEED(ov.alloc(0, n_out * 8));
    PC_NEED(segs.alloc(0, (size_t)n_seg_all * sizeof(SegDesc))); PC_NEED(tiles.alloc(0, (size_t)n_tiles * sizeof(SegTile)));
    PC_NEED(pk0.put(h_pk, n_in * 8));
    PC_NEED(segs.put(h_segs, (size_t)n_seg_all * sizeof(SegDesc))); PC_NEED(tiles.put(h_tiles, (size_t)n_tiles * sizeof(SegTile)));
    UnpackParams up; up.sb = sb; up.bits_qy = bits_qy; up.sh_q = sh_q;
    const SegDesc *d0 = segs.p<SegDesc>(), *d1 = d0 + n_segs[0], *d2 = d1 + n_segs[1];
    int rc = LRGE_OK;
    {
        Scratch sc(g_ctx);
        if (n_segs[2]) hipLaunchKernelGGL((k_seg_sort_local<1024, 16, LSORT_DB>), dim3(n_segs[2]), dim3(1024), LSORT_BYTES(1024, 16, LSORT_DB), g_ctx->stream, pk0.p<u64>(), ok.p<u64>(), ov.p<u64>(), d2, up, nbits);
        if (n_segs[1]) hipLaunchKernelGGL((k_seg_sort_local<512, 16, LSORT_DB>), dim3(n_segs[1]), dim3(512), LSORT_BYTES(512, 16, LSORT_DB), g_ctx->stream, pk0.p<u64>(), ok.p<u64>(), ov.p<u64>(), d1, up, nbits);
        if (n_segs[0]) hipLaunchKernelGGL((k_seg_sort_local<256, 8, 8>), dim3(n_segs[0]), dim3(256), LSORT_BYTES(256, 8, 8), g_ctx->stream, pk0.p<u64>(), ok.p<u64>(), ov.p<u64>(), d0, up, nbits);
        if (hipGetLastError() != hipSuccess) rc = LRGE_ERR_DEVICE;
        if (!rc) rc = radix_sort_packed_seg(g_ctx, sc, pk0.p<u64>(), pk1.p<u64>(), ok.p<u64>(), ov.p<u64>(), n_out, nbits, tiles.p<SegTile>(), n_tiles, up, n_items, src_first != 0);
        rc = finish(rc);
    }
    PC_NEED(ok.get(h_ok, n_out * 8)); PC_NEED(ov.get(h_ov, n_out * 8));
    *guard_ok = pk0.intact() && pk1.intact() && ok.intact() && ov.intact() && segs.intact() && tiles.intact();
    return rc;
}

// The segment-packed index sort over n entries in one of its three source forms.  form 0: (hash, y) pairs (h_x, h_y); 1: dense SEGW entries, the
// words h_x and the DIG members h_dig; 2: the wave-dense sketch's slots -- n_waves slots of `cap` words h_x and DIG members h_dig, h_cnt entries in
// each, h_offs their exclusive scan.  h_words receives the n packed words, h_seg_start the (256 << e) + 1 segment starts.  The sort releases its
// inputs to the pool; the guarded buffers here are none of the pool's, so that is a no-op.  The result may lie in a pool block of the sort's own.
int pc_index_sort(int form, const u64 *h_x, const u64 *h_y, const u32 *h_dig, const u32 *h_cnt, const u32 *h_offs, u32 n_waves, u32 cap, u64 n, int nbits,
                  u32 ybits, u32 pos1, u32 e, const char *opts, u64 *h_words, u32 *h_seg_start, int *guard_ok) {
    set_opts(opts);
    *guard_ok = 0;
    const size_t n_in = form == 2 ? (size_t)n_waves * cap : n, mb = form == 0 ? 8 : 4;      // input entries; bytes of the second member
    GBuf x, m, cnt, offs, k1, m1;
    PC_NEED(x.alloc(0, n_in * 8)); PC_NEED(m.alloc(0, n_in * mb)); PC_NEED(k1.alloc(0, n * 8)); PC_NEED(m1.alloc(0, n * mb));
    PC_NEED(x.put(h_x, n_in * 8)); PC_NEED(m.put(form == 0 ? (const void *)h_y : (const void *)h_dig, n_in * mb));
    if (form == 2) {
        PC_NEED(cnt.alloc(0, (size_t)n_waves * 4)); PC_NEED(offs.alloc(0, (size_t)n_waves * 4));
        PC_NEED(cnt.put(h_cnt, (size_t)n_waves * 4)); PC_NEED(offs.put(h_offs, (size_t)n_waves * 4));
    }
    u64 *res = nullptr; u32 *d_seg = nullptr;
    Scratch sc(g_ctx);
    const WaveSrc ws{x.p<u64>(), m.p<u32>(), cnt.p<u32>(), offs.p<u32>(), n_waves, cap};
    IndexSortIn in;
    if (form == 0) { in.x = x.p<u64>(); in.y = m.p<u64>(); }
    else if (form == 1) { in.x = x.p<u64>(); in.dig = m.p<u32>(); }
    else in.ws = &ws;
    const int rc = finish(index_sort_seg(g_ctx, sc, in, k1.p<u64>(), m1.p<u64>(), n, nbits, ybits, pos1, e, &res, &d_seg));
    if (!rc) {
        PC_NEED(res && d_seg);
        PC_NEED(hipMemcpy(h_words, res, n * 8, hipMemcpyDeviceToHost) == hipSuccess);
        PC_NEED(hipMemcpy(h_seg_start, d_seg, (((size_t)256 << e) + 1) * 4, hipMemcpyDeviceToHost) == hipSuccess);
    }
    *guard_ok = x.intact() && m.intact() && k1.intact() && m1.intact() && (form != 2 || (cnt.intact() && offs.intact()));
    return rc;
}

// compact_heads (async == 0; h_seg_start: n_seg + 1 forced boundaries or null) and compact_heads_async (async != 0: a starts buffer of
// n + 1 entries, no boundaries).  h_starts: room for n + 1 entries; *n_heads of them are returned.
int pc_heads(const u64 *h_keys, u64 n, u32 shift, const u32 *h_seg_start, u32 n_seg, int async, u32 *h_starts, u32 *n_heads, int *guard_ok) {
    set_opts(nullptr);
    *guard_ok = 0; *n_heads = 0;
    GBuf keys, segs, starts, cnt;
    PC_NEED(keys.alloc(0, n * 8)); PC_NEED(keys.put(h_keys, n * 8));
    PC_NEED(cnt.alloc(0, 4));
    if (h_seg_start) { PC_NEED(segs.alloc(0, ((size_t)n_seg + 1) * 4)); PC_NEED(segs.put(h_seg_start, ((size_t)n_seg + 1) * 4)); }
    int rc;
    Scratch sc(g_ctx);
    if (async) {
        PC_NEED(starts.alloc(0, (n + 1) * 4));
        rc = finish(compact_heads_async(g_ctx, sc, keys.p<u64>(), n, shift, starts.p<u32>(), cnt.p<u32>()));
        PC_NEED(cnt.get(n_heads, 4));
        if (!rc && *n_heads <= n) PC_NEED(starts.get(h_starts, (size_t)*n_heads * 4));
        *guard_ok = starts.intact();
    } else {
        u32 *d_st = nullptr;
        rc = finish(compact_heads(g_ctx, sc, keys.p<u64>(), n, shift, &d_st, n_heads, h_seg_start ? segs.p<u32>() : nullptr, n_seg));
        if (!rc && d_st && *n_heads <= n) PC_NEED(hipMemcpy(h_starts, d_st, (size_t)*n_heads * 4, hipMemcpyDeviceToHost) == hipSuccess);
        *guard_ok = 1;
    }
    *guard_ok = *guard_ok && keys.intact() && cnt.intact() && (!h_seg_start || segs.intact());
    return rc;
}

}   // extern "C"
