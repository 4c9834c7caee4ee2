// seed_check.hip -- the stages between the sorted minimizer stream and the anchor sort, one call each, for tests/test_gpu_seed.py: the ordered
// table build (lrge_amd/csrc/k_index.h: place_table_launch), the probe (k_lookup), the seed counts (k_seed_counts), the expansion (k_expand) and
// the expansion with the dead-pair filter (lrge_amd/csrc/k_seed.h: expand_q_launch).  The header is included as the product includes it: this
// file holds no kernel, and the table build and the k_expand_q class dispatch are the product's own host functions.  Each sc_ function takes
// host arrays, copies them into device buffers that carry a guard band in front and behind (a byte pattern), runs ONE stage on one stream,
// copies the result back and returns the stage's code; *guard_ok says whether every band still holds its pattern.  Inputs that would send a
// kernel outside its buffers (a list beyond pos[], a read number beyond the name tables) are refused on the host, before any launch.
// Not part of the ABI: include/lrge_hip.h does not declare these.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -o lrge_amd/_lib/libseed_check.so tools/seed_check.hip   (lrge_amd/build.py: build_seed_check)
#include "../lrge_amd/csrc/k_seed.h"

namespace {

const int SC_ERR_HARNESS = -1000;       // the harness's own failures (allocation, copy, refused input), never a stage's code
const size_t SC_GUARD = 4096;           // bytes of band on either side (a multiple of 256: the payload keeps the allocation's alignment)
const int SC_PATTERN = 0xA5;

lrge_hip_ctx *g_ctx = nullptr;

// one device buffer: [band | payload | band (+ back_extra)]
struct GBuf {
    u8 *raw = nullptr;
    size_t total = 0, off = 0, bytes = 0;
    ~GBuf() { release(); }
    void release() { if (raw) (void)hipFree(raw); raw = nullptr; }
    bool alloc(size_t nbytes, size_t back_extra = 0) {
        release();
        off = SC_GUARD; bytes = nbytes;
        total = (off + bytes + SC_GUARD + back_extra + 15) & ~(size_t)15;
        if (hipMalloc((void **)&raw, total) != hipSuccess) { raw = nullptr; return false; }
        return hipMemsetAsync(raw, SC_PATTERN, total, g_ctx->stream) == hipSuccess;
    }
    template <typename T> T *p() { return (T *)(raw + off); }
    bool put(const void *h, size_t nbytes, size_t at = 0) { return nbytes == 0 || hipMemcpyAsync(raw + off + at, h, nbytes, hipMemcpyHostToDevice, g_ctx->stream) == hipSuccess; }
    bool get(void *h, size_t nbytes, size_t from = 0) {
        if (nbytes == 0) return true;
        return hipMemcpyAsync(h, raw + off + from, nbytes, hipMemcpyDeviceToHost, g_ctx->stream) == hipSuccess && hipStreamSynchronize(g_ctx->stream) == hipSuccess;
    }
    bool intact() {
        std::vector<u8> f(off), b(total - off - bytes);
        if (hipMemcpyAsync(f.data(), raw, f.size(), hipMemcpyDeviceToHost, g_ctx->stream) != hipSuccess) return false;
        if (hipMemcpyAsync(b.data(), raw + off + bytes, b.size(), hipMemcpyDeviceToHost, g_ctx->stream) != hipSuccess) return false;
        if (hipStreamSynchronize(g_ctx->stream) != hipSuccess) return false;
        for (u8 x : f) if (x != SC_PATTERN) return false;
        for (u8 x : b) if (x != SC_PATTERN) return false;
        return true;
    }
};

// the table of the last sc_table call stays on the device for sc_lookup
GBuf *g_ht = nullptr;
u64 g_cap = 0, g_slots = 0; u32 g_fix = 0; bool g_ht_ok = false;

// the stream has to be idle and clean before the result counts
int finish(int rc) {
    if (hipStreamSynchronize(g_ctx->stream) != hipSuccess) { LRGE_SET_ERR(g_ctx, "synchronise: %s", hipGetErrorString(hipGetLastError())); return LRGE_ERR_DEVICE; }
    return rc;
}
#define SC_NEED(x) do { if (!(x)) { LRGE_SET_ERR(g_ctx, "harness: %s failed (%s)", #x, hipGetErrorString(hipGetLastError())); return SC_ERR_HARNESS; } } while (0)

}   // namespace

extern "C" {

// the seed side's inputs as host arrays (tests/test_gpu_seed.py mirrors this with a ctypes.Structure)
struct ScSeed {
    const u64 *qx, *qy; u64 n_mz;               // the query minimizer stream
    const u64 *hs; const u32 *hc, *hn;          // n_mz entries each (what k_lookup / k_seed_counts leave)
    const u64 *pos; u64 n_pos;                  // the index's position lists
    const u32 *t_len, *t_rank; u32 nt;
    const u32 *q_len, *q_rank; u32 nq;
    const u32 *qmz_off;                         // nq + 1
    const u32 *aoff;                            // n_mz + 1: the exclusive scan of hv
    const u32 *krank;                           // n_mz + 1, or null
    u32 pk_pos1, pk_ybits;
    i32 mid_occ, check_names, no_dual;
    u32 bits_rpos, bits_rid, bits_q;
};

int sc_init(int n_cu) {
    if (!g_ctx) {
        lrge_hip_ctx *c = new lrge_hip_ctx();
        memset(c->ms, 0, sizeof c->ms); memset(c->counters, 0, sizeof c->counters);
        c->timer_level = 0;
        if (hipStreamCreate(&c->stream) != hipSuccess) { delete c; return LRGE_ERR_DEVICE; }
        g_ctx = c;
    }
    g_ctx->n_cu = n_cu;
    return LRGE_OK;
}
void sc_shutdown() {
    if (!g_ctx) return;
    (void)hipStreamSynchronize(g_ctx->stream);
    delete g_ht; g_ht = nullptr; g_ht_ok = false;
    g_ctx->pool.destroy();
    (void)hipStreamDestroy(g_ctx->stream);
    delete g_ctx; g_ctx = nullptr;
}
const char *sc_last_error() { return g_ctx ? g_ctx->err.c_str() : "no context"; }

u32 sc_fix(int k, u32 pw) { return ht_fix_with_power(k, pw); }
u64 sc_seg_hash(u64 R, u32 sgm, u32 e, u32 nbits) { return seg_hash(R, sgm, e, nbits); }

// place_table_launch over n_runs runs of a sorted stream of M entries.  sparse == 0: h_skey (and h_ypos, when given) hold all M entries;
// sparse != 0: they hold one entry per RUN, which lands at the run's start -- the kernels read nothing else (every other entry keeps the
// band's pattern).  h_seg_start: the 256 << seg_e segment starts of a segment-packed stream, or null.  fused: the table is not cleared
// first; otherwise it is set to all ones as the index build does.  The table stays on the device for sc_lookup unless it overflowed.
int sc_table(const u64 *h_skey, const u64 *h_ypos, const u32 *h_run_start, u32 n_runs, u64 M, int sparse, u64 cap, u64 n_slots, u32 kshift, u32 fix,
             int fused, u32 pk_pos1, u32 inline_single, const u32 *h_seg_start, u32 seg_e, u32 seg_nbits, u32 max_bin, u32 grid_cap,
             u64 *h_ht, u32 *h_occ, u32 *overflow, u32 *last_slot, u64 *disp_sum, int *guard_ok) {
    g_ctx->err.clear();
    *guard_ok = 0; g_ht_ok = false;
    SC_NEED(n_runs != 0 && n_runs <= M && grid_cap != 0 && n_slots > cap / 2 && n_slots >= 1 && cap + n_runs < (1ULL << 32));
    for (u32 r = 0; r < n_runs; ++r) SC_NEED(h_run_start[r] < M && (r == 0 ? h_run_start[0] == 0 : h_run_start[r] > h_run_start[r - 1]));
    const u32 n_tiles = (u32)div_up(n_runs, PLACE_TILE), n_seg = 256u << seg_e;
    if (h_seg_start) for (u32 s = 0; s < n_seg; ++s) SC_NEED(h_seg_start[s] <= M && (s == 0 ? h_seg_start[0] == 0 : h_seg_start[s] >= h_seg_start[s - 1]));
    GBuf skey, ypos, rs, seg, bmax, occ;
    if (!g_ht) g_ht = new GBuf();
    SC_NEED(skey.alloc(M * 8)); SC_NEED(rs.alloc((size_t)n_runs * 4)); SC_NEED(bmax.alloc(((size_t)n_tiles + 1) * 4));
    SC_NEED(occ.alloc(((size_t)max_bin + 5) * 4)); SC_NEED(g_ht->alloc(2 * n_slots * 8));
    if (h_ypos) SC_NEED(ypos.alloc(M * 8));
    if (h_seg_start) { SC_NEED(seg.alloc((size_t)n_seg * 4)); SC_NEED(seg.put(h_seg_start, (size_t)n_seg * 4)); }
    if (sparse) {
        for (u32 r = 0; r < n_runs; ++r) {
            SC_NEED(skey.put(h_skey + r, 8, (size_t)h_run_start[r] * 8));
            if (h_ypos) SC_NEED(ypos.put(h_ypos + r, 8, (size_t)h_run_start[r] * 8));
        }
    } else {
        SC_NEED(skey.put(h_skey, M * 8));
        if (h_ypos) SC_NEED(ypos.put(h_ypos, M * 8));
    }
    SC_NEED(rs.put(h_run_start, (size_t)n_runs * 4));
    if (!fused) SC_NEED(hipMemsetAsync(g_ht->p<u64>(), 0xFF, 2 * n_slots * 8, g_ctx->stream) == hipSuccess);
    SC_NEED(hipMemsetAsync(occ.p<u32>(), 0, ((size_t)max_bin + 5) * 4, g_ctx->stream) == hipSuccess);
    int rc = finish(place_table_launch(g_ctx, skey.p<u64>(), rs.p<u32>(), n_runs, M, cap, n_slots, kshift, fix, fused != 0,
                                       h_ypos ? ypos.p<u64>() : (const u64 *)nullptr, pk_pos1, inline_single,
                                       SegStarts{h_seg_start ? seg.p<u32>() : (const u32 *)nullptr, seg_e, seg_nbits},
                                       bmax.p<u32>(), g_ht->p<u64>(), occ.p<u32>(), max_bin, grid_cap));
    if (rc) return rc;
    SC_NEED(g_ht->get(h_ht, 2 * n_slots * 8));
    SC_NEED(occ.get(h_occ, ((size_t)max_bin + 1) * 4));
    SC_NEED(occ.get(overflow, 4, ((size_t)max_bin + 1) * 4));
    SC_NEED(occ.get(disp_sum, 8, ((size_t)max_bin + 2 + ((max_bin + 2) & 1)) * 4));
    *last_slot = 0xFFFFFFFFu;
    if (fused) SC_NEED(bmax.get(last_slot, 4, (size_t)n_tiles * 4));
    *guard_ok = skey.intact() && rs.intact() && bmax.intact() && occ.intact() && g_ht->intact() && (!h_ypos || ypos.intact()) && (!h_seg_start || seg.intact());
    g_cap = cap; g_slots = n_slots; g_fix = fix; g_ht_ok = !*overflow && *guard_ok;
    return rc;
}

// k_lookup over the table the last sc_table call built (refused when that table overflowed: its probes have no end).  h_qx: n_mz words,
// hash << 8 | span.  h_hn: null = the kernel's hn is null.
int sc_lookup(const u64 *h_qx, u64 n_mz, i32 mid_occ, u64 *h_hs, u32 *h_hc, u32 *h_hn, int *guard_ok) {
    g_ctx->err.clear();
    *guard_ok = 0;
    SC_NEED(g_ht_ok && n_mz != 0);
    GBuf qx, hs, hc, hn;
    SC_NEED(qx.alloc(n_mz * 8)); SC_NEED(hs.alloc(n_mz * 8)); SC_NEED(hc.alloc(n_mz * 4));
    if (h_hn) SC_NEED(hn.alloc(n_mz * 4));
    SC_NEED(qx.put(h_qx, n_mz * 8));
    SeedParams sp; memset(&sp, 0, sizeof sp);
    sp.ht = g_ht->p<u64>(); sp.ht_cap = g_cap; sp.ht_fix = g_fix; sp.mid_occ = mid_occ;
    hipLaunchKernelGGL(k_lookup, dim3((u32)div_up(n_mz, 256)), dim3(256), 0, g_ctx->stream, qx.p<u64>(), n_mz, sp, hs.p<u64>(), hc.p<u32>(), h_hn ? hn.p<u32>() : (u32 *)nullptr);
    int rc = finish(hipGetLastError() == hipSuccess ? LRGE_OK : LRGE_ERR_DEVICE);
    if (rc) return rc;
    SC_NEED(hs.get(h_hs, n_mz * 8)); SC_NEED(hc.get(h_hc, n_mz * 4));
    if (h_hn) SC_NEED(hn.get(h_hn, n_mz * 4));
    *guard_ok = qx.intact() && hs.intact() && hc.intact() && (!h_hn || hn.intact()) && g_ht->intact();
    return rc;
}

}   // extern "C"

namespace {

// the device copies of one ScSeed
struct SeedDev {
    GBuf qx, qy, hs, hc, hn, pos, t_len, t_rank, q_len, q_rank, qmz_off, aoff, krank;
    SeedParams sp; KeyLayout kl;
    bool intact() {
        return qx.intact() && qy.intact() && hs.intact() && hc.intact() && hn.intact() && pos.intact() && t_len.intact() && t_rank.intact() &&
               q_len.intact() && q_rank.intact() && qmz_off.intact() && aoff.intact() && krank.intact();
    }
};
u64 y_of(const ScSeed *s, u64 w) {
    if (s->pk_ybits == 0) return w;
    const u64 yb = w & ((1ULL << s->pk_ybits) - 1);
    return (yb >> s->pk_pos1) << 32 | (yb & ((1ULL << s->pk_pos1) - 1));
}
// nothing a kernel derives from these arrays may point outside them; *raw_hits: the hits of the minimizers [b, e), an upper bound
// of what an expansion of that window can write
bool seed_valid(const ScSeed *s, const u32 *cnt, u64 b, u64 e, u64 *raw_hits) {
    *raw_hits = 0;
    if (b > e || e > s->n_mz || s->nq == 0 || s->nt == 0 || s->mid_occ < 0) return false;
    if (s->qmz_off) { for (u32 q = 0; q < s->nq; ++q) if (s->qmz_off[q] > s->qmz_off[q + 1]) return false; if (s->qmz_off[s->nq] > s->n_mz) return false; }
    for (u64 i = 0; i < s->n_mz; ++i) {
        const u32 c = cnt[i];
        if ((u32)(s->qy[i] >> 32) >= s->nq) return false;
        if (c == 0 || (i64)c > (i64)s->mid_occ) continue;
        if (s->hs[i] & HT_INLINE) { if (c != 1 || (u32)((s->hs[i] & ~HT_INLINE) >> 32) >= s->nt) return false; }
        else {
            if (s->hs[i] + c > s->n_pos) return false;
            for (u32 j = 0; j < c; ++j) if ((u32)(y_of(s, s->pos[s->hs[i] + j]) >> 32) >= s->nt) return false;
        }
        if (i >= b && i < e) *raw_hits += c;
    }
    return true;
}
int seed_put(const ScSeed *s, SeedDev &d) {
    const u64 n = s->n_mz;
    SC_NEED(d.qx.alloc(n * 8)); SC_NEED(d.qy.alloc(n * 8)); SC_NEED(d.hs.alloc(n * 8)); SC_NEED(d.hc.alloc(n * 4)); SC_NEED(d.hn.alloc(n * 4));
    SC_NEED(d.pos.alloc(s->n_pos * 8)); SC_NEED(d.t_len.alloc((size_t)s->nt * 4)); SC_NEED(d.t_rank.alloc((size_t)s->nt * 4));
    SC_NEED(d.q_len.alloc((size_t)s->nq * 4)); SC_NEED(d.q_rank.alloc((size_t)s->nq * 4)); SC_NEED(d.qmz_off.alloc(((size_t)s->nq + 1) * 4));
    SC_NEED(d.aoff.alloc((n + 1) * 4)); SC_NEED(d.krank.alloc((n + 1) * 4));
    if (s->qx) SC_NEED(d.qx.put(s->qx, n * 8));
    SC_NEED(d.qy.put(s->qy, n * 8)); SC_NEED(d.hs.put(s->hs, n * 8));
    if (s->hc) SC_NEED(d.hc.put(s->hc, n * 4));
    if (s->hn) SC_NEED(d.hn.put(s->hn, n * 4));
    SC_NEED(d.pos.put(s->pos, s->n_pos * 8));
    SC_NEED(d.t_len.put(s->t_len, (size_t)s->nt * 4)); SC_NEED(d.t_rank.put(s->t_rank, (size_t)s->nt * 4));
    SC_NEED(d.q_len.put(s->q_len, (size_t)s->nq * 4)); SC_NEED(d.q_rank.put(s->q_rank, (size_t)s->nq * 4));
    if (s->qmz_off) SC_NEED(d.qmz_off.put(s->qmz_off, ((size_t)s->nq + 1) * 4));
    if (s->aoff) SC_NEED(d.aoff.put(s->aoff, (n + 1) * 4));
    if (s->krank) SC_NEED(d.krank.put(s->krank, (n + 1) * 4));
    memset(&d.sp, 0, sizeof d.sp);
    d.sp.pos = d.pos.p<u64>(); d.sp.pk_pos1 = s->pk_pos1; d.sp.pk_ybits = s->pk_ybits;
    d.sp.t_len = d.t_len.p<u32>(); d.sp.t_rank = d.t_rank.p<u32>(); d.sp.q_len = d.q_len.p<u32>(); d.sp.q_rank = d.q_rank.p<u32>();
    d.sp.mid_occ = s->mid_occ; d.sp.check_names = s->check_names; d.sp.no_dual = s->no_dual;
    d.kl.bits_rpos = s->bits_rpos; d.kl.bits_rid = s->bits_rid; d.kl.bits_q = s->bits_q;
    return LRGE_OK;
}

}   // namespace

extern "C" {

// k_seed_counts over all n_mz minimizers (s->hc: the raw list lengths)
int sc_counts(const ScSeed *s, u32 *h_hn, u32 *h_hv, int *guard_ok) {
    g_ctx->err.clear();
    *guard_ok = 0;
    u64 raw;
    SC_NEED(s->n_mz != 0 && s->hc && seed_valid(s, s->hc, 0, s->n_mz, &raw));
    SeedDev d; GBuf hv;
    int rc = seed_put(s, d); if (rc) return rc;
    SC_NEED(hv.alloc(s->n_mz * 4));
    hipLaunchKernelGGL(k_seed_counts, dim3((u32)div_up(s->n_mz, 256)), dim3(256), 0, g_ctx->stream, d.qy.p<u64>(), s->n_mz, d.sp, d.hs.p<u64>(), d.hc.p<u32>(), d.hn.p<u32>(), hv.p<u32>());
    rc = finish(hipGetLastError() == hipSuccess ? LRGE_OK : LRGE_ERR_DEVICE);
    if (rc) return rc;
    SC_NEED(d.hn.get(h_hn, s->n_mz * 4)); SC_NEED(hv.get(h_hv, s->n_mz * 4));
    *guard_ok = d.intact() && hv.intact();
    return rc;
}

// k_expand over the minimizers [mz_begin, mz_end) (s->hn: the kept list lengths, s->aoff: the scan of hv).  packed_bits_qy != 0: the packed
// form (h_aval is not touched).  n_out = aoff[mz_end] - aoff[mz_begin] anchors come back.
int sc_expand(const ScSeed *s, u64 mz_begin, u64 mz_end, u32 q0, u32 packed_bits_qy, u64 n_out, u64 *h_akey, u64 *h_aval, int *guard_ok) {
    g_ctx->err.clear();
    *guard_ok = 0;
    u64 raw;
    SC_NEED(s->hn && s->aoff && s->qmz_off && s->qx && mz_begin < mz_end && seed_valid(s, s->hn, mz_begin, mz_end, &raw));
    SC_NEED(n_out == (u64)(s->aoff[mz_end] - s->aoff[mz_begin]) && n_out <= raw);
    for (u64 i = mz_begin; i < mz_end; ++i) SC_NEED((u32)(s->qy[i] >> 32) >= q0);
    SeedDev d; GBuf akey, aval;
    int rc = seed_put(s, d); if (rc) return rc;
    // (the bands behind the output cover whatever a wrong offset could make of the window's hits)
    SC_NEED(akey.alloc(n_out * 8, raw * 8)); SC_NEED(aval.alloc(n_out * 8, raw * 8));
    hipLaunchKernelGGL(k_expand, dim3((u32)div_up(mz_end - mz_begin, 256)), dim3(256), 0, g_ctx->stream, d.qx.p<u64>(), d.qy.p<u64>(), mz_begin, mz_end, d.sp,
                       d.hs.p<u64>(), d.hn.p<u32>(), d.aoff.p<u32>(), s->krank ? d.krank.p<u32>() : (const u32 *)nullptr, d.qmz_off.p<u32>(), q0, d.kl,
                       akey.p<u64>(), aval.p<u64>(), packed_bits_qy);
    rc = finish(hipGetLastError() == hipSuccess ? LRGE_OK : LRGE_ERR_DEVICE);
    if (rc) return rc;
    SC_NEED(akey.get(h_akey, n_out * 8));
    if (!packed_bits_qy) SC_NEED(aval.get(h_aval, n_out * 8));
    *guard_ok = d.intact() && akey.intact() && aval.intact();
    return rc;
}

// expand_q_launch for the queries [q0, q0 + nqb) into a buffer that spans the anchors of the minimizers [mz_begin, mz_end): mz_begin may lie
// in front of query q0's first minimizer and mz_end behind the last one's, so that slots of queries outside the launch exist.  h_akey
// (n_out = aoff[mz_end] - aoff[mz_begin] words) and h_kept (nqb words) go in as the test filled them and come back as the launches left them.
int sc_expand_q(const ScSeed *s, u64 mz_begin, u64 mz_end, u32 q0, u32 nqb, u32 smax, u32 mmax, u32 n_planes, u32 bits_qy, u64 n_out, u64 *h_akey, u32 *h_kept,
                int *guard_ok) {
    g_ctx->err.clear();
    *guard_ok = 0;
    u64 raw;
    SC_NEED(s->hn && s->aoff && s->qmz_off && s->qx && nqb != 0 && q0 + nqb <= s->nq && n_planes >= 1 && n_planes <= EXPQ_PLANES && bits_qy != 0);
    SC_NEED(mz_begin <= s->qmz_off[q0] && s->qmz_off[q0 + nqb] <= mz_end && seed_valid(s, s->hn, mz_begin, mz_end, &raw));
    SC_NEED(n_out == (u64)(s->aoff[mz_end] - s->aoff[mz_begin]) && n_out <= raw);
    // (a query's minimizers carry its number: the key's query field is q - q0)
    for (u32 q = q0; q < q0 + nqb; ++q) for (u64 i = s->qmz_off[q]; i < s->qmz_off[q + 1]; ++i) SC_NEED((u32)(s->qy[i] >> 32) == q);
    std::vector<u32> qtot(nqb), h_qlist;
    for (u32 q = 0; q < nqb; ++q) qtot[q] = s->aoff[s->qmz_off[q0 + q + 1]] - s->aoff[s->qmz_off[q0 + q]];     // (k_query_totals_from_scan)
    SeedDev d; GBuf akey, kept, qlist;
    int rc = seed_put(s, d); if (rc) return rc;
    SC_NEED(akey.alloc(n_out * 8, raw * 8)); SC_NEED(kept.alloc((size_t)nqb * 4)); SC_NEED(qlist.alloc((size_t)nqb * 4));
    SC_NEED(akey.put(h_akey, n_out * 8)); SC_NEED(kept.put(h_kept, (size_t)nqb * 4));
    rc = finish(expand_q_launch(g_ctx, qtot.data(), nqb, smax, mmax, n_planes, h_qlist, qlist.p<u32>(), d.qx.p<u64>(), d.qy.p<u64>(), mz_begin, d.sp,
                                d.hs.p<u64>(), d.hn.p<u32>(), d.aoff.p<u32>(), d.qmz_off.p<u32>(), q0, d.kl, akey.p<u64>(), bits_qy, kept.p<u32>()));
    if (rc) return rc;
    SC_NEED(akey.get(h_akey, n_out * 8)); SC_NEED(kept.get(h_kept, (size_t)nqb * 4));
    *guard_ok = d.intact() && akey.intact() && kept.intact() && qlist.intact();
    return rc;
}

}   // extern "C"
