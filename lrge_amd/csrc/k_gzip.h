// k_gzip.h -- speculative parallel inflate of plain / multi-member gzip on the device.
//
//   k_gz_find     one 256-thread workgroup per nominal chunk: the lanes test consecutive bit offsets (the 13-bit header test
//                 of gz_maybe_candidate first, the full gz_is_candidate only for the survivors, with per-lane tables in LDS);
//                 the smallest passing offset, or GZ_NONE.
//   k_gz_decode   one wavefront per chunk, wave-uniform like k_inflate (whose LDS tables and wavefront-scope loads it shares): gz_decode from the chunk's candidate to its stop.
//                 The last 32 Ki symbols live in an LDS ring of u16 (back-references never leave LDS); every symbol also
//                 streams to the chunk's HBM slot.
//   k_gz_window   one workgroup walks the round's accepted chunks in order: the window of chunk k+1 is the last 32 KiB of
//                 (window k ++ chunk k resolved).  Sequential, but 32 KiB per chunk, held in LDS.
//   k_gz_resolve  a grid over every symbol of the round (tiles of 256 lanes x 1 KiB stripes): symbols to bytes through the
//                 chunk's window, written at the chunk's output offset, and the CRC-32 of each lane's piece of each member
//                 segment, shifted to the segment's end and XOR-combined (vector atomics) into the segment's CRC.
#pragma once
#include "internal.h"
#include "k_inflate.h"
#include "gzip_core.h"
#include "gzip_round.h"

#define GZ_FIND_THREADS 256
#define GZ_STRIPE 1024u
#define GZ_RESOLVE_THREADS 256
#define GZ_TILE (GZ_STRIPE * GZ_RESOLVE_THREADS)

struct GzTile { u32 link, s0; };

__global__ __launch_bounds__(GZ_FIND_THREADS) void k_gz_find(const u8 *__restrict__ in, u32 n, u32 chunk, u32 lim, u32 *__restrict__ cand) {
    __shared__ u8 tab[GZ_FIND_THREADS * 128];
    __shared__ u16 cnt[GZ_FIND_THREADS * 32];
    __shared__ u32 best;
    const u32 c = blockIdx.x + 1, t = threadIdx.x;
    const u32 b0 = 8 * c * chunk;
    const u32 b1 = 8 * (u32)min((u64)(c + 1) * chunk, (u64)lim);
    if (t == 0) best = GZ_NONE;
    __syncthreads();
    for (u32 base = b0; base < b1; base += GZ_FIND_THREADS) {
        const u32 bit = base + t;
        if (bit < b1 && gz_maybe_candidate(in, n, bit) && gz_is_candidate(in, n, bit, tab + t * 128, cnt + t * 32)) atomicMin(&best, bit);
        __syncthreads();
        const u32 found = best;
        __syncthreads();
        if (found != GZ_NONE) break;
    }
    if (t == 0) cand[c] = best;
}

struct alignas(16) GzLds {
    u16 ring[GZ_WIN];
    InfLdsTabs tabs;
};

struct GzDevEnv : InfDevTabs {
    static constexpr int full = GZ_E_OVERFLOW;
    u16 *ring;
    u16 *out;              // the chunk's HBM slot
    GzSeg *sp;
    u32 pos, cap;
    bool own;              // the current member started in this chunk, at symbol mstart (set by gz_decode)
    u32 mstart;
    __device__ GzDevEnv(GzLds &S, u32 lane_, u16 *out_, GzSeg *sp_, u32 cap_) : InfDevTabs(S.tabs, lane_), ring(S.ring), out(out_), sp(sp_), pos(0), cap(cap_) {}
    __device__ u32 reach() const { return own ? pos - mstart : pos + GZ_WIN; }
    __device__ void put(u32 i, u16 v) { st_wave(ring + (i & (GZ_WIN - 1)), v); out[i] = v; }
    __device__ void lit(u8 b) { if (lane == 0) put(pos, b); ++pos; }
    __device__ void copy(u32 dist, u32 len) {
        for (u32 c = 0; c < len; c += 64) {                   // len <= 258: at most 5 steps
            const u32 j = c + lane;
            if (j < len) {
                // j >= dist repeats the first dist symbols: the source is always before pos (see k_inflate.h)
                const i64 src = (i64)pos - dist + (j < dist ? j : j % dist);
                put(pos + j, src >= 0 ? ld_wave(ring + ((u32)src & (GZ_WIN - 1))) : (u16)(GZ_MARK | (u32)(GZ_WIN + src)));
            }
        }
        pos += len;
    }
    __device__ void stored(const u8 *src, u32 n) {
        for (u32 j = lane; j < n; j += 64) put(pos + j, src[j]);
        pos += n;
    }
    __device__ void seg(u32 i, const GzSeg &s) { if (lane == 0) sp[i] = s; }
};

__global__ __launch_bounds__(64) void k_gz_decode(const u8 *__restrict__ in, u32 n, u32 eof, const GzTask *__restrict__ tasks, u32 nt,
                                                  u16 *__restrict__ sym, GzSeg *__restrict__ seg, GzRes *__restrict__ res) {
    __shared__ GzLds S;
    const u32 k = blockIdx.x, lane = threadIdx.x;
    if (k >= nt) return;
    const GzTask T = tasks[k];
    GzDevEnv e(S, lane, sym + T.sym_off, seg + T.seg_off, T.cap);
    GzRes r;
    gz_decode(e, in, n, eof != 0, T.start, T.stop, T.seg_cap, r);
    if (lane == 0) res[k] = r;
}

// the symbols of link L
__device__ __forceinline__ const u16 *gz_link_sym(const GzLink &L, const u16 *sym, const u16 *const *big) {
    return (L.big ? big[L.big - 1] : sym) + L.sym_off;
}

__global__ __launch_bounds__(1024) void k_gz_window(const GzLink *__restrict__ links, u32 nl, const u16 *sym, const u16 *const *big,
                                                    u8 *__restrict__ carry, u8 *__restrict__ windows) {
    __shared__ u8 w[2][GZ_WIN];
    const u32 t = threadIdx.x;
    for (u32 j = t; j < GZ_WIN; j += 1024) w[0][j] = carry[j];
    __syncthreads();
    for (u32 k = 0; k < nl; ++k) {
        const u8 *cur = w[k & 1];
        u8 *nxt = w[(k + 1) & 1];
        const GzLink L = links[k];
        const u16 *sy = gz_link_sym(L, sym, big);
        for (u32 j = t; j < GZ_WIN; j += 1024) {
            windows[(u64)k * GZ_WIN + j] = cur[j];
            const u64 idx = (u64)L.n_sym + j;                    // in (window ++ chunk)
            u32 v;
            if (idx < GZ_WIN) v = cur[idx];
            else { v = sy[idx - GZ_WIN]; if (v >= 256) v = cur[v & (GZ_WIN - 1)]; }
            nxt[j] = (u8)v;
        }
        __syncthreads();
    }
    for (u32 j = t; j < GZ_WIN; j += 1024) carry[j] = w[nl & 1][j];
}

__global__ __launch_bounds__(GZ_RESOLVE_THREADS) void k_gz_resolve(const GzLink *__restrict__ links, const GzTile *__restrict__ tiles,
                                                                   const u16 *sym, const u16 *const *big, const u8 *__restrict__ windows,
                                                                   const GzSeg *__restrict__ segs, u8 *__restrict__ out,
                                                                   u32 *__restrict__ seg_crc, u32 *__restrict__ err) {
    __shared__ u32 tab[256];
    __shared__ u32 pw[32];
    const u32 t = threadIdx.x;
    inf_crc_table(tab, t, GZ_RESOLVE_THREADS);
    if (t == 0) gz_crc_powers(pw, 32);
    __syncthreads();
    const GzTile T = tiles[blockIdx.x];
    const GzLink L = links[T.link];
    const u32 a = T.s0 + t * GZ_STRIPE;
    const u32 z = min(a + GZ_STRIPE, L.n_sym);
    if (a >= z) return;
    const u16 *sy = gz_link_sym(L, sym, big);
    const u8 *win = windows + (u64)T.link * GZ_WIN;
    u8 *o = out + L.out_off;
    const GzSeg *sg = segs + L.seg0;
    u32 lo = 0, hi = L.nseg;                                   // the first segment that ends after a
    while (lo < hi) { const u32 m = (lo + hi) >> 1; if (sg[m].o1 > a) hi = m; else lo = m + 1; }
    u32 g = lo, ps = a, c = 0xFFFFFFFFu;
    const u32 bad_below = GZ_WIN - L.valid;
    bool bad = false;
    for (u32 i = a; i < z; ++i) {
        while (g < L.nseg && i >= sg[g].o1) {                  // a segment ends at i: its piece [ps, i)
            if (i > ps) atomicXor(seg_crc + L.seg0 + g, gz_crc_shift_tab(pw, ~c, sg[g].o1 - i));
            ++g; ps = i; c = 0xFFFFFFFFu;
        }
        const u32 v = sy[i];
        u32 b = v;
        if (v >= 256) { b = win[v & (GZ_WIN - 1)]; bad |= (v & (GZ_WIN - 1)) < bad_below; }
        o[i] = (u8)b;
        c = gz_crc_run(tab, c, (u8)b);
    }
    if (g < L.nseg && z > ps) atomicXor(seg_crc + L.seg0 + g, gz_crc_shift_tab(pw, ~c, sg[g].o1 - z));
    if (bad) atomicMin(err, T.link + 1);                     // (0xFFFFFFFF: none)
}

// ---- the seek map ----
// k_gz_win_pick: the windows of the links a census keeps as entries, gathered out of `windows` into one block that comes down in one copy
// (a workgroup a window, 16 bytes a lane and step)
__global__ __launch_bounds__(256) void k_gz_win_pick(const u8 *__restrict__ windows, const u32 *__restrict__ link, u8 *__restrict__ out) {
    const uint4 *src = reinterpret_cast<const uint4 *>(windows + (u64)link[blockIdx.x] * GZ_WIN);
    uint4 *dst = reinterpret_cast<uint4 *>(out + (u64)blockIdx.x * GZ_WIN);
    for (u32 j = threadIdx.x; j < GZ_WIN / 16; j += 256) dst[j] = src[j];
}

// k_gz_entry: one wavefront an entry, gz_decode from the entry's bit to the next entry's with the window preloaded into a byte ring in
// LDS (gzip_core.h GzSeedEnv): no markers, no window chain, no resolve.  74 KiB of LDS a workgroup, two on a CU, as k_gz_decode.
struct alignas(16) GzEntryLds {
    u8 ring[GZ_RING];
    InfLdsTabs tabs;
    u32 crc_tab[256];
    u32 pw[32];
};

struct GzSeedDevMem {
    __device__ static u8 ld(const u8 *p) { return ld_wave(p); }
    __device__ static void st(u8 *p, u8 v) { st_wave(p, v); }
    __device__ static void word(u8 *p, u32 w) { *reinterpret_cast<u32 *>(p) = w; }
    __device__ static u32 wave_xor(u32 c) { for (int m = 32; m; m >>= 1) c ^= (u32)__shfl_xor((int)c, m); return c; }
};
typedef GzSeedEnv<InfDevTabs, GzSeedDevMem> GzSeedDevEnv;

__global__ __launch_bounds__(64) void k_gz_entry(const u8 *__restrict__ comp, const GzEntryTask *__restrict__ tasks, u32 nt, const u8 *__restrict__ wins,
                                                 u8 *__restrict__ stage, u32 *__restrict__ status) {
    __shared__ GzEntryLds S;
    const u32 k = blockIdx.x, lane = threadIdx.x;
    if (k >= nt) return;
    inf_crc_table(S.crc_tab, lane, 64);
    if (lane == 0) gz_crc_powers(S.pw, 32);
    const GzEntryTask T = tasks[k];
    u8 *dst = stage + T.out_off;
    GzSeedDevEnv e(S.ring, S.crc_tab, S.pw, dst, (u32)((uintptr_t)dst & 3u), T.len, T.valid, S.tabs, lane);
    if (T.win != GZ_NONE) e.preload(wins + (u64)T.win * GZ_WIN);
    __syncthreads();
    const u32 rc = gz_entry_run(e, comp + T.c_off, T);
    if (lane == 0) status[k] = rc;
}
