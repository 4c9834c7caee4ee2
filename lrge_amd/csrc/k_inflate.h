// k_inflate.h -- BGZF block decode on the device: one wavefront (a 64-lane workgroup) per block.
//
// The bit reader and symbol decode of inflate_core.h run wave-uniform (every lane holds the same state; the loads are
// made uniform with readfirstlane).  The block's whole output (ISIZE <= 64 KiB) is assembled in LDS, so every
// back-reference is a short LDS read; literals are stored by lane 0, match copies and stored blocks are spread over the
// lanes (an overlapping copy -- distance shorter than the length -- reads out[pos - dist + j % dist], always a byte
// before pos, so the lanes of a copy never depend on one another).  The CRC-32 is computed over 64 lane stripes and
// combined (inf_crc_stripe), then the block is written to its output offset with coalesced stores.  A block that fails
// any check writes nothing but its status word.
#pragma once
#include "internal.h"
#include "inflate_core.h"

// one block of a chunk: offsets relative to the chunk's input / output buffers (a chunk is < 2 GiB on either side)
struct InfBlk { u32 c_off, d_len, o_off, isize, crc; };

// the code tables and code lengths of one wavefront's decoder, in LDS
struct InfLdsTabs {
    InfCode lt, dt, ct;
    u8 lens[320];
};

struct alignas(16) InfLds {
    u8 out[INF_MAX_ISIZE];
    InfLdsTabs tabs;
    u32 crc_tab[256];
};

// Loads of values this wavefront stored moments before (the match source): relaxed atomics of wavefront scope, the house
// idiom of k_chain_common.h -- no hardware fence, but the compiler may not reuse or reorder them across our stores.
template <class T> __device__ __forceinline__ T ld_wave(const T *p) { return __hip_atomic_load(const_cast<T *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
template <class T> __device__ __forceinline__ void st_wave(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

// the part of the decoder's environment (inflate_core.h) that every one-wavefront kernel shares (k_gzip.h too)
struct InfDevTabs {
    u32 lane, nl;
    InfCode *lt, *dt, *ct;
    u8 *lens;
    __device__ InfDevTabs(InfLdsTabs &t, u32 lane_) : lane(lane_), nl(64), lt(&t.lt), dt(&t.dt), ct(&t.ct), lens(t.lens) {}
    __device__ void sync() { __syncthreads(); }
};

struct InfDevEnv : InfDevTabs {
    static constexpr int full = INF_E_OUTPUT;
    u8 *out;
    u32 pos, cap;
    __device__ InfDevEnv(InfLds &S, u32 lane_, u32 cap_) : InfDevTabs(S.tabs, lane_), out(S.out), pos(0), cap(cap_) {}
    __device__ u32 reach() const { return pos; }             // a distance may not reach before the block's first byte
    __device__ void lit(u8 b) { if (lane == 0) st_wave(out + pos, b); ++pos; }
    __device__ void copy(u32 dist, u32 len) {
        for (u32 c = 0; c < len; c += 64) {                   // len <= 258: at most 5 steps
            const u32 j = c + lane;
            if (j < len) st_wave(out + pos + j, ld_wave(out + pos - dist + (j < dist ? j : j % dist)));
        }
        pos += len;
    }
    __device__ void stored(const u8 *src, u32 n) {
        for (u32 j = lane; j < n; j += 64) st_wave(out + pos + j, src[j]);
        pos += n;
    }
};

__global__ __launch_bounds__(64) void k_inflate(const u8 *__restrict__ in, const InfBlk *__restrict__ blk, u32 n_blk,
                                                u8 *__restrict__ out, u32 *__restrict__ status) {
    __shared__ InfLds S;
    const u32 b = blockIdx.x, lane = threadIdx.x;
    if (b >= n_blk) return;
    inf_crc_table(S.crc_tab, lane, 64);
    const InfBlk B = blk[b];
    InfDevEnv e(S, lane, B.isize <= INF_MAX_ISIZE ? B.isize : INF_MAX_ISIZE);     // (the host scan guarantees <=)
    __syncthreads();
    int rc = inf_raw(e, in + B.c_off, 0, B.d_len);              // block-relative: bit offsets stay far below 2^32
    if (B.isize > INF_MAX_ISIZE) rc = INF_E_OUTPUT;
    __syncthreads();
    if (!rc) {
        u32 c = inf_crc_stripe(S.crc_tab, S.out, e.cap, lane, 64);
        for (int m = 32; m; m >>= 1) c ^= (u32)__shfl_xor((int)c, m);
        if (c != B.crc) rc = INF_E_CRC;
    }
    if (!rc) {
        u8 *dst = out + B.o_off;
        const u32 n = e.cap;
        u32 head = (4u - (B.o_off & 3u)) & 3u;                 // bytes up to the first 4-byte aligned output address
        if (head > n) head = n;
        if (lane < head) dst[lane] = S.out[lane];
        const u32 nw = (n - head) >> 2;
        for (u32 w = lane; w < nw; w += 64) {
            const u8 *s = S.out + head + 4 * w;
            reinterpret_cast<u32 *>(dst + head)[w] = (u32)s[0] | (u32)s[1] << 8 | (u32)s[2] << 16 | (u32)s[3] << 24;
        }
        for (u32 j = head + 4 * nw + lane; j < n; j += 64) dst[j] = S.out[j];
    }
    if (lane == 0) status[b] = (u32)rc;
}
