// k_bzip2.h -- bzip2 blocks decoded in parallel on the device (the rules and the sequential form of every
// step are bz_core.h, the rounds and the chain bz_round.h):
//   k_bz_find        every bit offset of the compressed bytes against the two 48-bit magics, 16 bytes per lane
//   k_bz_decode      one wavefront per candidate: header, tables in LDS, Huffman + move-to-front + runs into the BWT column L
//   k_bz_scatter     one wavefront per accepted block: the stable counting scatter of L into the links tt (4 B per byte)
//   k_bz_walk        one lane per block: n dependent loads through tt (latency-bound: the blocks of a round are its parallelism)
//   k_bz_rle_count   one lane per block: the length of the block's text behind the run-length layer
//   k_bz_rle_write   one lane per block: the text at its place in the round's output, with the block's CRC
// A census that leaves a seek map runs k_bz_walk_rec and k_bz_rle_write_rec in their place: the same bodies with the
// recording mark sink (bz_core.h BzMarkRec), BZ_MARKS marks a block.  The mapped open enters a block at those marks:
//   k_bz_marks_text  one wavefront per block, lane j from mark j: its segment of the walk fed straight through the run-length layer
//                    and the CRC into the text (bz_segment_lane); the bytes in front of the run-length layer are never stored
#pragma once
#include "bz_core.h"
#include "bz_round.h"

#define BZ_FIND_THREADS 256

// `in` is 16-byte aligned and readable (zeros) for BZ_PAD bytes behind its n bytes.  A candidate is 8 * byte + shift, with
// BZ_END_FLAG for the end-of-stream magic; at most `cap` are written (in any order: the host sorts them), *count counts them all.
__global__ __launch_bounds__(BZ_FIND_THREADS) void k_bz_find(const u8 *__restrict__ in, u64 n, u64 *__restrict__ cand, u32 cap, u32 *__restrict__ count) {
    const u64 v = (u64)blockIdx.x * BZ_FIND_THREADS + threadIdx.x;   // this lane's 16 bytes
    if (v * 16 >= n) return;
    const uint4 a = ((const uint4 *)in)[v], b = ((const uint4 *)in)[v + 1];
    // bytes [16 v, 16 v + 24) as big-endian words
    const u32 W[6] = {__builtin_bswap32(a.x), __builtin_bswap32(a.y), __builtin_bswap32(a.z), __builtin_bswap32(a.w), __builtin_bswap32(b.x), __builtin_bswap32(b.y)};
#pragma unroll
    for (u32 j = 0; j < 16; ++j) {
        const u64 hi = (u64)W[j >> 2] << 32 | W[(j >> 2) + 1];
        const u32 sh = 8 * (j & 3);
        const u64 w = sh ? hi << sh | W[(j >> 2) + 2] >> (32 - sh) : hi;   // bytes [16 v + j, 16 v + j + 8)
#pragma unroll
        for (u32 s = 0; s < 8; ++s) {
            const u32 kind = bz_magic_in(w, s);
            const u64 bit = 8 * (16 * v + j) + s;
            if (kind && bit + 48 <= 8 * n) {
                const u32 at = atomicAdd(count, 1u);
                if (at < cap) cand[at] = bit | (kind == 2 ? BZ_END_FLAG : 0);
            }
        }
    }
}

struct BzDevEnv {
    static constexpr u32 PER = 4;             // 256 list entries over 64 lanes
    BzTabs *t;
    u32 lane, nl;
    __device__ void sync() { __syncthreads(); }
};

// candidate c: from bit pos[c] into slot c of L (bs bytes) and cnt (256 counts)
__global__ __launch_bounds__(64) void k_bz_decode(const u8 *__restrict__ in, u64 n, const u64 *__restrict__ pos, u32 k, u32 bs, u8 *__restrict__ L,
                                                  u32 *__restrict__ cnt, BzRes *__restrict__ res) {
    __shared__ BzTabs T;
    const u32 c = blockIdx.x, lane = threadIdx.x;
    if (c >= k) return;
    BzDevEnv e{&T, lane, 64};
    BzRes r;
    bz_decode_block(e, in, n, pos[c], bs, L + (u64)c * bs, r);
    if (r.status == BZ_OK) for (u32 i = lane; i < 256; i += 64) cnt[(u64)c * 256 + i] = T.cnt[i];
    if (lane == 0) res[c] = r;
}

// link a: tt[j] = i << 8 | c for the j-th byte of the sorted column (bz_scatter), 64 bytes of L per step, ranks inside a step from
// the lanes that hold the same byte
__global__ __launch_bounds__(64) void k_bz_scatter(const BzLink *__restrict__ links, u32 m, u32 bs, const u8 *__restrict__ L, const u32 *__restrict__ cnt,
                                                   u32 *__restrict__ tt) {
    __shared__ u32 cf[256];
    const u32 a = blockIdx.x, lane = threadIdx.x;
    if (a >= m) return;
    const BzLink K = links[a];
    const u8 *Lc = L + (u64)K.slot * bs;
    const u32 *c = cnt + (u64)K.slot * 256;
    u32 *t = tt + K.tt_off;
    {
        const u32 v0 = c[4 * lane], v1 = c[4 * lane + 1], v2 = c[4 * lane + 2], v3 = c[4 * lane + 3];
        const u32 s = v0 + v1 + v2 + v3, ex = wave_incl_scan_u32(s) - s;
        cf[4 * lane] = ex; cf[4 * lane + 1] = ex + v0; cf[4 * lane + 2] = ex + v0 + v1; cf[4 * lane + 3] = ex + v0 + v1 + v2;
    }
    __syncthreads();
    for (u32 i0 = 0; i0 < K.n; i0 += 64) {
        const u32 i = i0 + lane;
        const bool valid = i < K.n;
        const u32 d = valid ? Lc[i] : 0;
        u64 same = __ballot(valid);
#pragma unroll
        for (u32 bit = 0; bit < 8; ++bit) {
            const u64 set = __ballot((d >> bit) & 1);
            same &= ((d >> bit) & 1) ? set : ~set;
        }
        const u32 rank = (u32)__popcll(same & lanemask_lt()), total = (u32)__popcll(same);
        const u32 base = valid ? cf[d] : 0;
        __syncthreads();
        if (valid) {
            const u32 at = base + rank;
            if (at < K.n) t[at] = i << 8 | d;
            if (rank + 1 == total) cf[d] = base + total;
        }
        __syncthreads();
    }
}

// link a (one per lane): the walk of bz_walk, into the block's slot of L (the column is not needed any more)
__global__ __launch_bounds__(64) void k_bz_walk(const BzLink *__restrict__ links, u32 m, u32 bs, const u32 *__restrict__ tt, u8 *__restrict__ L, u32 *__restrict__ bad) {
    const u32 a = blockIdx.x * 64 + threadIdx.x;
    if (a >= m) return;
    const BzLink K = links[a];
    if (!bz_walk(tt + K.tt_off, K.n, K.orig, L + (u64)K.slot * bs)) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(64) void k_bz_rle_count(const BzLink *__restrict__ links, u32 m, u32 bs, const u8 *__restrict__ pre, u64 *__restrict__ len) {
    const u32 a = blockIdx.x * 64 + threadIdx.x;
    if (a >= m) return;
    const BzLink K = links[a];
    len[a] = bz_rle_len(pre + (u64)K.slot * bs, K.n);
}

__global__ __launch_bounds__(64) void k_bz_rle_write(const BzLink *__restrict__ links, u32 m, u32 bs, const u8 *__restrict__ pre, u8 *__restrict__ out,
                                                     u32 *__restrict__ crc) {
    __shared__ u32 tab[256];
    bz_crc_table(tab, threadIdx.x, 64);
    __syncthreads();
    const u32 a = blockIdx.x * 64 + threadIdx.x;
    if (a >= m) return;
    const BzLink K = links[a];
    crc[a] = bz_rle_write(pre + (u64)K.slot * bs, K.n, tab, out + K.out_off);
}

// ---- the recording forms: marks + a * BZ_MARKS are link a's (zeroed by the host: a block has bz_mark_count(n) of them) ----
__global__ __launch_bounds__(64) void k_bz_walk_rec(const BzLink *__restrict__ links, u32 m, u32 bs, const u32 *__restrict__ tt, u8 *__restrict__ L, u32 *__restrict__ bad,
                                                    BzMark *__restrict__ marks) {
    const u32 a = blockIdx.x * 64 + threadIdx.x;
    if (a >= m) return;
    const BzLink K = links[a];
    if (!bz_walk(tt + K.tt_off, K.n, K.orig, L + (u64)K.slot * bs, BzMarkRec(marks + (u64)a * BZ_MARKS, K.n))) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(64) void k_bz_rle_write_rec(const BzLink *__restrict__ links, u32 m, u32 bs, const u8 *__restrict__ pre, u8 *__restrict__ out,
                                                         u32 *__restrict__ crc, BzMark *__restrict__ marks) {
    __shared__ u32 tab[256];
    bz_crc_table(tab, threadIdx.x, 64);
    __syncthreads();
    const u32 a = blockIdx.x * 64 + threadIdx.x;
    if (a >= m) return;
    const BzLink K = links[a];
    crc[a] = bz_rle_write(pre + (u64)K.slot * bs, K.n, tab, out + K.out_off, BzMarkRec(marks + (u64)a * BZ_MARKS, K.n));
}

// ---- the seeded decode ----
// Block a of a mapped open's batch: its links tt + tt_off (k_bz_scatter's, n of them), its text out + out_off of `len` bytes, its marks
// marks + mark0 * BZ_MARKS; orig and crc are the map's (the host has compared the entropy decode's with them).  Lane j runs segment j
// (an idle lane where j * seg >= n) and compares where it arrives with mark j + 1; a lane that fails gives the block BZ_E_ENTRY.
// No lane loads tt at an index >= n or stores outside its own text range [mark j's offset, mark j + 1's), whatever the marks hold
struct BzMarkTask { u64 tt_off, out_off; u32 n, orig, crc, len, mark0, pad; };
__global__ __launch_bounds__(64) void k_bz_marks_text(const BzMarkTask *__restrict__ tasks, u32 m, const u32 *__restrict__ tt, const BzMark *__restrict__ marks,
                                                      u8 *__restrict__ out, u32 *__restrict__ status) {
    __shared__ u32 tab[256];
    __shared__ BzMark mk[BZ_MARKS];
    const u32 a = blockIdx.x, lane = threadIdx.x;
    if (a >= m) return;
    bz_crc_table(tab, lane, 64);
    const BzMarkTask K = tasks[a];
    mk[lane] = marks[(u64)K.mark0 * BZ_MARKS + lane];
    __syncthreads();
    const bool good = bz_segment_lane(tt + K.tt_off, K.n, K.orig, K.crc, K.len, mk, lane, tab, out + K.out_off);
    const bool all = __all(good);
    if (lane == 0) status[a] = all ? (u32)BZ_OK : (u32)BZ_E_ENTRY;
}
