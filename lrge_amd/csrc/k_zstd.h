// k_zstd.h -- Zstandard blocks decoded in parallel on the device (the rules and the sequential form of every
// step are zs_core.h, the walk, the rounds and the scan zs_round.h):
//   k_zs_heads       one lane per compressed block: literals header, Number_of_Sequences, modes, where every description ends
//   k_zs_literals    one wavefront per compressed block: the Huffman table in LDS, the four streams on four lanes
//   k_zs_sequences   one wavefront per compressed block: three FSE tables in LDS (a lane each), the backward stream on one lane,
//                    the block's output size and its repeat-offset transfer function
//   k_zs_execute     one wavefront per block, all blocks of the round at once: literal runs and matches in 64-byte steps; a source
//                    in front of the block is not read, the byte's origin is recorded instead
//   k_zs_resolve     one workgroup per frame of the round: its blocks in order, a barrier between them; deferred bytes read final ones
//   k_zs_xxh64       one wavefront per frame: four lanes hold the four accumulators
//   k_zs_xxh64_part  the same for a frame that spans rounds of the sliding driver: one wavefront per part, the accumulators from
//                    and to a state in device memory
//   k_zs_slide       the history to the front of the work text, source and destination overlapping: one workgroup, chunk by chunk
// No workgroup waits for another: every dependency is a kernel boundary or a barrier inside one workgroup.
#pragma once
#include "zs_core.h"
#include "zs_round.h"

#define ZS_RESOLVE_THREADS 1024

struct ZsDevEnv {
    ZsTabs *t;
    u32 lane;
    u8 tb[1];
    u32 to[1];
    __device__ u32 lane0() const { return lane; }
    __device__ u32 lane1() const { return lane + 1; }
    __device__ u32 slot(u32) const { return 0; }
    __device__ void sync() { __syncthreads(); }
};

// `in` is readable (zeros) for ZS_PAD bytes behind its n bytes; every block lies inside the n bytes (zs_walk)
__global__ __launch_bounds__(64) void k_zs_heads(const u8 *__restrict__ in, const ZsBlock *__restrict__ blocks, u32 k, ZsHead *__restrict__ heads) {
    const u32 j = blockIdx.x * 64 + threadIdx.x;
    if (j >= k) return;
    const ZsBlock &B = blocks[j];
    if (B.type != 2) return;
    ZsHead h;
    zs_block_head(in + B.src, B.size, B.bmax, h);
    heads[j] = h;
}

__global__ __launch_bounds__(64) void k_zs_literals(const u8 *__restrict__ in, u64 n, const ZsBlock *__restrict__ blocks, u32 k, u8 *__restrict__ lit, u32 *__restrict__ status) {
    __shared__ ZsTabs T;
    const u32 j = blockIdx.x;
    if (j >= k || blocks[j].type != 2) return;
    ZsDevEnv e{&T, threadIdx.x, {0}, {0}};
    const u32 st = zs_literals(e, in, n, blocks[j], lit + blocks[j].lit_off);
    if (threadIdx.x == 0) status[j] = st;
}

__global__ __launch_bounds__(64) void k_zs_sequences(const u8 *__restrict__ in, u64 n, const ZsBlock *__restrict__ blocks, u32 k, ZsSeq *__restrict__ seq,
                                                     ZsSeqRes *__restrict__ res) {
    __shared__ ZsTabs T;
    const u32 j = blockIdx.x;
    if (j >= k || blocks[j].type != 2) return;
    ZsDevEnv e{&T, threadIdx.x, {0}, {0}};
    ZsSeqRes r;
    zs_sequences(e, in, n, blocks[j], seq + blocks[j].seq_off, r);
    // (a table that failed is seen by every lane; the stream's own result is lane 0's)
    if (threadIdx.x == 0) res[j] = r;
}

// block j's bytes at text + blocks[j].out, their origins at org + (blocks[j].out - base): base is where the round's text starts
__global__ __launch_bounds__(64) void k_zs_execute(const u8 *__restrict__ in, const ZsBlock *__restrict__ blocks, u32 k, const u8 *__restrict__ lit,
                                                   const ZsSeq *__restrict__ seq, u8 *text, u32 *org, u64 base, u32 *__restrict__ status) {
    const u32 j = blockIdx.x;
    if (j >= k) return;
    ZsDevEnv e{nullptr, threadIdx.x, {0}, {0}};
    const u32 st = zs_execute(e, in, blocks[j], lit + blocks[j].lit_off, seq + blocks[j].seq_off, text, org + (blocks[j].out - base));
    if (threadIdx.x == 0) status[j] = st;
}

// group g: blocks [group[g], group[g + 1]) belong to one frame
__global__ __launch_bounds__(ZS_RESOLVE_THREADS) void k_zs_resolve(const ZsBlock *__restrict__ blocks, const u32 *__restrict__ group, u8 *text, const u32 *__restrict__ org,
                                                                   u64 base) {
    const u32 g = blockIdx.x;
    for (u32 j = group[g]; j < group[g + 1]; ++j) {
        zs_resolve_block(text, org + (blocks[j].out - base), blocks[j].out, blocks[j].out_size, threadIdx.x, threadIdx.x + 1, ZS_RESOLVE_THREADS);
        __syncthreads();           // (a workgroup-scope fence too: the next block's reads see these bytes)
    }
}

// frame f of the launch: text[span[2 f], span[2 f] + span[2 f + 1])
__global__ __launch_bounds__(64) void k_zs_xxh64(const u8 *__restrict__ text, const u64 *__restrict__ span, u64 *__restrict__ out) {
    __shared__ ZsTabs T;
    ZsDevEnv e{&T, threadIdx.x, {0}, {0}};
    const u64 h = zs_xxh64(e, text + span[2 * blockIdx.x], span[2 * blockIdx.x + 1]);
    if (threadIdx.x == 0) out[blockIdx.x] = h;
}

// part f of the launch: text[job[f].at, + job[f].len) into state[job[f].slot & 1] (zs_xxh64_part); two parts of one launch are of
// two frames and name two states
__global__ __launch_bounds__(64) void k_zs_xxh64_part(const u8 *__restrict__ text, const ZsXxhJob *__restrict__ job, ZsXxh *state, u64 *__restrict__ out) {
    __shared__ ZsTabs T;
    ZsDevEnv e{&T, threadIdx.x, {0}, {0}};
    const ZsXxhJob J = job[blockIdx.x];
    const u64 h = zs_xxh64_part(e, state[J.slot & 1], text + J.at, J.len, (J.flags & 1) != 0, (J.flags & 2) != 0);
    if (threadIdx.x == 0) out[blockIdx.x] = h;
}

// text[from, from + n) to text[0, n), from > 0, the two overlapping when from < n.  One workgroup walks the bytes upwards in chunks
// of ZS_SLIDE_THREADS * ZS_SLIDE_PER: every thread reads its bytes of a chunk, the barrier, then writes them.  A chunk's writes end
// below the next chunk's reads (from > 0), and a thread has read a chunk before it passes that chunk's barrier, so no byte is
// overwritten before it is read
#define ZS_SLIDE_THREADS 1024
#define ZS_SLIDE_PER 16
__global__ __launch_bounds__(ZS_SLIDE_THREADS) void k_zs_slide(u8 *text, u64 from, u64 n) {
    for (u64 c = 0; c < n; c += (u64)ZS_SLIDE_THREADS * ZS_SLIDE_PER) {
        u8 v[ZS_SLIDE_PER];
        for (u32 k = 0; k < ZS_SLIDE_PER; ++k) { const u64 i = c + (u64)k * ZS_SLIDE_THREADS + threadIdx.x; v[k] = i < n ? text[from + i] : (u8)0; }
        __syncthreads();
        for (u32 k = 0; k < ZS_SLIDE_PER; ++k) { const u64 i = c + (u64)k * ZS_SLIDE_THREADS + threadIdx.x; if (i < n) text[i] = v[k]; }
    }
}
