// k_xz.h -- .xz blocks decoded in parallel on the device (the rules and the sequential form of both steps are
// xz_core.h, the walk, the rounds and the launches xz_round.h):
//   k_xz_decode      one wavefront per unfinished block of the round: the chunks the host gave it for this launch.  The model
//                    (28 268 bytes at most), the staged compressed bytes and the ring of recent output live in LDS; control is
//                    wavefront-uniform, the copies are 64 lanes wide; the decoder state goes back to the block's slot in HBM
//   k_xz_check       one wavefront per block that has a check: CRC32 or CRC64 over 64 stripes, combined by shifts
// No workgroup waits for another: a block never needs another block's text.
#pragma once
#include "xz_core.h"
#include "xz_round.h"

struct XzDevEnv {
    uint16_t *probs;
    u8 *stage, *ring;
    u64 *tab, *part;
    u32 lane;
    __device__ u32 lane0() const { return lane; }
    __device__ u32 lane1() const { return lane + 1; }
    __device__ void sync() { __syncthreads(); }
};

// `in`: the file; chunks: the call's chunk table; text: the round's text; slots: the round's state slots (XZ_SLOT_BYTES each)
__global__ __launch_bounds__(64) void k_xz_decode(const u8 *__restrict__ in, const XzChunk *__restrict__ chunks, const XzTask *__restrict__ tasks, u32 m, u8 *text,
                                                  u8 *slots, u32 *__restrict__ status, u32 *__restrict__ bad_chunk) {
    __shared__ uint16_t probs[XZ_PROBS_MAX];
    __shared__ u8 stage[XZ_STAGE];
    __shared__ u8 ring[XZ_RING];
    const u32 a = blockIdx.x;
    if (a >= m) return;
    XzDevEnv e{probs, stage, ring, nullptr, nullptr, threadIdx.x};
    u32 bad = 0;
    const u32 st = xz_decode(e, in, chunks, tasks[a], text, slots, &bad);
    if (threadIdx.x == 0) { status[a] = st; bad_chunk[a] = bad; }
}

__global__ __launch_bounds__(64) void k_xz_check(const u8 *__restrict__ text, const XzSpan *__restrict__ spans, u32 m, u64 *__restrict__ out) {
    __shared__ u64 tab[256];
    __shared__ u64 part[XZ_NL];
    const u32 a = blockIdx.x;
    if (a >= m) return;
    XzDevEnv e{nullptr, nullptr, nullptr, tab, part, threadIdx.x};
    const u64 c = xz_check(e, text + spans[a].at, spans[a].len, spans[a].wide != 0);
    if (threadIdx.x == 0) out[a] = c;
}
