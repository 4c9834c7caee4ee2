// k_cram.h -- the base blocks of an unaligned CRAM file decoded on the device (the steps are rans_core.h, the
// stream heads, the rounds and the launches cram_round.h):
//   k_rans_decode    one wavefront per block of the round: stored bytes copied, rANS 4x8 / rANS Nx16 entropy-decoded with the
//                    states in lanes 0..N-1, then the RLE and PACK expansions in the same wavefront.  The model (alphabet and
//                    cumulative frequencies) lives in LDS when it fits the launch's LDS, else its frequencies are read from global
//                    memory.  The output lands at the block's precomputed offset; one status word per block comes back.
// No workgroup waits for another: a block never needs another block's bytes.
#pragma once
#include "internal.h"
#include "k_prims.h"
#include "rans_core.h"

struct RansDevEnv {
    static constexpr uint32_t NV = 1;
    u32 lane;
    __device__ u32 lane0() const { return lane; }
    __device__ u32 lane1() const { return lane + 1; }
    __device__ void sync() { __threadfence_block(); __syncthreads(); }
    __device__ u64 ballot(const bool *f) const { return __ballot(f[0]); }
    // the exclusive scan of one value a lane; returns the wavefront's sum
    __device__ u64 excl_scan(const u64 *v, u64 *at) const {
        u64 x = v[0];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 lo = __shfl_up((u32)x, d, 64), hi = __shfl_up((u32)(x >> 32), d, 64);
            if ((int)lane >= d) x += (u64)hi << 32 | lo;
        }
        at[0] = x - v[0];
        return (u64)(u32)__shfl((int)(u32)x, 63, 64) | (u64)(u32)__shfl((int)(u32)(x >> 32), 63, 64) << 32;
    }
};

// lds_words: the 16-bit words of dynamic LDS this launch was given (at most RANS_LDS_U16)
__global__ __launch_bounds__(64) void k_rans_decode(const u8 *__restrict__ in, const RansBlk *__restrict__ blks, u32 m, const uint16_t *__restrict__ tabs,
                                                    const u8 *__restrict__ aux, const u32 *__restrict__ runs, u32 lds_words, u8 *tmp, u8 *out, u32 *__restrict__ status) {
    extern __shared__ uint16_t rans_lds[];
    const u32 a = blockIdx.x;
    if (a >= m) return;
    RansDevEnv e{threadIdx.x};
    const RansBlk b = blks[a];
    const u32 st = rans_block(e, in, b, tabs, aux, runs, rans_lds, lds_words, tmp, out);
    if (threadIdx.x == 0) status[a] = st;
}
