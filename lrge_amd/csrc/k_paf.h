// k_paf.h -- overlaps.paf written on the device: the length step and the write step over paf_core.h.
// Between them the host runs scan_exclusive_u32 (k_prims.h) over one slice of line lengths.
#pragma once
#include "internal.h"
#include "k_prims.h"
#include "paf_core.h"

static_assert(sizeof(lrge_hip_chain) == PAF_REC_DWORDS * 4, "paf_core.h reads a chain record as 12 dwords");

// what both kernels read besides the records: per-read lengths and name offset tables of both sets, per-query statistics
struct PafIn {
    const u32 *rec;                     // [n][12]
    const u32 *q_len, *t_len;           // the sets' own device arrays
    const u64 *q_name_off, *t_name_off; // [nq + 1], [nt + 1] into the name blobs
    const u8 *q_names, *t_names;
    const i32 *rl; const u64 *sum_span; const u32 *n_kept;      // [nq]
};
struct PafTotals { unsigned long long bytes; u32 unproven; u32 pad; };

#define PAF_MEASURE_THREADS 256

// One lane per chain: the dv code, its proof, and the line's length.  The wavefront's unproven chains and its bytes reach the
// totals through one atomic each per wavefront.
__global__ void __launch_bounds__(PAF_MEASURE_THREADS) k_paf_measure(PafIn in, u64 n, u32 *__restrict__ code_out, u32 *__restrict__ len_out, PafTotals *tot) {
    const u64 i = (u64)blockIdx.x * PAF_MEASURE_THREADS + threadIdx.x;
    u32 len = 0, bad = 0;
    if (i < n) {
        const uint4 *rp = reinterpret_cast<const uint4 *>(in.rec + i * PAF_REC_DWORDS);      // (48-byte records in a 256-byte aligned block)
        const uint4 a = rp[0], b = rp[1], c = rp[2];
        const u32 rec[PAF_REC_DWORDS] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
        const u32 q = rec[PAF_R_QUERY], t = rec[PAF_R_TARGET];
        const u32 qlen = in.q_len[q], tlen = in.t_len[t];
        const PafEst est = paf_est((i32)rec[PAF_R_CNT], (i32)rec[PAF_R_NSEEDS], (i32)rec[PAF_R_QS], (i32)rec[PAF_R_RS], (i32)rec[PAF_R_RE], qlen, tlen,
                                   in.sum_span[q], in.n_kept[q]);
        u32 code; int unproven;
        PAF_CHAIN_DV(est, pow, code, unproven);
        bad = (u32)unproven;
        len = (u32)(in.q_name_off[q + 1] - in.q_name_off[q]) + (u32)(in.t_name_off[t + 1] - in.t_name_off[t]) + paf_fixed_width(rec, qlen, tlen, code, in.rl[q]);
        code_out[i] = code;
        len_out[i] = len;
    }
    const u64 bal = __ballot(bad != 0);
    u64 bytes = len;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) bytes += __shfl_down(bytes, d, 64);
    if (lane_id() == 0) {
        if (bal) atomicAdd(&tot->unproven, (u32)__popcll(bal));
        if (bytes) atomicAdd(&tot->bytes, (unsigned long long)bytes);
    }
}

#define PAF_WRITE_WAVES 4
#define PAF_ROW_BYTES 192      // one wavefront's LDS row: the fixed part (PAF_FIXED_BOUND), padded to a multiple of 64
static_assert(PAF_ROW_BYTES >= PAF_FIXED_BOUND && PAF_ROW_BYTES % 64 == 0, "the LDS row holds the fixed part");

// 64 lanes copy [src, src + n) to [dst, dst + n), 64 bytes a step; nothing is stored at or behind `end`
__device__ __forceinline__ void paf_wave_copy(u8 *__restrict__ dst, const u8 *__restrict__ src, u32 n, const u8 *end) {
    for (u32 j = lane_id(); j < n; j += 64)
        if (dst + j < end) dst[j] = src[j];
}

// One wavefront per line of the slice [i0, i0 + m): lanes 0..14 format one field each, a wave prefix sum of the widths places them
// in the wavefront's LDS row, and all 64 lanes copy out qname, the fields in front of tname, tname, and the rest.
// off[0..m]: the slice's exclusive scan of the line lengths (off[m] = its bytes); out: the slice's text.  A lane stores only inside
// [off[i], off[i + 1]).
__global__ void __launch_bounds__(PAF_WRITE_WAVES * 64) k_paf_write(PafIn in, u64 i0, u32 m, const u32 *__restrict__ code, const u32 *__restrict__ off, u8 *__restrict__ out) {
    __shared__ u8 rows[PAF_WRITE_WAVES][PAF_ROW_BYTES];
    const u32 lane = lane_id(), wv = threadIdx.x >> 6;
    const u32 li = blockIdx.x * PAF_WRITE_WAVES + wv;      // line of the slice (wavefront-uniform)
    if (li >= m) return;
    const u64 i = i0 + li;
    u8 *row = rows[wv];
    const u32 mine = lane < PAF_REC_DWORDS ? in.rec[i * PAF_REC_DWORDS + lane] : 0u;      // the record: one dword a lane
    const u32 q = __shfl(mine, PAF_R_QUERY, 64), t = __shfl(mine, PAF_R_TARGET, 64);
    const u32 f = lane;
    const u32 d = paf_field_rec_dword(f < PAF_N_FIELDS ? f : PAF_F_MAPQ);
    u32 v = __shfl(mine, d < PAF_REC_DWORDS ? d : 0u, 64);
    if (f == PAF_F_QLEN) v = in.q_len[q];
    else if (f == PAF_F_TLEN) v = in.t_len[t];
    else if (f == PAF_F_DV) v = code[i];
    else if (f == PAF_F_RL) v = (u32)in.rl[q];
    PafText tx; tx.lo = 0; tx.hi = 0; tx.n = 0;
    const u32 w = f < PAF_N_FIELDS ? paf_field(f, v, tx) : 0u;
    const u32 incl = wave_incl_scan_u32(w);
    const u32 pos = incl - w;
    if (f < PAF_N_FIELDS)
        for (u32 j = 0; j < w; ++j)
            if (pos + j < PAF_ROW_BYTES) row[pos + j] = paf_field_byte(f, tx, j);
    const u32 len_a = __shfl(pos, PAF_F_TLEN, 64);             // the fields between the names
    const u32 len_f = __shfl(incl, PAF_N_FIELDS - 1, 64);      // the whole fixed part
    const u64 qa = in.q_name_off[q], ta = in.t_name_off[t];
    const u32 qnl = (u32)(in.q_name_off[q + 1] - qa), tnl = (u32)(in.t_name_off[t + 1] - ta);
    u8 *dst = out + off[li];
    const u8 *end = out + off[li + 1];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // (the row is written and read by this wavefront only)
    __builtin_amdgcn_wave_barrier();
    paf_wave_copy(dst, in.q_names + qa, qnl, end);
    paf_wave_copy(dst + qnl, row, len_a, end);
    paf_wave_copy(dst + qnl + len_a, in.t_names + ta, tnl, end);
    paf_wave_copy(dst + qnl + len_a + tnl, row + len_a, len_f - len_a, end);
}
