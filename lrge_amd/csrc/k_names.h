// k_names.h -- the kernels of the identifier ranking by fixed LSD passes (rules: name_lsd.h, pass loop:
// name_lsd_round.h, host side: host_names.inl).  One thread per sorted position, 256 threads per workgroup; the sorts between
// them are radix_sort_pairs, the scan is scan_exclusive_u32 (k_prims.h).  Bandwidth-trivial at these sizes: the care is in the
// bounds.  Every index that comes out of device memory is checked against n before it is used (the host has checked off and len
// against the blob; a value that fails here raises a status bit and the call fails), and an identifier is cut at the blob's end,
// so no load leaves [blob, blob + padded size).
#pragma once
#include "internal.h"
#include "name_lsd.h"

#define NL_THREADS 256

struct NlArgs {
    const u64 *w8;      // the blob as aligned words
    u64 n_text;         // its identifier bytes (NL_PAD zero bytes and more follow)
    const u64 *off;     // [n]
    const u32 *len;     // [n]
    u32 n;
    u32 W;
    u32 *stat;          // [0]: distinct identifiers (the scan's total), [1]: status bits (NL_BAD_*)
};

__device__ __forceinline__ void nl_entry(const NlArgs &A, u64 e, u64 &o, u32 &l) {
    o = A.off[e]; l = A.len[e];
    if (o > A.n_text) { o = A.n_text; l = 0; }
    if ((u64)l > A.n_text - o) l = (u32)(A.n_text - o);
}

// key[p] = the key of pass `pass` (W: the length, w < W: word w) of entry val[p]; first: of entry p, and val[p] = p is written
__global__ __launch_bounds__(NL_THREADS) void k_nl_key(NlArgs A, u64 *val, u64 *key, u32 pass, u32 first) {
    const u64 p = (u64)blockIdx.x * NL_THREADS + threadIdx.x;
    if (p >= A.n) return;
    const u64 e = first ? p : val[p];
    if (e >= A.n) { atomicOr(A.stat + 1, NL_BAD_VAL); key[p] = 0; return; }
    if (first) val[p] = p;
    u64 o; u32 l;
    nl_entry(A, e, o, l);
    key[p] = nl_pass_key(A.w8, o, l, pass, A.W);
}

// flag[p] = 1 when sorted position p starts a run of equal identifiers
__global__ __launch_bounds__(NL_THREADS) void k_nl_heads(NlArgs A, const u64 *val, u32 *flag) {
    const u64 p = (u64)blockIdx.x * NL_THREADS + threadIdx.x;
    if (p >= A.n) return;
    if (p == 0) { flag[0] = 1; return; }
    const u64 a = val[p - 1], b = val[p];
    if (a >= A.n || b >= A.n) { atomicOr(A.stat + 1, NL_BAD_VAL); flag[p] = 1; return; }
    u64 oa, ob; u32 la, lb;
    nl_entry(A, a, oa, la);
    nl_entry(A, b, ob, lb);
    flag[p] = nl_equal(A.w8, oa, la, ob, lb, A.W) ? 0u : 1u;
}

// k_nl_rank, first half: a head writes the sorted position its run starts at
__global__ __launch_bounds__(NL_THREADS) void k_nl_starts(NlArgs A, const u32 *flag, const u32 *excl, u32 *start) {
    const u64 p = (u64)blockIdx.x * NL_THREADS + threadIdx.x;
    if (p >= A.n || !flag[p]) return;
    const u32 r = excl[p];
    if (r >= A.n) { atomicOr(A.stat + 1, NL_BAD_RUN); return; }
    start[r] = (u32)p;
}

// k_nl_rank, second half: every position writes the start of its run as the rank of its entry
__global__ __launch_bounds__(NL_THREADS) void k_nl_rank(NlArgs A, const u64 *val, const u32 *flag, const u32 *excl, const u32 *start, u32 *rank_out) {
    const u64 p = (u64)blockIdx.x * NL_THREADS + threadIdx.x;
    if (p >= A.n) return;
    const u32 r = nl_run_of(excl[p], flag[p]);
    const u64 e = val[p];
    if (r >= A.n) { atomicOr(A.stat + 1, NL_BAD_RUN); return; }
    if (e >= A.n) { atomicOr(A.stat + 1, NL_BAD_VAL); return; }
    rank_out[e] = start[r];
}
