// pair_owner.h -- which rank counts the (query, name) pairs of a query in lrge_hip_overlap_twoset_tsharded.
//
// THE RULE (stated here once; lrge_amd/parallel.py: pair_owner_bounds restates it for the tests): rank r of `world` owns the
// queries [floor(r * nq / world), floor((r + 1) * nq / world)) -- contiguous ranges in rank order that tile [0, nq).  The product
// is taken in 64 bits: nq < 2^32 and r <= world <= TS_MAX_WORLD, so it cannot wrap.
#pragma once

__host__ __device__ inline unsigned long long pair_owner_first(unsigned long long r, unsigned long long nq, unsigned long long world) {
    return r * nq / world;      // first query of rank r; r == world gives nq
}
