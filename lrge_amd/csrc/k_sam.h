// k_sam.h -- unaligned SAM records found on the device in text that is resident in HBM; the rules are those
// of sam_core.h, which the host twin (sam_twin.cpp) runs too.  The line table comes from k_fx_census / k_fx_scatter in their
// FASTQ form (k_fastx.h), the identifiers and the bases leave through k_fx_names and k_fx_gather; what is here is in between:
//   k_sam_mark      one lane per line: 1 for a record line, 0 for an empty or '@' line          12 B read, 4 B written per line
//   (k_prims.h's exclusive scan of the marks ranks the records and counts them)
//   k_sam_records   one wavefront per record line: the line in steps of SAM_STEP bytes up to its tenth tab, the tabs ranked by
//                   a wave scan of the lanes' popcounts; then one lane applies sam_record and writes the record (FxRec, 32 B),
//                   its lengths and the verdict bits.  Quality strings and tags are never read.
// Lines that carry no record are skipped by their mark, not compacted away: a SAM file has a few header lines and a record line
// for every read, so a list of the record lines would cost 4 B per line to build and save nothing.
#pragma once
#include "k_fastx.h"
#include "sam_core.h"

#define SAM_THREADS 256
#define SAM_WAVES (SAM_THREADS / 64)

__global__ __launch_bounds__(SAM_THREADS) void k_sam_mark(const u8 *__restrict__ t, u64 n, const u64 *__restrict__ ls, u64 n_lf, u64 n_lines, u32 *__restrict__ mark) {
    const u64 j = (u64)blockIdx.x * SAM_THREADS + threadIdx.x;
    if (j >= n_lines) return;
    u64 a, e;
    fx_line(t, n, ls, n_lf, j, &a, &e);
    mark[j] = (u32)sam_is_record_line(t, a, e);
}

// rank: the exclusive scan of mark.  flags[0]: the verdict bits of all records; name_total: the identifiers' bytes
__global__ __launch_bounds__(SAM_THREADS) void k_sam_records(const u8 *__restrict__ t, u64 n, const u64 *__restrict__ ls, u64 n_lf, u64 n_lines,
                                                             const u32 *__restrict__ mark, const u32 *__restrict__ rank, FxRec *__restrict__ recs,
                                                             u32 *__restrict__ seq_len, u32 *__restrict__ name_len, u32 *__restrict__ flags,
                                                             unsigned long long *__restrict__ name_total) {
    const u32 lane = lane_id();
    const u64 n_waves = (u64)gridDim.x * SAM_WAVES;
    u32 f = 0;                                              // (lane 0 carries the wavefront's verdict bits and identifier bytes)
    u64 nb = 0;
    for (u64 j = (u64)blockIdx.x * SAM_WAVES + (threadIdx.x >> 6); j < n_lines; j += n_waves) {
        if (!mark[j]) continue;
        u64 a, e;
        fx_line(t, n, ls, n_lf, j, &a, &e);
        u64 t1 = 0, t2 = 0, t9 = 0, t10 = 0;
        u32 seen = 0;                                       // tabs in front of this step
        for (u64 p0 = a & ~(u64)15; p0 < e && seen < 10; p0 += SAM_STEP) {
            const u64 p = p0 + (u64)lane * 16;
            u32 m = 0;
            if (p < e) {                                    // (e <= n: the group lies inside the text and its FX_PAD)
                const uint4 q = *reinterpret_cast<const uint4 *>(t + p);
                m = sam_tab_mask(q.x, q.y, q.z, q.w, p, a, e);
            }
            if (!__ballot(m != 0)) continue;                // a step inside the sequence: no tab in 1 KiB
            const u32 cnt = (u32)__popc(m), inc = wave_incl_scan_u32(cnt), excl = seen + inc - cnt;
#pragma unroll
            for (u32 s = 0; s < SAM_N_TABS; ++s) {
                const u32 k = sam_tab_rank(s);
                const bool mine = excl < k && k <= excl + cnt;
                const u64 who = __ballot(mine);
                if (!who) continue;
                const u64 pos = __shfl(mine ? p + sam_nth_bit(m, k - excl - 1) : (u64)0, __ffsll((unsigned long long)who) - 1, 64);
                if (s == 0) t1 = pos; else if (s == 1) t2 = pos; else if (s == 2) t9 = pos; else t10 = pos;
            }
            seen += (u32)__shfl((int)inc, 63, 64);
        }
        if (lane == 0) {
            FxRec rec = {0, 0, 0, 0, 0};
            const u32 v = seen < 10 ? FX_UNPROVEN : sam_record(t, a, t1, t2, t9, t10, &rec);
            if (v) { rec.name_len = 0; rec.seq_len = 0; rec.seq_span = 0; }
            const u32 r = rank[j];
            recs[r] = rec;
            seq_len[r] = rec.seq_len; name_len[r] = rec.name_len;
            f |= v; nb += rec.name_len;
        }
    }
    if (lane == 0) {
        if (f) atomicOr(flags, f);
        if (nb) atomicAdd(name_total, (unsigned long long)nb);
    }
}
