// k_bam.h -- unaligned BAM records found on the device in text that is resident in HBM; the rules are those
// of bam_core.h, which the host twin (bam_twin.cpp) runs too.
//
// The records form a length-prefixed chain, so the work per record is one dependent load: the path is bound by memory latency,
// not by bandwidth.  The records area is cut into segments that are walked side by side, each from a start of its own, and the
// host ties the walks together (bam_chain_plan).
//   k_bam_header   one lane: the header walk -> {verdict, hdr_end}
//   k_bam_find     one wavefront per segment: 64 consecutive offsets a step through bam_plausible, the first hit by ballot
//   k_bam_walk     one lane per listed segment: the chain from the given start to the segment's end -> {start, count, landing};
//                  the first round (every segment, from its candidate) and the repair rounds (a list, from landing[s - 1])
//   k_bam_records  one lane per segment, behind the exclusive scan of the counts: the walk again from the proven start, writing
//                  FxRec, seq_len, name_len; verdict bits and identifier bytes as k_fx_records leaves them (k_fx_names follows)
//   k_bam_gather   one wavefront per selected read: packed 4-bit codes -> ASCII in aligned words, 8 bases per lane and step
//   k_bam_spans, k_bam_store   windowed ingest: the packed bytes of a window's records into the base store
//   k_bam_keep     sampled ingest: identifier and packed bytes of a window's chosen records, by k_bam_store's body
// A walker takes the 24 bytes of a record's fixed fields and nothing else of it; lanes of one wavefront walk different segments,
// and a short list is spread over the workgroups (walker i is lane i / gridDim.x of workgroup i % gridDim.x), so that few
// segments still use many CUs.  The text buffer has FX_PAD bytes behind its end (k_fastx.h): the gather's word behind an
// unaligned source word may lie there; bam_record itself reads no byte at or past n.
#pragma once
#include "internal.h"
#include "k_prims.h"
#include "bam_core.h"

struct BamHeader { u64 hdr_end; u32 verdict, pad; };

__global__ __launch_bounds__(64) void k_bam_header(const u8 *__restrict__ t, u64 n, BamHeader *__restrict__ out) {
    if (threadIdx.x || blockIdx.x) return;
    BamHeader h = {0, 0, 0};
    uint64_t e = 0;
    h.verdict = bam_header(t, n, &e);
    h.hdr_end = e;
    *out = h;
}

// cand[s]: the first plausible record start in segment s > 0, or BAM_NONE; cand[0] = hdr_end, the one start that is known
__global__ __launch_bounds__(64) void k_bam_find(const u8 *__restrict__ t, u64 n, u64 hdr_end, u64 S, u64 *__restrict__ cand) {
    const u64 s = blockIdx.x;
    const u32 lane = threadIdx.x;
    if (s == 0) { if (lane == 0) cand[0] = hdr_end; return; }
    const u64 end = bam_seg_end(hdr_end, S, n, s);
    u64 hit = BAM_NONE;
    for (u64 p = bam_seg_begin(hdr_end, S, s); p < end; p += 64) {
        const u64 off = p + lane;
        const u64 b = __ballot(off < end && bam_plausible(t, n, off));
        if (b) { hit = p + (u64)(__ffsll((unsigned long long)b) - 1); break; }
    }
    if (lane == 0) cand[s] = hit;
}

// walker i: segment list[i] from from[i], or (list == nullptr) segment i from cand[i]; out[i] is its summary
__global__ __launch_bounds__(64) void k_bam_walk(const u8 *__restrict__ t, u64 n, u64 hdr_end, u64 S, const u32 *__restrict__ list, const u64 *__restrict__ from,
                                                 const u64 *__restrict__ cand, u64 n_list, u32 tail, BamSeg *__restrict__ out) {
    const u64 i = (u64)blockIdx.x + (u64)gridDim.x * threadIdx.x;
    if (i >= n_list) return;
    const u64 s = list ? list[i] : i;
    out[i] = bam_walk(t, n, list ? from[i] : cand[i], bam_seg_end(hdr_end, S, n, s), tail != 0);
}

// start[s]: the proven start of segment s (BAM_NONE: a record spans it); base[s], base[s + 1]: its slice of the table.
// cut: where the proven chain ends (n, or the incomplete record start a window's last segment stops at).
// flags[0]: the verdict bits of all records; name_total: the identifiers' bytes
__global__ __launch_bounds__(64) void k_bam_records(const u8 *__restrict__ t, u64 n, u64 hdr_end, u64 S, const u64 *__restrict__ start, const u64 *__restrict__ base,
                                                    u64 n_seg, u64 cut, FxRec *__restrict__ recs, u32 *__restrict__ seq_len, u32 *__restrict__ name_len,
                                                    u32 *__restrict__ flags, unsigned long long *__restrict__ name_total) {
    const u64 s = (u64)blockIdx.x + (u64)gridDim.x * threadIdx.x;
    u32 f = 0;
    u64 nl = 0;
    if (s < n_seg && start[s] != BAM_NONE) {
        const u64 b = base[s];
        uint64_t nb = 0;
        const u64 end = bam_seg_end(hdr_end, S, n, s);
        f = bam_walk_records(t, n, start[s], end < cut ? end : cut, base[s + 1] - b, recs + b, seq_len + b, name_len + b, &nb);
        nl = nb;
    }
    for (int d = 32; d > 0; d >>= 1) { f |= __shfl_down(f, d, 64); nl += __shfl_down(nl, d, 64); }
    if (lane_id() == 0) {
        if (f) atomicOr(flags, f);
        if (nl) atomicAdd(name_total, (unsigned long long)nl);
    }
}

// Read j of the selection (record idx[j]) to dense[boff[j], boff[j + 1]): seq_len bases from seq_span packed bytes.  Bytes up
// to the first aligned word of the destination and behind the last whole group of eight go one base a lane; in between a lane
// takes the source word its eight bases start in and the one behind it (bam_window) and stores two aligned words.  An odd length
// leaves the last low nibble unread.
__global__ __launch_bounds__(64) void k_bam_gather(const u8 *__restrict__ t, const FxRec *__restrict__ recs, const u32 *__restrict__ idx, const u64 *__restrict__ boff,
                                                   u32 n_sel, u8 *__restrict__ dense) {
    const u32 lane = threadIdx.x;
    for (u32 j = blockIdx.x; j < n_sel; j += gridDim.x) {
        const FxRec rec = recs[idx[j]];
        const u8 *s = t + rec.seq_off;
        u8 *d = dense + boff[j];
        const u64 len = rec.seq_len;
        u64 head = (4 - ((uintptr_t)d & 3)) & 3;
        if (head > len) head = len;
        if (lane < head) d[lane] = (u8)bam_base(s, lane);
        const u64 ng = (len - head) >> 3;
        u32 *dw = reinterpret_cast<u32 *>(d + head);
        for (u64 g = lane; g < ng; g += 64) {
            u32 w[2];
            bam_group8(s, head + 8 * g, w);
            dw[2 * g] = w[0]; dw[2 * g + 1] = w[1];
        }
        const u64 i = head + 8 * ng + lane;
        if (i < len) d[i] = (u8)bam_base(s, i);
    }
}

// ---- windowed ingest: the packed bases of a window's records into the base store (fx_window.h) ----
// span[r] = (seq_len[r] + 1) / 2: the bytes record r takes in the store; their exclusive scan is k_bam_store's dst
__global__ __launch_bounds__(256) void k_bam_spans(const u32 *__restrict__ seq_len, u64 n_rec, u32 *__restrict__ span) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r < n_rec) span[r] = (u32)(((u64)seq_len[r] + 1) >> 1);
}

// The copy body of k_bam_store and k_bam_keep, one wavefront: `len` bytes from s to d.
// A plain byte copy between two buffers whose alignments differ: single bytes up to the first 16-byte boundary of the
// destination, then 16 bytes per lane and step -- five aligned source words funnel-shifted into four (four when source and
// destination agree modulo 4, which is uniform over the record) and one 16-byte store, so a wavefront moves 1 KiB a step and a
// HiFi record of 5-10 KB is a handful of steps -- then single bytes behind the last whole group.  The word behind an
// unaligned source word may lie up to 3 bytes behind the record: inside the block, or in the FX_PAD bytes behind it.
__device__ __forceinline__ void bam_copy_packed(const u8 *__restrict__ s, u8 *__restrict__ d, u64 len, u32 lane) {
    u64 head = (16 - ((uintptr_t)d & 15)) & 15;
    if (head > len) head = len;
    if (lane < head) d[lane] = s[lane];
    const u64 ng = (len - head) >> 4;
    const u32 mis = (u32)((uintptr_t)(s + head) & 3), sh = mis * 8;
    const u32 *q0 = reinterpret_cast<const u32 *>(s + head - mis);        // (pointer arithmetic: the loads stay global)
    uint4 *dq = reinterpret_cast<uint4 *>(d + head);
    if (sh == 0) {
        for (u64 g = lane; g < ng; g += 64) {
            const u32 *q = q0 + 4 * g;
            dq[g] = make_uint4(q[0], q[1], q[2], q[3]);
        }
    } else {
        for (u64 g = lane; g < ng; g += 64) {
            const u32 *q = q0 + 4 * g;
            const u32 a = q[0], b = q[1], c = q[2], e = q[3], f = q[4];
            dq[g] = make_uint4((a >> sh) | (b << (32 - sh)), (b >> sh) | (c << (32 - sh)), (c >> sh) | (e << (32 - sh)), (e >> sh) | (f << (32 - sh)));
        }
    }
    const u64 i = head + 16 * ng + lane;
    if (i < len) d[i] = s[i];
}

// Record r's seq_span packed bytes to store[dst[r], dst[r] + seq_span), one wavefront per record, grid-strided; every record
// starts on a byte and the pad nibble of an odd length is copied as it is, so k_bam_gather reads the store as it reads the
// text.  The copy is bam_copy_packed.
// No LDS, no scratch; the launch is k_fx_store's (a wavefront per workgroup, 32 workgroups a CU: 8 a SIMD, full occupancy
// for a copy whose only cost is the latency of its loads).
__global__ __launch_bounds__(64) void k_bam_store(const u8 *__restrict__ t, const FxRec *__restrict__ recs, const u32 *__restrict__ dst, u64 n_rec, u8 *__restrict__ store) {
    const u32 lane = threadIdx.x;
    for (u64 r = blockIdx.x; r < n_rec; r += gridDim.x) bam_copy_packed(t + recs[r].seq_off, store + dst[r], recs[r].seq_span, lane);
}

// ---- sampled ingest (fx_window.h FX_KEEP_SEL) ----
// Chosen record j of the window (sel[j] - r0 in its table), one wavefront each, grid-strided: its identifier's name_len bytes as they
// are (NULs kept; `*` has length 0 already) to names[name_dst[j], ..), its seq_span packed bytes to store[dst[j], ..) by
// bam_copy_packed.  dst: the exclusive scan of the chosen spans (k_fx_pick, k_bam_spans), name_dst: that of the chosen identifier
// lengths; `store` and `names` point behind what the earlier windows kept.  No LDS, no scratch; the launch is k_fx_keep's.
__global__ __launch_bounds__(64) void k_bam_keep(const u8 *__restrict__ t, const FxRec *__restrict__ recs, const u32 *__restrict__ sel, u32 r0, u64 n_sel,
                                                 const u32 *__restrict__ dst, const u32 *__restrict__ name_dst, u8 *__restrict__ store, u8 *__restrict__ names) {
    const u32 lane = threadIdx.x;
    for (u64 j = blockIdx.x; j < n_sel; j += gridDim.x) {
        const FxRec rec = recs[sel[j] - r0];
        const u8 *s = t + rec.name_off;
        u8 *d = names + name_dst[j];
        for (u32 i = lane; i < rec.name_len; i += 64) d[i] = s[i];
        bam_copy_packed(t + rec.seq_off, store + dst[j], rec.seq_span, lane);
    }
}
