// k_fastx.h -- FASTA / FASTQ records found on the device in text that is resident in HBM; the rules are
// those of fastx_core.h, which the host twin (fastx_twin.cpp) runs too.
//
// A lane takes one 16-byte load of the text and forms three 16-bit masks from it (fx_group_masks): line feeds, removed bytes,
// FASTA headers.  A 256-lane workgroup covers a tile of FX_TILE = 4096 bytes.
//   k_fx_census    text -> per-tile counts of the three masks                      1 B read per text byte
//   k_fx_summary   one workgroup: totals, the first and last byte that is not removed, the bytes the host decides the format by
//   (k_prims.h's exclusive scan turns the counts into offsets)
//   k_fx_scatter   text -> FASTQ: the start of every line (8 B per line); FASTA: offset of every header and the removed bytes
//                  in front of it (12 B per record)                                1 B read per text byte
//   k_fx_records   one lane per record: the record table (FxRec, 32 B), lengths, verdict bits
//   k_fx_names     identifiers compacted into one dense buffer
//   k_fx_gather    one wavefront per selected read: its bases into one dense ASCII buffer, removed bytes dropped
//   k_fx_store     windowed ingest: one wavefront per record of a window, its bases into the base store   (same copy)
//   k_fx_bases     selected ingest: the sum of a window's sequence lengths           4 B read per record
//   k_fx_pick      one lane per chosen record of a window: its two lengths into dense arrays
//   k_fx_keep      one wavefront per chosen record: its identifier into the identifier buffer, its bases into the store   (same copy)
//   k_fx_seek      seek map: one lane per record of a window, the first record start of every cell   32 B read per record
//   k_fx_runs      mapped open: the trimmed runs from the decode staging to the tail of the block, a wavefront per 4 KiB tile
// The text buffer is allocated with FX_PAD bytes behind its end, so whole 16-byte groups (and the word behind an unaligned
// source word of the gather) may be loaded; every byte at or past `n` is masked out before use.
#pragma once
#include "internal.h"
#include "k_prims.h"
#include "fastx_core.h"
#include "fx_seek.h"

#define FX_THREADS 256
#define FX_PAD 64u
static_assert(FX_THREADS * 16 == FX_TILE, "a lane per 16-byte group");

// what k_fx_summary leaves for the host (FxCensus and the two tile numbers it came from)
struct FxSummary { u64 n_lf, n_rem, n_hdr, first, last; u32 head, at_first, tail, pad; };

// the masks of the group at p (a multiple of 16; p < n)
__device__ __forceinline__ FxMasks fx_load_masks(const u8 *__restrict__ t, u64 n, u64 p) {
    const uint4 q = *reinterpret_cast<const uint4 *>(t + p);
    const u32 prev = p ? t[p - 1] : '\n', next = p + 16 < n ? t[p + 16] : FX_EOT;
    return fx_group_masks(q.x, q.y, q.z, q.w, prev, next, (u32)(n - p < 16 ? n - p : 16));
}
__device__ __forceinline__ u32 fx_valid_mask(u64 n, u64 p) { return n - p < 16 ? (1u << (u32)(n - p)) - 1 : 0xFFFFu; }

// exclusive scan of one value per lane over the workgroup (FX_THREADS lanes); ws: FX_THREADS / 64 words of LDS
__device__ __forceinline__ u32 fx_block_excl(u32 v, u32 *ws) {
    const u32 inc = wave_incl_scan_u32(v);
    __syncthreads();                                        // (ws may still be read from the previous use)
    if (lane_id() == 63) ws[threadIdx.x >> 6] = inc;
    __syncthreads();
    u32 off = inc - v;
    for (u32 w = 0; w < (threadIdx.x >> 6); ++w) off += ws[w];
    return off;
}

__global__ __launch_bounds__(FX_THREADS) void k_fx_census(const u8 *__restrict__ t, u64 n, u32 *__restrict__ c_lf, u32 *__restrict__ c_rem,
                                                          u32 *__restrict__ c_hdr) {
    __shared__ u32 ws[3][FX_THREADS / 64];
    const u64 p = (u64)blockIdx.x * FX_TILE + (u64)threadIdx.x * 16;
    u32 a = 0, b = 0, c = 0;
    if (p < n) {
        const FxMasks m = fx_load_masks(t, n, p);
        a = (u32)__popc(m.lf); b = (u32)__popc(m.rem); c = (u32)__popc(m.hdr);
    }
    for (int d = 32; d > 0; d >>= 1) { a += __shfl_down(a, d, 64); b += __shfl_down(b, d, 64); c += __shfl_down(c, d, 64); }
    if (lane_id() == 0) { ws[0][threadIdx.x >> 6] = a; ws[1][threadIdx.x >> 6] = b; ws[2][threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x < 3) {
        u32 s = 0;
        for (int w = 0; w < FX_THREADS / 64; ++w) s += ws[threadIdx.x][w];
        (threadIdx.x == 0 ? c_lf : threadIdx.x == 1 ? c_rem : c_hdr)[blockIdx.x] = s;
    }
}

// one workgroup of FX_THREADS lanes over the tile counts (12 B per 4096 text bytes)
__global__ __launch_bounds__(FX_THREADS) void k_fx_summary(const u8 *__restrict__ t, u64 n, const u32 *__restrict__ c_lf, const u32 *__restrict__ c_rem,
                                                           const u32 *__restrict__ c_hdr, u64 n_tiles, FxSummary *__restrict__ out) {
    __shared__ u64 s_sum[3][FX_THREADS / 64];
    __shared__ u64 s_tile[2][FX_THREADS / 64];
    __shared__ u32 s_pos[2];
    u64 a = 0, b = 0, c = 0, tf = n_tiles, tl = 0;          // tl: 1 + the last tile with a byte that stays
    for (u64 k = threadIdx.x; k < n_tiles; k += FX_THREADS) {
        const u32 rem = c_rem[k];
        a += c_lf[k]; b += rem; c += c_hdr[k];
        const u64 bytes = n - k * FX_TILE < FX_TILE ? n - k * FX_TILE : FX_TILE;
        if (rem < bytes) { if (tf == n_tiles) tf = k; tl = k + 1; }
    }
    for (int d = 32; d > 0; d >>= 1) {
        a += __shfl_down(a, d, 64); b += __shfl_down(b, d, 64); c += __shfl_down(c, d, 64);
        const u64 of = __shfl_down(tf, d, 64), ol = __shfl_down(tl, d, 64);
        tf = of < tf ? of : tf; tl = ol > tl ? ol : tl;
    }
    if (lane_id() == 0) {
        const u32 w = threadIdx.x >> 6;
        s_sum[0][w] = a; s_sum[1][w] = b; s_sum[2][w] = c; s_tile[0][w] = tf; s_tile[1][w] = tl;
    }
    if (threadIdx.x == 0) { s_pos[0] = 0xFFFFFFFFu; s_pos[1] = 0; }
    __syncthreads();
    a = b = c = 0; tf = n_tiles; tl = 0;
    for (int w = 0; w < FX_THREADS / 64; ++w) {
        a += s_sum[0][w]; b += s_sum[1][w]; c += s_sum[2][w];
        tf = s_tile[0][w] < tf ? s_tile[0][w] : tf; tl = s_tile[1][w] > tl ? s_tile[1][w] : tl;
    }
    // the exact positions inside those two tiles: a lane per group, as everywhere
    if (tf < n_tiles) {
        for (int side = 0; side < 2; ++side) {
            const u64 p = (side ? tl - 1 : tf) * FX_TILE + (u64)threadIdx.x * 16;
            if (p >= n) continue;
            const u32 keep = ~fx_load_masks(t, n, p).rem & fx_valid_mask(n, p);
            if (!keep) continue;
            if (!side) atomicMin(&s_pos[0], threadIdx.x * 16 + (u32)__ffs(keep) - 1);
            else atomicMax(&s_pos[1], threadIdx.x * 16 + 31 - (u32)__clz(keep));
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        FxSummary s;
        s.n_lf = a; s.n_rem = b; s.n_hdr = c;
        s.first = tf < n_tiles ? tf * FX_TILE + s_pos[0] : n;
        s.last = tf < n_tiles ? (tl - 1) * FX_TILE + s_pos[1] : n;
        s.head = 0;
        for (u32 i = 0; i < 4 && i < n; ++i) s.head |= (u32)t[i] << (8 * i);
        s.at_first = s.first < n ? t[s.first] : 0;
        s.tail = n ? t[n - 1] : 0;
        s.pad = 0;
        *out = s;
    }
}

// FASTQ (fmt == FX_FMT_FASTQ): ls[k + 1] = 1 + the offset of line feed k, and the line numbers of the bytes at `first` and
// `last` into lines[0..1].  FASTA: hpos / hrem of every header.  o_*: the exclusive scans of the census.
__global__ __launch_bounds__(FX_THREADS) void k_fx_scatter(const u8 *__restrict__ t, u64 n, int fmt, const u32 *__restrict__ o_lf, const u32 *__restrict__ o_rem,
                                                           const u32 *__restrict__ o_hdr, u64 first, u64 last, u64 *__restrict__ ls, u64 *__restrict__ lines,
                                                           u64 *__restrict__ hpos, u32 *__restrict__ hrem) {
    __shared__ u32 ws[FX_THREADS / 64];
    const u64 p = (u64)blockIdx.x * FX_TILE + (u64)threadIdx.x * 16;
    FxMasks m = {0, 0, 0};
    if (p < n) m = fx_load_masks(t, n, p);
    if (fmt == FX_FMT_FASTQ) {
        u64 r = (u64)o_lf[blockIdx.x] + fx_block_excl((u32)__popc(m.lf), ws);
        if (p == 0 && threadIdx.x == 0) ls[0] = 0;
        if (first >= p && first < p + 16) lines[0] = r + (u32)__popc(m.lf & ((1u << (u32)(first - p)) - 1));
        if (last >= p && last < p + 16) lines[1] = r + (u32)__popc(m.lf & ((1u << (u32)(last - p)) - 1));
        for (u32 b = m.lf; b; b &= b - 1) ls[++r] = p + (u32)__ffs(b);            // (__ffs is 1-based: the byte behind the line feed)
    } else {
        u64 r = (u64)o_hdr[blockIdx.x] + fx_block_excl((u32)__popc(m.hdr), ws);
        const u32 rem = o_rem[blockIdx.x] + fx_block_excl((u32)__popc(m.rem), ws);
        for (u32 b = m.hdr; b; b &= b - 1, ++r) {
            const u32 i = (u32)__ffs(b) - 1;
            hpos[r] = p + i;
            hrem[r] = rem + (u32)__popc(m.rem & ((1u << i) - 1));
        }
    }
}

// flags[0]: the verdict bits of all records; name_total: the identifiers' bytes
__global__ __launch_bounds__(FX_THREADS) void k_fx_records(const u8 *__restrict__ t, u64 n, int fmt, u64 n_rec, const u64 *__restrict__ ls, u64 n_lf, u64 n_lines,
                                                           u64 l0, const u64 *__restrict__ hpos, const u32 *__restrict__ hrem, u64 n_rem, FxRec *__restrict__ recs,
                                                           u32 *__restrict__ seq_len, u32 *__restrict__ name_len, u32 *__restrict__ flags,
                                                           unsigned long long *__restrict__ name_total) {
    const u64 r = (u64)blockIdx.x * FX_THREADS + threadIdx.x;
    u32 f = 0;
    u64 nl = 0;
    if (r < n_rec) {
        FxRec rec = {0, 0, 0, 0, 0};
        f = fmt == FX_FMT_FASTQ ? fx_fastq_record(t, n, ls, n_lf, n_lines, l0, r, &rec) : fx_fasta_record(t, n, hpos, hrem, n_rec, n_rem, r, &rec);
        if (f) { rec.name_len = 0; rec.seq_len = 0; rec.seq_span = 0; }
        recs[r] = rec;
        seq_len[r] = rec.seq_len; name_len[r] = rec.name_len;
        nl = rec.name_len;
    }
    for (int d = 32; d > 0; d >>= 1) { f |= __shfl_down(f, d, 64); nl += __shfl_down(nl, d, 64); }
    if (lane_id() == 0) {
        if (f) atomicOr(flags, f);
        if (nl) atomicAdd(name_total, (unsigned long long)nl);
    }
}

// name_dst: the exclusive scan of name_len
__global__ __launch_bounds__(FX_THREADS) void k_fx_names(const u8 *__restrict__ t, const FxRec *__restrict__ recs, const u32 *__restrict__ name_dst, u64 n_rec,
                                                         u8 *__restrict__ names) {
    const u64 r = (u64)blockIdx.x * FX_THREADS + threadIdx.x;
    if (r >= n_rec) return;
    const u8 *s = t + recs[r].name_off;
    u8 *d = names + name_dst[r];
    const u32 k = recs[r].name_len;
    for (u32 i = 0; i < k; ++i) d[i] = s[i];
}

// s[0, len) to d[0, len) by one wavefront (`lane` of 64), for every alignment of either: aligned 4-byte words of the destination, each
// assembled from the two source words it overlaps (the word behind the last source byte may be loaded: FX_PAD), bytes at both ends
__device__ __forceinline__ void fx_copy_span(const u8 *__restrict__ s, u8 *__restrict__ d, u64 len, u32 lane) {
    u64 head = (4 - ((uintptr_t)d & 3)) & 3;
    if (head > len) head = len;
    if (lane < head) d[lane] = s[lane];
    const u64 nw = (len - head) >> 2;
    for (u64 w = lane; w < nw; w += 64) {
        const uintptr_t sa = (uintptr_t)(s + head + 4 * w);
        const u32 sh = (u32)(sa & 3) * 8;
        const u32 *q = reinterpret_cast<const u32 *>(sa & ~(uintptr_t)3);
        const u32 lo = q[0];
        reinterpret_cast<u32 *>(d + head)[w] = sh ? (u32)((((u64)q[1] << 32) | lo) >> sh) : lo;
    }
    for (u64 i = head + 4 * nw + lane; i < len; i += 64) d[i] = s[i];
}

// The bases of one record to d[0, seq_len), by one wavefront (`lane` of 64).  A single-line sequence (span == length) is copied
// by fx_copy_span; a multi-line one is compacted group by
// group with a wave scan of the kept bytes.
__device__ __forceinline__ void fx_copy_bases(const u8 *__restrict__ t, u64 n, const FxRec &rec, u8 *__restrict__ d, u32 lane) {
    const u64 a = rec.seq_off, len = rec.seq_len;
    if (rec.seq_span == len) {
        fx_copy_span(t + a, d, len, lane);
    } else {
        const u64 b = a + rec.seq_span;
        u64 done = 0;
        for (u64 p0 = a & ~(u64)15; p0 < b; p0 += 64 * 16) {
            const u64 p = p0 + (u64)lane * 16;
            u32 keep = 0;
            uint4 q = {0, 0, 0, 0};
            if (p < b && p < n) {
                q = *reinterpret_cast<const uint4 *>(t + p);
                const u32 next = p + 16 < n ? t[p + 16] : FX_EOT;
                keep = ~fx_group_masks(q.x, q.y, q.z, q.w, '\n', next, (u32)(n - p < 16 ? n - p : 16)).rem & fx_valid_mask(n, p);
                if (p < a) keep &= ~((1u << (u32)(a - p)) - 1);
                if (b - p < 16) keep &= (1u << (u32)(b - p)) - 1;
            }
            const u32 cnt = (u32)__popc(keep), inc = wave_incl_scan_u32(cnt);
            u64 o = done + inc - cnt;
            const u32 w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (u32 i = 0; i < 16; ++i)
                if ((keep >> i) & 1) d[o++] = (u8)(w[i >> 2] >> ((i & 3) * 8));
            done += (u32)__shfl((int)inc, 63, 64);
        }
    }
}

// Read j of the selection (record idx[j]) to dense[boff[j], boff[j + 1]).
__global__ __launch_bounds__(64) void k_fx_gather(const u8 *__restrict__ t, u64 n, const FxRec *__restrict__ recs, const u32 *__restrict__ idx,
                                                  const u64 *__restrict__ boff, u32 n_sel, u8 *__restrict__ dense) {
    for (u32 j = blockIdx.x; j < n_sel; j += gridDim.x) fx_copy_bases(t, n, recs[idx[j]], dense + boff[j], threadIdx.x);
}

// Windowed ingest (fx_window.h): every record of a window's prefix to store[dst[r], dst[r] + seq_len), all of
// them in file order.  dst: the exclusive scan of the window's seq_len; `store` points behind the bases of the earlier windows.
__global__ __launch_bounds__(64) void k_fx_store(const u8 *__restrict__ t, u64 n, const FxRec *__restrict__ recs, const u32 *__restrict__ dst, u64 n_rec,
                                                 u8 *__restrict__ store) {
    for (u64 r = blockIdx.x; r < n_rec; r += gridDim.x) fx_copy_bases(t, n, recs[r], store + dst[r], threadIdx.x);
}

// Selected ingest (fx_window.h FX_KEEP_NONE / FX_KEEP_SEL).  The sum of a window's seq_len, added to *total: the
// bases the pass has seen.  Grid stride, one atomic a wavefront; *total comes back with the verdict words of k_fx_records.
__global__ __launch_bounds__(FX_THREADS) void k_fx_bases(const u32 *__restrict__ seq_len, u64 n_rec, unsigned long long *__restrict__ total) {
    u64 s = 0;
    for (u64 r = (u64)blockIdx.x * FX_THREADS + threadIdx.x; r < n_rec; r += (u64)gridDim.x * FX_THREADS) s += seq_len[r];
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
    if (lane_id() == 0 && s) atomicAdd(total, (unsigned long long)s);
}

// The chosen records of a window, one lane each: sel[0, n_sel) is the window's slice of the selection (fx_sel_slice: file
// ordinals, ascending), r0 the ordinal of the window's first record.  Their lengths go to dense arrays of n_sel entries, the inputs
// of the two scans that place them and of the copies to the host.
__global__ __launch_bounds__(FX_THREADS) void k_fx_pick(const u32 *__restrict__ sel, u32 r0, u64 n_sel, const u32 *__restrict__ seq_len, const u32 *__restrict__ name_len,
                                                        u32 *__restrict__ pick_seq, u32 *__restrict__ pick_name) {
    const u64 j = (u64)blockIdx.x * FX_THREADS + threadIdx.x;
    if (j >= n_sel) return;
    const u32 r = sel[j] - r0;
    pick_seq[j] = seq_len[r]; pick_name[j] = name_len[r];
}

// Chosen record j of the window, one wavefront each: its identifier to names[name_dst[j], ..), its bases to store[dst[j], ..) by the
// copy body of k_fx_gather and k_fx_store.  dst / name_dst: the exclusive scans of k_fx_pick's arrays; `store` and `names` point
// behind what the earlier windows kept.
__global__ __launch_bounds__(64) void k_fx_keep(const u8 *__restrict__ t, u64 n, const FxRec *__restrict__ recs, const u32 *__restrict__ sel, u32 r0, u64 n_sel,
                                                const u32 *__restrict__ dst, const u32 *__restrict__ name_dst, u8 *__restrict__ store, u8 *__restrict__ names) {
    for (u64 j = blockIdx.x; j < n_sel; j += gridDim.x) {
        const FxRec rec = recs[sel[j] - r0];
        const u8 *s = t + rec.name_off;
        u8 *d = names + name_dst[j];
        for (u32 i = threadIdx.x; i < rec.name_len; i += 64) d[i] = s[i];
        fx_copy_bases(t, n, rec, store + dst[j], threadIdx.x);
    }
}

// The seek map of a census (fx_seek.h), behind k_fx_records or k_bam_records: one lane per record of the window's
// proven prefix.  Record r starts at window offset fx_rec_start(recs[r].name_off, lead) -- the '>' or '@' of its header line (lead 1),
// the block_size field of a BAM record (lead 36) --, which is text offset `through` + that.
// A record whose cell (text offset / stride) differs from its predecessor's is the first that starts in its cell: its index goes
// to slot[cell - cell0] and its window offset to slot[n_cells + cell - cell0] (preset to FX_SEEK_NONE); record 0 always writes.
// cell0: the cell of the window's first byte; every record lies in [cell0, cell0 + n_cells).
__global__ __launch_bounds__(FX_THREADS) void k_fx_seek(const FxRec *__restrict__ recs, u64 n_rec, u64 through, u64 stride, u64 cell0, u64 n_cells, u32 lead,
                                                        u32 *__restrict__ slot) {
    const u64 r = (u64)blockIdx.x * FX_THREADS + threadIdx.x;
    if (r >= n_rec) return;
    const u64 at = fx_rec_start(recs[r].name_off, lead), cell = (through + at) / stride;
    if (r && (through + fx_rec_start(recs[r - 1].name_off, lead)) / stride == cell) return;
    const u64 c = cell - cell0;
    if (c >= n_cells) return;                               // (never: the prefix ends inside the last cell)
    slot[c] = (u32)r; slot[n_cells + c] = (u32)at;
}

// The mapped open: copy j of the table is src[c.src, c.src + c.len) to dst[c.dst, ..), the trimmed part of a run
// in the decode staging to its place behind the block's tail.  The copies are cut into tiles of FX_RUN_TILE bytes; first[j] is
// the number of tiles in front of copy j (first[n_copy]: all of them), made by the host, and a wavefront takes a tile: it finds
// its copy by bisection and moves the tile with fx_copy_span, whatever the alignment of either side.
#define FX_RUN_TILE 4096u
struct FxRunCopy { u64 src, dst, len; };
__global__ __launch_bounds__(64) void k_fx_runs(const u8 *__restrict__ src, u8 *__restrict__ dst, const FxRunCopy *__restrict__ copies, const u64 *__restrict__ first,
                                                u32 n_copy) {
    const u64 tile = blockIdx.x;                            // (the grid is first[n_copy] wavefronts: a window is below 2^32 bytes, its tiles below 2^21)
    if (tile >= first[n_copy]) return;
    u32 lo = 0, hi = n_copy;                                // the last copy whose first tile is at or below `tile`
    while (hi - lo > 1) { const u32 mid = lo + (hi - lo) / 2; if (first[mid] <= tile) lo = mid; else hi = mid; }
    const FxRunCopy c = copies[lo];
    const u64 off = (tile - first[lo]) * FX_RUN_TILE, m = c.len - off < FX_RUN_TILE ? c.len - off : FX_RUN_TILE;
    fx_copy_span(src + c.src + off, dst + c.dst + off, m, threadIdx.x);
}
