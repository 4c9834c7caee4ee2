// host_bzip2.inl -- bzip2 decompressed on the device (k_bzip2.h): the backend that bz_round.h's bz_run drives and
// the C entry point.  Included into lrge_hip.hip behind host_gzip.inl (GzBuf).
//
// The compressed bytes go up once and stay for the call (they are a fraction of the text).  Option BZIP2_ROUND_BLOCKS: the
// candidates decoded per round; its default is what half of the arena's idle bytes plus the device's free bytes hold at
// bz_candidate_bytes per candidate, at most BZ_ROUND_MAX.  Option BZIP2_TIMING: the stages are separated by synchronisations and
// their times are printed to stderr when the call ends (tools/bzip2_bench.py).
//
// A census that leaves a seek map sets keep_marks: finish launches the recording forms of the walk and the
// run-length write, and the recorder of bz_round.h fetches the round's marks in one copy (marks_out).  Without it nothing else is
// launched, copied or reported.  The mapped open enters blocks at their marks through stage_up / seeded (fx_src_seek_bzip2).

#include "dev_keep.h"

static const char *bz_status_name(int s) {
    switch (s) {
    case BZ_E_MAGIC: return "no bzip2 stream header or block magic";
    case BZ_E_INPUT: return "unexpected end of compressed data";
    case BZ_E_RANDOMISED: return "a randomised block";
    case BZ_E_GROUPS: return "invalid number of coding tables, selectors or symbols";
    case BZ_E_SELECTOR: return "a selector out of range";
    case BZ_E_LENGTH: return "a code length out of range";
    case BZ_E_CODE: return "invalid code";
    case BZ_E_SIZE: return "a block above the level's block size";
    case BZ_E_NO_EOB: return "no end-of-block symbol";
    case BZ_E_ORIGPTR: return "origPtr outside the block";
    case BZ_E_BLOCK_CRC: return "block CRC mismatch";
    case BZ_E_STREAM_CRC: return "stream CRC mismatch";
    case BZ_E_TRAILING: return "bytes behind the end of the stream";
    case BZ_E_CHAIN: return "a block ends where no block starts";
    case BZ_E_RUN: return "a block stops behind four equal bytes";
    case BZ_E_ENTRY: return "a block does not arrive where its marks say";
    default: return "unknown status";
    }
}

namespace {
struct BzDev : DevKeep {
    GzBuf in, list, count, pos, res, L, cnt, links, tt, lens, crc, out, bad, marks, tasks;
    u64 n = 0;
    u32 bs = 0;
    bool timing = false, keep_marks = false;
    double ms[6] = {0, 0, 0, 0, 0, 0};                            // find, entropy, scatter, walk, run-length layer and CRC, the seeded decode (k_bz_marks_text)
    explicit BzDev(lrge_hip_ctx *c) : DevKeep(c) {
        for (GzBuf *b : {&in, &list, &count, &pos, &res, &L, &cnt, &links, &tt, &lens, &crc, &out, &bad, &marks, &tasks}) b->ctx = c;
        timing = c->opt("BZIP2_TIMING") != nullptr;
    }
    ~BzDev() { (void)hipStreamSynchronize(ctx->stream); }
    bool load(const uint8_t *d, uint64_t len) {
        n = len;
        const u64 body = len & ~(u64)15, size = ((len + 15) & ~(u64)15) + BZ_PAD;
        if (!in.need((size_t)size, &e)) return false;
        if (!ok(hipMemsetAsync(in.as<u8>() + body, 0, (size_t)(size - body), ctx->stream))) return false;
        if (!ok(hipMemcpyAsync(in.p, d, (size_t)len, hipMemcpyHostToDevice, ctx->stream))) return false;
        return sync();
    }
    bool find(std::vector<uint64_t> &c) {
        Lap lap(*this, ms[0], timing);
        // about one candidate per block is expected: a list that proves too short is sized by the count, and the scan runs once more
        u64 cap = n / 64 + 16;
        for (int pass = 0;; ++pass) {
            u32 found = 0;
            if (cap > 0xFFFFFFFFull) { e = hipErrorInvalidValue; return false; }
            if (!list.need((size_t)cap * 8, &e) || !count.need(4, &e)) return false;
            if (!ok(hipMemsetAsync(count.p, 0, 4, ctx->stream))) return false;
            hipLaunchKernelGGL(k_bz_find, dim3((u32)div_up(div_up(n, 16), BZ_FIND_THREADS)), dim3(BZ_FIND_THREADS), 0, ctx->stream, in.as<const u8>(), n, list.as<u64>(),
                               (u32)cap, count.as<u32>());
            if (!ok(hipGetLastError())) return false;
            if (!ok(hipMemcpyAsync(&found, count.p, 4, hipMemcpyDeviceToHost, ctx->stream)) || !sync()) return false;
            if (found > cap) {
                if (pass) { e = hipErrorUnknown; return false; }   // (the same bytes gave another count)
                cap = found;
                continue;
            }
            c.resize(found);
            if (found && (!ok(hipMemcpyAsync(c.data(), list.p, (size_t)found * 8, hipMemcpyDeviceToHost, ctx->stream)) || !sync())) return false;
            std::sort(c.begin(), c.end(), [](uint64_t a, uint64_t b) { return (a & ~BZ_END_FLAG) < (b & ~BZ_END_FLAG); });
            return lap.end();
        }
    }
    // (the text of a block is about its size again)
    uint32_t default_round(uint32_t block) { return (uint32_t)std::min<u64>(BZ_ROUND_MAX, std::max<u64>(1, dev_budget(ctx) / (bz_candidate_bytes(block) + block))); }
    bool decode(const uint64_t *p, uint32_t k, uint32_t block, BzRes *r) {
        Lap lap(*this, ms[1], timing);
        bs = block;
        if (!pos.need((size_t)k * 8, &e) || !res.need((size_t)k * sizeof(BzRes), &e) || !L.need((size_t)k * bs, &e) || !cnt.need((size_t)k * 1024, &e)) return false;
        if (!ok(hipMemcpyAsync(pos.p, p, (size_t)k * 8, hipMemcpyHostToDevice, ctx->stream))) return false;
        hipLaunchKernelGGL(k_bz_decode, dim3(k), dim3(64), 0, ctx->stream, in.as<const u8>(), n, pos.as<const u64>(), k, bs, L.as<u8>(), cnt.as<u32>(), res.as<BzRes>());
        if (!ok(hipGetLastError())) return false;
        if (!ok(hipMemcpyAsync(r, res.p, (size_t)k * sizeof(BzRes), hipMemcpyDeviceToHost, ctx->stream)) || !sync()) return false;
        return lap.end();
    }
    bool finish(BzLink *l, uint32_t m, uint32_t *crc_h, uint64_t *out_bytes, const uint8_t **bytes) {
        hipStream_t st = ctx->stream;
        u64 links_n = 0;
        for (uint32_t a = 0; a < m; ++a) { l[a].tt_off = links_n; links_n += l[a].n; }
        if (!links.need((size_t)m * sizeof(BzLink), &e) || !tt.need((size_t)links_n * 4, &e) || !lens.need((size_t)m * 8, &e) || !crc.need((size_t)m * 4, &e) ||
            !bad.need(4, &e))
            return false;
        if (!ok(hipMemcpyAsync(links.p, l, (size_t)m * sizeof(BzLink), hipMemcpyHostToDevice, st)) || !ok(hipMemsetAsync(bad.p, 0, 4, st))) return false;
        const u32 lane_blocks = (u32)div_up(m, 64);
        if (keep_marks && (!marks.need((size_t)m * BZ_MARKS * sizeof(BzMark), &e) || !ok(hipMemsetAsync(marks.p, 0, (size_t)m * BZ_MARKS * sizeof(BzMark), st)))) return false;
        {
            Lap lap(*this, ms[2], timing);
            hipLaunchKernelGGL(k_bz_scatter, dim3(m), dim3(64), 0, st, links.as<const BzLink>(), m, bs, L.as<const u8>(), cnt.as<const u32>(), tt.as<u32>());
            if (!ok(hipGetLastError()) || !lap.end()) return false;
        }
        {
            Lap lap(*this, ms[3], timing);
            if (keep_marks) hipLaunchKernelGGL(k_bz_walk_rec, dim3(lane_blocks), dim3(64), 0, st, links.as<const BzLink>(), m, bs, tt.as<const u32>(), L.as<u8>(), bad.as<u32>(), marks.as<BzMark>());
            else hipLaunchKernelGGL(k_bz_walk, dim3(lane_blocks), dim3(64), 0, st, links.as<const BzLink>(), m, bs, tt.as<const u32>(), L.as<u8>(), bad.as<u32>());
            if (!ok(hipGetLastError()) || !lap.end()) return false;
        }
        Lap lap(*this, ms[4], timing);
        hipLaunchKernelGGL(k_bz_rle_count, dim3(lane_blocks), dim3(64), 0, st, links.as<const BzLink>(), m, bs, L.as<const u8>(), lens.as<u64>());
        if (!ok(hipGetLastError())) return false;
        std::vector<u64> len_h(m);
        u32 bad_h = 0;
        if (!ok(hipMemcpyAsync(len_h.data(), lens.p, (size_t)m * 8, hipMemcpyDeviceToHost, st)) || !ok(hipMemcpyAsync(&bad_h, bad.p, 4, hipMemcpyDeviceToHost, st)) || !sync())
            return false;
        if (bad_h) { e = hipErrorUnknown; return false; }          // (a link left its block: the counts were not L's)
        u64 total = 0;
        for (uint32_t a = 0; a < m; ++a) { l[a].out_off = total; l[a].run_open = (len_h[a] & BZ_RUN_OPEN) != 0; total += len_h[a] & ~BZ_RUN_OPEN; }
        // the text: in a buffer of the round on its way to the host, or behind the earlier rounds' in the block that stays
        u8 *dst;
        if (to_host) { if (!out.need((size_t)total + 4, &e)) return false; dst = out.as<u8>(); }
        else { if (!keep_reserve(total)) return false; dst = keep + keep_len; }
        if (!ok(hipMemcpyAsync(links.p, l, (size_t)m * sizeof(BzLink), hipMemcpyHostToDevice, st))) return false;
        if (keep_marks) hipLaunchKernelGGL(k_bz_rle_write_rec, dim3(lane_blocks), dim3(64), 0, st, links.as<const BzLink>(), m, bs, L.as<const u8>(), dst, crc.as<u32>(), marks.as<BzMark>());
        else hipLaunchKernelGGL(k_bz_rle_write, dim3(lane_blocks), dim3(64), 0, st, links.as<const BzLink>(), m, bs, L.as<const u8>(), dst, crc.as<u32>());
        if (!ok(hipGetLastError())) return false;
        if (!ok(hipMemcpyAsync(crc_h, crc.p, (size_t)m * 4, hipMemcpyDeviceToHost, st))) return false;
        if (!lap.end()) return false;
        if (!to_host) keep_len += total;
        // (to the host, deliver has drained the stream; the block that stays is flushed before the CRCs are waited for)
        if (!(*bytes = deliver(dst, total)) || (!to_host && !sync())) return false;
        *out_bytes = total;
        return true;
    }
    // the marks finish left for its m links, BZ_MARKS a link, in one copy down (bz_round.h BzSeekRec)
    bool marks_out(BzMark *dst, uint32_t m) {
        return ok(hipMemcpyAsync(dst, marks.p, (size_t)m * BZ_MARKS * sizeof(BzMark), hipMemcpyDeviceToHost, ctx->stream)) && sync();
    }

    // ---- the mapped open (fx_src_seek_bzip2) ----
    // `total` staged bytes at host pointer h (pinned) in one copy up: comp_len bytes of file ranges back to back, zeros up to marks_at
    // (a multiple of 16, at least BZ_PAD of them), then the needed blocks' marks.  decode() then takes positions rebased to the ranges
    u64 marks_at = 0;
    bool stage_up(const u8 *h, u64 comp_len, u64 at, u64 total) {
        n = comp_len; marks_at = at;
        if (!in.need((size_t)total + 16, &e)) return false;
        return ok(hipMemcpyAsync(in.p, h, (size_t)total, hipMemcpyHostToDevice, ctx->stream));
    }
    // m blocks that decode() left in slots 0..m-1 (l: slot, n, orig; tt_off is filled here; t: the same blocks' tasks, tt_off filled
    // here too) entered at their marks: the scatter, then one wavefront a block writes its text to d_out + t[a].out_off.  status[a]: BZ_OK or BZ_E_ENTRY
    bool seeded(BzLink *l, BzMarkTask *t, uint32_t m, u8 *d_out, u32 *status) {
        hipStream_t st = ctx->stream;
        u64 links_n = 0;
        for (uint32_t a = 0; a < m; ++a) { l[a].tt_off = t[a].tt_off = links_n; links_n += l[a].n; }
        if (!links.need((size_t)m * sizeof(BzLink), &e) || !tasks.need((size_t)m * sizeof(BzMarkTask), &e) || !tt.need((size_t)links_n * 4, &e) || !crc.need((size_t)m * 4, &e)) return false;
        if (!ok(hipMemcpyAsync(links.p, l, (size_t)m * sizeof(BzLink), hipMemcpyHostToDevice, st)) || !ok(hipMemcpyAsync(tasks.p, t, (size_t)m * sizeof(BzMarkTask), hipMemcpyHostToDevice, st)))
            return false;
        {
            Lap lap(*this, ms[2], timing);
            hipLaunchKernelGGL(k_bz_scatter, dim3(m), dim3(64), 0, st, links.as<const BzLink>(), m, bs, L.as<const u8>(), cnt.as<const u32>(), tt.as<u32>());
            if (!ok(hipGetLastError()) || !lap.end()) return false;
        }
        Lap lap(*this, ms[5], timing);
        hipLaunchKernelGGL(k_bz_marks_text, dim3(m), dim3(64), 0, st, tasks.as<const BzMarkTask>(), m, tt.as<const u32>(), (const BzMark *)(in.as<const u8>() + marks_at), d_out, crc.as<u32>());
        if (!ok(hipGetLastError())) return false;
        if (!ok(hipMemcpyAsync(status, crc.p, (size_t)m * 4, hipMemcpyDeviceToHost, st)) || !sync()) return false;     // (links and tasks are pageable: their copies are done)
        return lap.end();
    }
    void print_timing() const {
        if (timing) fprintf(stderr, "[lrge_hip] bzip2 stages ms: find %.3f entropy %.3f scatter %.3f walk %.3f rle_crc %.3f marks_text %.3f\n", ms[0], ms[1], ms[2], ms[3], ms[4], ms[5]);
    }
};
}  // namespace

// the whole bzip2 buffer through `sink`; LRGE_ERR_PARSE / DEVICE as lrge_hip_bzip2_inflate
static int bzip2_inflate_impl(lrge_hip_ctx *ctx, const uint8_t *comp, uint64_t comp_len, int (*sink)(void *, const void *, uint64_t), void *user,
                              lrge_hip_bzip2_stats *stats) {
    (void)hipSetDevice(ctx->device);
    static const CodecText text = {"bzip2", bz_status_name, 0, nullptr};
    BzStats st;
    BzDev dev(ctx);
    return codec_inflate(dev, text, sink, user, [&](auto &to_sink, u64 *bad) { return bz_run(dev, comp, comp_len, ctx->opt_u64("BZIP2_ROUND_BLOCKS", 0), to_sink, st, bad); }, [&] {
        if (dev.timing) fprintf(stderr, "[lrge_hip] bzip2 stages ms: find %.3f entropy %.3f scatter %.3f walk %.3f rle_crc %.3f\n", dev.ms[0], dev.ms[1], dev.ms[2], dev.ms[3], dev.ms[4]);
        if (stats) { stats->blocks = st.blocks; stats->candidates = st.candidates; stats->rejected_candidates = st.rejected; stats->rounds = st.rounds; stats->bytes_out = st.bytes_out; }
    });
}

extern "C" int lrge_hip_bzip2_inflate(lrge_hip_ctx *ctx, const void *comp, uint64_t comp_len, int (*sink)(void *user, const void *bytes, uint64_t n),
                                      void *user, lrge_hip_bzip2_stats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (!ctx || !sink || (!comp && comp_len)) return LRGE_ERR_INVALID;
    return bzip2_inflate_impl(ctx, (const uint8_t *)comp, comp_len, sink, user, stats);
}
