// zs_round.h -- host side of the block-parallel Zstandard decode: the walk over frame and block headers, rounds of consecutive
// blocks, the table sources of treeless and repeat-mode blocks, the layout of a round's scratch, the scan that gives every block
// its place in the text and its incoming repeat offsets, and the frame checks (content size, checksum).  One template drives
// both the device (host_zstd.inl: kernels of k_zstd.h) and the host twin (zs_twin.cpp: the same steps as loops over zs_core.h),
// so the CPU suite tests this logic as the library runs it.
//
// The text of the whole call stays in one block of the backend: a match may reach back through every earlier block of its frame,
// in this round or in one before, and a deferred byte is read from there when its round is resolved.
//
// A backend that slides (slides(): DESIGN section 26) keeps less: a work text [history | round], where the history is the last
// min(frame_pos, window) bytes of the frame that is open when the round starts.  The positions the backend sees (ZsBlock::out, the
// spans of the checksums) are then positions in that work text; everything else -- frame_pos, the repeat offsets, the table
// sources, the statistics -- is the same.  The checksum of a frame that spans rounds continues from a state the backend keeps
// (zs_xxh64_part of zs_core.h).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "zs_core.h"

struct ZsStats { uint64_t frames, skippable, blocks, raw_blocks, rle_blocks, sequences, checksums_checked, rounds, bytes_out; };
// a sliding run: its rounds, the largest history carried into one, the largest work text [history | round], the bytes of all histories
struct ZsSlide { uint64_t rounds, max_history, max_work, moved; };
// one part of a frame's checksum (zs_xxh64_part): work text [at, at + len) goes into state `slot`; flags 1: the frame's first part, 2: its last
struct ZsXxhJob { uint64_t at, len; uint32_t slot, flags; };
struct ZsFrame {
    uint64_t at;                    // the frame's magic in the file
    uint64_t fcs;                   // Frame_Content_Size (has_fcs)
    uint64_t sum_at;                // where the checksum word stands (has_sum)
    uint32_t window, bmax;
    uint32_t first, n_blocks;       // its blocks in the table
    bool has_fcs, has_sum;
};

enum { ZS_RUN_OK = 0, ZS_RUN_DEVICE = -2 };
#define ZS_ROUND_MAX 4096u
// bytes of device memory a block of a round needs at most beside the text: literals, sequences (a match has three bytes or more),
// the origins of its bytes
static inline uint64_t zs_block_bytes() { return (uint64_t)ZS_BLOCK_MAX + (uint64_t)(ZS_BLOCK_MAX / 3) * sizeof(ZsSeq) + (uint64_t)ZS_BLOCK_MAX * 4 + sizeof(ZsBlock) + sizeof(ZsSeqRes); }

// the frames and blocks of d[0, n): a hop per block.  ZS_OK or a status with *bad the byte offset it belongs to
static inline int zs_walk(const uint8_t *d, uint64_t n, std::vector<ZsFrame> &frames, std::vector<ZsBlock> &blocks, uint64_t *skippable, uint64_t *bad) {
    uint64_t p = 0;
    *skippable = 0;
    while (p < n) {
        *bad = p;
        if (p + 4 > n) return ZS_E_INPUT;
        const uint32_t magic = zs_le32(d + p);
        if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {
            if (p + 8 > n) return ZS_E_INPUT;
            const uint64_t len = zs_le32(d + p + 4);
            if (p + 8 + len > n) return ZS_E_INPUT;
            p += 8 + len; ++*skippable;
            continue;
        }
        if (magic != 0xFD2FB528u) return ZS_E_MAGIC;
        ZsFrame f{};
        f.at = p;
        if (p + 5 > n) return ZS_E_INPUT;
        const uint32_t fhd = d[p + 4], fcs_flag = fhd >> 6, single = (fhd >> 5) & 1, did_flag = fhd & 3;
        if (fhd & 8) return ZS_E_RESERVED;
        f.has_sum = (fhd >> 2) & 1;
        uint64_t q = p + 5;
        uint64_t window = 0;
        if (!single) {
            if (q + 1 > n) return ZS_E_INPUT;
            const uint32_t wd = d[q++], wlog = 10 + (wd >> 3);
            if (wlog > 27) return ZS_E_WINDOW;
            window = ((uint64_t)1 << wlog) + (((uint64_t)1 << wlog) >> 3) * (wd & 7);
        }
        const uint32_t did_len = did_flag == 3 ? 4 : did_flag;
        if (q + did_len > n) return ZS_E_INPUT;
        uint32_t did = 0;
        for (uint32_t i = 0; i < did_len; ++i) did |= (uint32_t)d[q + i] << (8 * i);
        if (did) return ZS_E_DICT;
        q += did_len;
        const uint32_t fcs_len = fcs_flag == 0 ? single : 1u << fcs_flag;
        if (q + fcs_len > n) return ZS_E_INPUT;
        if (fcs_len) {
            f.has_fcs = true;
            for (uint32_t i = 0; i < fcs_len; ++i) f.fcs |= (uint64_t)d[q + i] << (8 * i);
            if (fcs_len == 2) f.fcs += 256;
            q += fcs_len;
        }
        if (single) window = f.fcs;
        if (window > ZS_WINDOW_MAX) return ZS_E_WINDOW;
        f.window = (uint32_t)window;
        f.bmax = (uint32_t)std::min<uint64_t>(window, ZS_BLOCK_MAX);
        f.first = (uint32_t)blocks.size();
        for (;;) {
            *bad = q;
            if (q + 3 > n) return ZS_E_INPUT;
            const uint32_t bh = zs_le24(d + q), last = bh & 1, type = (bh >> 1) & 3, size = bh >> 3;
            if (type == 3) return ZS_E_BLOCK_TYPE;
            if (size > f.bmax) return ZS_E_BLOCK_SIZE;
            q += 3;
            const uint64_t bytes = type == 1 ? 1 : size;
            if (q + bytes > n) return ZS_E_INPUT;
            ZsBlock b{};
            b.src = q; b.size = size; b.type = type; b.bmax = f.bmax; b.window = f.window;
            if (blocks.size() >= 0xFFFFFFFEull) return ZS_E_TOO_BIG;
            blocks.push_back(b);
            q += bytes;
            if (last) break;
        }
        f.n_blocks = (uint32_t)blocks.size() - f.first;
        if (f.has_sum) {
            *bad = q;
            if (q + 4 > n) return ZS_E_INPUT;
            f.sum_at = q; q += 4;
        }
        frames.push_back(f);
        p = q;
    }
    return ZS_OK;
}

// D (the decode backend):
//   bool load(const uint8_t *d, uint64_t n)                       the whole compressed input
//   uint32_t default_round()                                      blocks per round when the caller names none
//   bool heads(ZsBlock *b, uint32_t k)                            b[i].h of the compressed blocks among b[0, k)
//   bool entropy(const ZsBlock *b, uint32_t k, uint64_t lit_bytes, uint64_t n_seq, uint32_t *lit_status, ZsSeqRes *res)
//                                                                 literals and sequences of the round into its scratch
//   bool reserve(uint64_t bytes)                                  room for that many bytes behind the text so far; false with
//                                                                 over() when the budget does not hold them
//   bool execute(const ZsBlock *b, uint32_t k, const uint32_t *first_of_frame, uint32_t n_groups, uint64_t bytes, uint32_t *status)
//                                                                 the round's bytes behind the text, deferred sources resolved
//                                                                 (first_of_frame: where the blocks of each frame of the round start, and k)
//   bool xxh64(const uint64_t *at, const uint64_t *len, uint32_t m, uint64_t *h)
//                                                                 of text[at[i], at[i] + len[i]), the m frames at once
//   const uint8_t *bytes(uint64_t at, uint64_t len)               the text for the sink (nullptr: failure)
//   bool slides()                                                 the sliding mode.  Then also, with every position one of the work text:
//   bool plan(uint64_t work_bytes)                                once, before the first round: no work text is larger (false with over(): the budget)
//   bool slide(uint64_t history, uint64_t bytes)                  in front of execute: the work text is the `history` bytes retire() kept, then
//                                                                 room for the round's `bytes`
//   bool xxh64_part(const ZsXxhJob *job, uint32_t m, uint64_t *h) the m parts at once; h[i] counts for a last part
//   bool retire(uint64_t keep_bytes)                              the round is checked: its bytes go on to where the text is collected, and
//                                                                 the last keep_bytes of the work text are the next round's history
// sink(bytes, n) -> bool (false: stop with ZS_RUN_DEVICE)
// Returns ZS_RUN_OK, ZS_RUN_DEVICE or a ZS_E_* status (*bad_off: the byte offset it belongs to).
template <class D, class Sink>
static int zs_run(D &dev, const uint8_t *d, uint64_t n, uint64_t round_blocks, bool checksum, Sink &&sink, ZsStats &st, uint64_t *bad_off, ZsSlide *slide_out = nullptr) {
    memset(&st, 0, sizeof st);
    if (slide_out) memset(slide_out, 0, sizeof *slide_out);
    uint64_t bad_dummy = 0;
    uint64_t &bad = bad_off ? *bad_off : bad_dummy;
    bad = 0;
    std::vector<ZsFrame> frames;
    std::vector<ZsBlock> blocks;
    int rc = zs_walk(d, n, frames, blocks, &st.skippable, &bad);
    if (rc) return rc;
    st.frames = frames.size();
    if (!dev.load(d, n)) return ZS_RUN_DEVICE;
    const uint32_t K = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(round_blocks ? round_blocks : dev.default_round(), 1), ZS_ROUND_MAX);
    const uint64_t nb = blocks.size();
    const bool slide = dev.slides();
    if (slide) {
        // the largest work text of the run, from the headers alone: a block gives at most bmax bytes (raw and RLE: its size), and the
        // history is at most the window and at most what the frame's earlier blocks give
        uint64_t work = 0, fp = 0, in_round = 0, hist = 0;
        size_t f = 0;
        for (uint64_t i = 0; i < nb; ++i) {
            while (i >= (uint64_t)frames[f].first + frames[f].n_blocks) ++f;
            if (i == frames[f].first) fp = 0;
            if (i % K == 0) { in_round = 0; hist = std::min<uint64_t>(fp, frames[f].window); }
            const uint64_t ub = blocks[i].type == 2 ? blocks[i].bmax : blocks[i].size;
            fp += ub; in_round += ub;
            work = std::max(work, hist + in_round);
        }
        if (!dev.plan(work)) return dev.over() ? (int)ZS_E_TOO_BIG : (int)ZS_RUN_DEVICE;
    }
    ZsSlide sl = {0, 0, 0, 0};
    uint64_t H = 0;                                 // sliding: the history in front of the next round
    uint64_t hashed = 0; uint32_t slot = 0;         // sliding: the bytes of the open frame its checksum state holds, and which state
    std::vector<ZsXxhJob> jobs;
    std::vector<size_t> job_f;
    std::vector<uint64_t> job_h;
    // the state that crosses blocks and rounds, per frame
    size_t fi = 0;                                  // the frame of the next block
    uint64_t frame_pos = 0, frame_out = 0;          // bytes of that frame so far, where its text starts
    uint64_t text = 0;                              // bytes of text so far
    uint32_t rep[3] = {1, 4, 8};
    uint64_t huf_at = 0; uint32_t huf_len = 0;
    ZsTabSrc tab[3] = {{0, 0, 3}, {0, 0, 3}, {0, 0, 3}};          // mode 3: nothing in front
    std::vector<uint32_t> lit_status, ex_status, groups;
    std::vector<ZsSeqRes> res;
    std::vector<uint64_t> sum_at, sum_len, sum_h;
    std::vector<size_t> sum_f;
    for (uint64_t i = 0; i < nb;) {
        const uint32_t k = (uint32_t)std::min<uint64_t>(K, nb - i);
        ZsBlock *B = &blocks[i];
        ++st.rounds;
        if (!dev.heads(B, k)) return ZS_RUN_DEVICE;
        // table sources, scratch layout
        uint64_t lit_bytes = 0, n_seq = 0;
        {
            size_t f = fi;
            uint64_t hat = huf_at; uint32_t hlen = huf_len;
            ZsTabSrc tb[3] = {tab[0], tab[1], tab[2]};
            for (uint32_t j = 0; j < k; ++j) {
                ZsBlock &b = B[j];
                while (i + j >= (uint64_t)frames[f].first + frames[f].n_blocks) ++f;
                if (i + j == frames[f].first) { hlen = 0; for (auto &x : tb) x = ZsTabSrc{0, 0, 3}; }
                if (b.type != 2) continue;
                const ZsHead &h = b.h;
                bad = b.src;
                if (h.status) return (int)h.status;
                if (h.lit_type == 2) { hat = b.src + h.lit_at; hlen = h.huf_len; }
                if (h.lit_type >= 2) { if (!hlen) return ZS_E_NO_TABLE; b.huf_at = hat; b.huf_len = hlen; }
                if (h.nseq) {
                    for (uint32_t t = 0; t < 3; ++t) {
                        const uint32_t mode = (h.modes >> (4 - 2 * t)) & 3;
                        if (mode == 3) { if (tb[t].mode == 3) return ZS_E_NO_TABLE; }
                        else tb[t] = ZsTabSrc{b.src + h.tab_at[t], mode == 2 ? (t < 2 ? h.tab_at[t + 1] : h.bits_at) - h.tab_at[t] : (uint32_t)(mode == 1), mode};
                        b.tab[t] = tb[t];
                    }
                }
                b.lit_off = lit_bytes; lit_bytes += h.regen;
                b.seq_off = n_seq; n_seq += h.nseq;
            }
            // (the state moves on only when the round is accepted: below)
        }
        lit_status.assign(k, 0); res.assign(k, ZsSeqRes{});
        if (!dev.entropy(B, k, lit_bytes, n_seq, lit_status.data(), res.data())) return ZS_RUN_DEVICE;
        // the scan: places, repeat offsets, frame ends
        groups.clear();
        uint64_t round_bytes = 0;
        const uint64_t text0 = text;
        // Sliding: the round's work text is [history | round], and a position in it is the position in the call's text minus
        // `shift`.  H (left by the round before) is the last min(frame_pos, window) bytes of the frame that is still open, 0 when
        // the round starts with a frame's first block.  That is enough: a block of the open frame at frame_pos has the history's
        // first byte min(frame_pos', window) bytes in front of the round (frame_pos' <= frame_pos: the frame's bytes then), and
        // zs_execute refuses off > frame_pos + op and off > window, so no source lies in front of it; a frame that starts inside
        // the round has frame_pos 0 at its first block, which stands behind the history, and the same refusal keeps its sources
        // inside the round.  A deferred byte's origin is a source of that kind, so the resolve stays inside as well.
        const uint64_t shift = slide ? text0 - H : 0;
        const bool mid = slide && H > 0;            // (H > 0: the open frame has bytes, so it is in front of this round's first block)
        const size_t f_mid = fi;
        const uint64_t fp0 = frame_pos;
        struct Done { size_t f; uint64_t out, len; };
        std::vector<Done> done;
        for (uint32_t j = 0; j < k; ++j) {
            ZsBlock &b = B[j];
            while (i + j >= (uint64_t)frames[fi].first + frames[fi].n_blocks) ++fi;
            const ZsFrame &f = frames[fi];
            if (i + j == f.first) {
                frame_pos = 0; frame_out = text; rep[0] = 1; rep[1] = 4; rep[2] = 8; huf_len = 0;
                for (auto &x : tab) x = ZsTabSrc{0, 0, 3};
            }
            if (j == 0 || i + j == f.first) groups.push_back(j);
            bad = b.src;
            b.frame_pos = frame_pos; b.out = text - shift;
            memcpy(b.rep, rep, sizeof rep);
            if (b.type != 2) { b.out_size = b.size; st.raw_blocks += b.type == 0; st.rle_blocks += b.type == 1; }
            else {
                if (lit_status[j]) return (int)lit_status[j];
                if (res[j].status) return (int)res[j].status;
                b.out_size = res[j].out_size;
                if (b.out_size > b.bmax) return ZS_E_BLOCK_SIZE;
                uint32_t next[3];
                if (!zs_rep_apply(res[j].f, rep, next)) return ZS_E_OFFSET;
                memcpy(rep, next, sizeof rep);
                if (b.h.lit_type == 2) { huf_at = b.huf_at; huf_len = b.huf_len; }
                if (b.h.nseq) for (uint32_t t = 0; t < 3; ++t) tab[t] = b.tab[t];
                st.sequences += b.h.nseq;
            }
            frame_pos += b.out_size; text += b.out_size; round_bytes += b.out_size;
            if (f.has_fcs && frame_pos > f.fcs) { bad = f.at; return ZS_E_CONTENT_SIZE; }
            if (i + j + 1 == (uint64_t)f.first + f.n_blocks) done.push_back(Done{fi, frame_out, frame_pos});
        }
        groups.push_back(k);
        if (slide) {
            ++sl.rounds; sl.max_history = std::max(sl.max_history, H); sl.max_work = std::max(sl.max_work, H + round_bytes); sl.moved += H;
            if (slide_out) *slide_out = sl;
        }
        if (!dev.reserve(round_bytes)) return dev.over() ? (int)ZS_E_TOO_BIG : (int)ZS_RUN_DEVICE;
        if (slide && !dev.slide(H, round_bytes)) return dev.over() ? (int)ZS_E_TOO_BIG : (int)ZS_RUN_DEVICE;
        ex_status.assign(k, 0);
        if (!dev.execute(B, k, groups.data(), (uint32_t)groups.size() - 1, round_bytes, ex_status.data())) return ZS_RUN_DEVICE;
        for (uint32_t j = 0; j < k; ++j) if (ex_status[j]) { bad = B[j].src; return (int)ex_status[j]; }
        // the frames that ended in this round: content size, then the checksums of all of them in one launch
        // Sliding: a frame that was open when the round started, or stays open behind it, is hashed in parts.  A part starts at
        // the frame byte `hashed`, a multiple of 32 and at most 31 bytes in front of the round: inside the history, which is the
        // frame's last min(frame_pos, window) bytes with a window of 1 KiB at the least, or of the whole frame (single segment)
        sum_at.clear(); sum_len.clear(); sum_f.clear(); jobs.clear(); job_f.clear();
        const bool open_end = slide && i + k < (uint64_t)frames[fi].first + frames[fi].n_blocks;
        const bool sum_mid = mid && frames[f_mid].has_sum && checksum;      // the frame in front of the round goes on in it (done[0], or open behind it too)
        if (sum_mid && fp0 - hashed > H) return ZS_RUN_DEVICE;               // (never: see above)
        for (const Done &x : done) {
            const ZsFrame &f = frames[x.f];
            if (f.has_fcs && x.len != f.fcs) { bad = f.at; return ZS_E_CONTENT_SIZE; }
            if (!(f.has_sum && checksum)) continue;
            if (sum_mid && x.f == f_mid) { jobs.push_back(ZsXxhJob{x.out + hashed - shift, x.len - hashed, slot, 2}); job_f.push_back(x.f); }
            else { sum_at.push_back(x.out - shift); sum_len.push_back(x.len); sum_f.push_back(x.f); }
        }
        if (open_end && frames[fi].has_sum && checksum) {
            const bool first = !(mid && done.empty());     // the frame started in this round
            if (first) { hashed = 0; slot ^= 1; }
            const uint64_t len = frame_pos - hashed;
            jobs.push_back(ZsXxhJob{frame_out + hashed - shift, len, slot, first ? 1u : 0u}); job_f.push_back((size_t)-1);
            hashed += len / 32 * 32;
        }
        if (!jobs.empty()) {
            job_h.assign(jobs.size(), 0);
            if (!dev.xxh64_part(jobs.data(), (uint32_t)jobs.size(), job_h.data())) return ZS_RUN_DEVICE;
            for (size_t a = 0; a < jobs.size(); ++a) {
                if (job_f[a] == (size_t)-1) continue;
                ++st.checksums_checked;
                if ((uint32_t)job_h[a] != zs_le32(d + frames[job_f[a]].sum_at)) { bad = frames[job_f[a]].sum_at; return ZS_E_CHECKSUM; }
            }
        }
        if (!sum_f.empty()) {
            sum_h.assign(sum_f.size(), 0);
            if (!dev.xxh64(sum_at.data(), sum_len.data(), (uint32_t)sum_f.size(), sum_h.data())) return ZS_RUN_DEVICE;
            for (size_t a = 0; a < sum_f.size(); ++a) {
                ++st.checksums_checked;
                if ((uint32_t)sum_h[a] != zs_le32(d + frames[sum_f[a]].sum_at)) { bad = frames[sum_f[a]].sum_at; return ZS_E_CHECKSUM; }
            }
        }
        st.blocks += k;
        if (slide) {
            // what the next round needs: the last min(window, frame_pos) bytes of the frame that is still open, nothing behind a frame's end
            H = open_end ? std::min<uint64_t>(frames[fi].window, frame_pos) : 0;
            if (!dev.retire(H)) return ZS_RUN_DEVICE;
        }
        if (round_bytes) {
            const uint8_t *bytes = dev.bytes(text0 - shift, round_bytes);
            if (!bytes || !sink(bytes, round_bytes)) return ZS_RUN_DEVICE;
        }
        st.bytes_out += round_bytes;
        i += k;
    }
    return ZS_RUN_OK;
}
