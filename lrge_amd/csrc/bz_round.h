// bz_round.h -- host side of the block-parallel bzip2 decode: the stream header, rounds of candidates, the chain that accepts
// blocks, the block and stream CRC checks and the tail rule.  One template drives both the device (host_bzip2.inl: kernels of
// k_bzip2.h) and the host twin (bz_twin.cpp: the same steps as loops over bz_core.h), so the CPU suite tests this logic as the
// library runs it.
//
// The finder is exhaustive: it reports every bit offset that carries the block magic or the end-of-stream magic, so every true
// block start is a candidate and nothing is ever decoded again.  A round decodes the next `round_blocks` candidates.
//
// Chain argument.  The first block starts at bit 32.  A block decoded from a true start follows the real stream, so it ends where
// the next block, or the end of the stream, really starts.  Candidate c is accepted if and only if its position is the end of the
// last accepted block; then it is a true start too.  A candidate in front of that position is a false one (48 bits of block data
// that look like a magic): it is counted and its output is never used, whatever status it ended with.  An accepted block must
// have decoded with BZ_OK and its bytes must give its stored CRC.  An end position that is no candidate means damage.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "bz_core.h"

struct BzStats { uint64_t blocks, candidates, rejected, rounds, bytes_out; };
// an accepted block of a round: its slot among the round's decodes, its place in the round's links and text
struct BzLink { uint64_t tt_off, out_off; uint32_t slot, n, orig, run_open; };   // run_open: bz_rle_len's BZ_RUN_OPEN

enum { BZ_RUN_OK = 0, BZ_RUN_DEVICE = -2 };
#define BZ_ROUND_MAX 4096u      // candidates per round at most

// bytes of device memory one candidate of a round needs at block size bs: L (later the bytes in front of the run-length layer),
// the links of the inverse BWT, the counts; the text itself comes on top
static inline uint64_t bz_candidate_bytes(uint32_t bs) { return (uint64_t)bs * 5 + 256 * 4 + 256; }

// 32 bits at bit offset `pos` of d[0, n), zero past the end
static inline uint32_t bz_host_bits32(const uint8_t *d, uint64_t n, uint64_t pos) {
    BzBits b;
    bz_bits_init(b, d, n, pos);
    return bz_peek32(b);
}

// What a recorder sees of a round, after its checks: the accepted links in order (slot: the candidate among pos / res), the stored CRCs
// their texts gave, the text offset of the round's first byte and the round's text bytes
struct BzRound { const uint64_t *pos; const BzRes *res; const BzLink *links; uint32_t m; const uint32_t *stored; uint64_t text_base, out_bytes; };

// The recorder of a census that leaves a seek map (fx_seek.h FX_SEEK_BZIP2; Map: FxSeekMap): it keeps the block
// table, groups the blocks into entries by the spacing and asks the backend once a round for the marks of the accepted blocks, which
// `finish` left when the backend was told to record (keep_marks): bool marks_out(BzMark *dst, uint32_t m) -- BZ_MARKS marks a link,
// in the links' order, in one copy down.  One template for device and twin, as GzSeekRec is
template <class D, class Map> struct BzSeekRec {
    Map *m;
    uint64_t spacing;
    bool round(D &dev, const BzRound &r) {
        if (!r.m) return true;
        for (uint32_t a = 0; a < r.m; ++a) {
            const BzLink &l = r.links[a];
            const uint64_t off = r.text_base + l.out_off, len = (a + 1 < r.m ? r.links[a + 1].out_off : r.out_bytes) - l.out_off;
            if (m->bz_ent.empty() || off >= m->bz_ent.back().off + spacing) m->bz_ent.push_back({m->bz.size(), m->bz.size(), off, 0});
            auto &e = m->bz_ent.back();
            m->bz.push_back({r.pos[l.slot], r.res[l.slot].end_bit, off, len, l.n, l.orig, r.stored[a], (uint32_t)(m->bz_ent.size() - 1)});
            ++e.b1; e.len += len;
        }
        const size_t at = m->bz_marks.size();
        m->bz_marks.resize(at + (size_t)r.m * BZ_MARKS);
        return dev.marks_out(&m->bz_marks[at], r.m);
    }
};
struct BzNoRec { template <class D> bool round(D &, const BzRound &) { return true; } };

// D (the decode backend):
//   bool load(const uint8_t *d, uint64_t n)                       the whole compressed input
//   bool find(std::vector<uint64_t> &cand)                        every bit offset with a magic, ascending (BZ_END_FLAG: the end magic)
//   uint32_t default_round(uint32_t bs)                           candidates per round when the caller names none
//   bool decode(const uint64_t *pos, uint32_t k, uint32_t bs, BzRes *res)   the entropy decode of k candidates into slots 0..k-1
//   bool finish(BzLink *l, uint32_t m, uint32_t *crc, uint64_t *out_bytes, const uint8_t **bytes)
//                                                                 inverse BWT and run-length layer of the accepted slots, in order;
//                                                                 fills tt_off / out_off / run_open, the CRC of every block's text, the text
// sink(bytes, n) -> bool (false: stop with BZ_RUN_DEVICE)
// cand_in: a candidate list instead of the finder's (tests).
// rec: a recorder (rec->round(dev, BzRound) after every round's checks; false: stop with BZ_RUN_DEVICE), or null: nothing more is asked of the backend
// Returns BZ_RUN_OK, BZ_RUN_DEVICE or a BZ_E_* status (*bad_off: the byte offset it belongs to).
template <class D, class Sink, class Rec = BzNoRec>
static int bz_run(D &dev, const uint8_t *d, uint64_t n, uint64_t round_blocks, Sink &&sink, BzStats &st, uint64_t *bad_off,
                  const std::vector<uint64_t> *cand_in = nullptr, Rec *rec = nullptr) {
    memset(&st, 0, sizeof st);
    uint64_t bad_dummy = 0;
    uint64_t &bad = bad_off ? *bad_off : bad_dummy;
    bad = 0;
    if (n < 4 || d[0] != 'B' || d[1] != 'Z' || d[2] != 'h' || d[3] < '1' || d[3] > '9') return BZ_E_MAGIC;
    const uint32_t bs = (uint32_t)(d[3] - '0') * 100000u;
    if (!dev.load(d, n)) return BZ_RUN_DEVICE;
    std::vector<uint64_t> cand;
    if (cand_in) cand = *cand_in;
    else if (!dev.find(cand)) return BZ_RUN_DEVICE;
    std::vector<uint64_t> B, E;                       // block starts, stream ends
    for (uint64_t c : cand) (c & BZ_END_FLAG ? E : B).push_back(c & ~BZ_END_FLAG);
    st.candidates = B.size();
    const uint32_t K = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(round_blocks ? round_blocks : dev.default_round(bs), 1), BZ_ROUND_MAX);
    uint64_t expect = 32;                             // where the chain stands: the end of the last accepted block
    uint32_t combined = 0;
    size_t i = 0;
    std::vector<BzRes> res;
    std::vector<BzLink> links;
    std::vector<uint32_t> crc, stored;
    for (;;) {
        if (std::binary_search(E.begin(), E.end(), expect)) {        // the end of the stream: combined CRC, padding, nothing behind
            bad = expect >> 3;
            if (expect + 80 > 8 * n) return BZ_E_INPUT;
            if (bz_host_bits32(d, n, expect + 48) != combined) return BZ_E_STREAM_CRC;
            if ((expect + 80 + 7) >> 3 != n) { bad = (expect + 80 + 7) >> 3; return BZ_E_TRAILING; }
            st.rejected += B.size() - i;
            return BZ_RUN_OK;
        }
        while (i < B.size() && B[i] < expect) { ++i; ++st.rejected; }
        if (i == B.size() || B[i] != expect) { bad = expect >> 3; return expect + 48 > 8 * n ? (int)BZ_E_INPUT : (int)BZ_E_CHAIN; }
        const uint32_t k = (uint32_t)std::min<uint64_t>(K, B.size() - i);
        ++st.rounds;
        res.assign(k, BzRes{0, 0, 0, 0, 0});
        if (!dev.decode(&B[i], k, bs, res.data())) return BZ_RUN_DEVICE;
        links.clear(); stored.clear();
        uint32_t j = 0;
        for (; j < k; ++j) {
            if (B[i + j] < expect) { ++st.rejected; continue; }
            if (B[i + j] > expect) break;                            // the chain left the candidates: the end of the stream, or damage
            const BzRes &r = res[j];
            if (r.status != BZ_OK) { bad = expect >> 3; return (int)r.status; }
            links.push_back(BzLink{0, 0, j, r.n, r.orig, 0});
            stored.push_back(r.crc);
            expect = r.end_bit;
        }
        const uint64_t first = B[i], *round_pos = &B[i];
        i += j;
        const uint32_t m = (uint32_t)links.size();
        crc.assign(m, 0);
        uint64_t out_bytes = 0;
        const uint8_t *bytes = nullptr;
        if (!dev.finish(links.data(), m, crc.data(), &out_bytes, &bytes)) return BZ_RUN_DEVICE;
        for (uint32_t a = 0; a < m; ++a) {
            if (links[a].run_open || crc[a] != stored[a]) {
                bad = (a ? res[links[a - 1].slot].end_bit : first) >> 3;
                return links[a].run_open ? BZ_E_RUN : BZ_E_BLOCK_CRC;
            }
            combined = bz_rotl1(combined) ^ crc[a];
        }
        st.blocks += m;
        if (rec && !rec->round(dev, BzRound{round_pos, res.data(), links.data(), m, stored.data(), st.bytes_out, out_bytes})) return BZ_RUN_DEVICE;
        if (out_bytes && !sink(bytes, out_bytes)) return BZ_RUN_DEVICE;
        st.bytes_out += out_bytes;
    }
}
