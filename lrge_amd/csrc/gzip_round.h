// gzip_round.h -- host side of the speculative gzip decode: rounds, chunks, the chain walk, window bookkeeping and the
// member checks.  One template drives both the device (host_gzip.inl: kernels of k_gzip.h) and the host twin
// (gzip_twin.cpp: the same steps run sequentially on the CPU), so the CPU suite tests this logic as the library runs it.
//
// A round takes at most `round` compressed bytes from where the previous round really ended (plus an overhang, so the last
// chunk can reach its stop).  It is cut into nominal chunks of `chunk` bytes.  Chunk 0 starts at the known position; the
// finder gives every other chunk its smallest candidate boundary, chunks without one are merged into their predecessor.
// Each surviving chunk is decoded from its candidate to the next survivor's candidate (gz_decode's stop rule).
//
// Chain argument.  Chunk 0 starts at a true boundary.  A chunk decoded from a true boundary follows the real stream, so it
// stops at the first true boundary at or past its stop; its symbols are exact up to the window.  The walk accepts chunk k
// only when the accepted chunk k-1 ended exactly at k's candidate; then k also started at a true boundary, with the member
// state that the stream has there (a member header starts a member; a block start continues the one k-1 was in).  Any other
// chunk is decoded again from k-1's true end.  So every accepted chunk is a true decode and no output of a false start is used.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "fx_seek.h"
#include "gzip_core.h"

struct GzStats { uint64_t members, chunks, speculative, rejected, redecoded, overflow_retries, bytes_out; };
struct GzCfg { uint64_t chunk, round, ratio; };

// one chunk decode: [start, stop) of the round's buffer, symbols into the task's slot (cap symbols, seg_cap segments)
struct GzTask { uint32_t start, stop, cap, seg_cap; uint64_t sym_off; uint32_t seg_off, big; };   // big: extra buffer big - 1 (0: the slots)
// an accepted chunk: where its symbols are (its task's slot, or extra buffer big - 1 at sym_off), where its bytes go in the
// round's output, how many bytes of its window belong to its member, its segments in the round's flat segment list, its start
struct GzLink { uint64_t sym_off, out_off; uint32_t big, n_sym, valid, seg0, nseg, start; };   // start: round-relative bit

enum { GZ_RUN_OK = 0, GZ_RUN_TOO_MANY = -1, GZ_RUN_DEVICE = -2 };

#define GZ_MAX_SEGS_PER_CHUNK 512u
#define GZ_RETRY_FACTOR 4u

#define GZ_SLOT_BUDGET ((uint64_t)4 << 30)   // bytes of symbol slots per round: a round holds at most this / slot chunks
#define GZ_STORED_MAX 65540u                 // the longest stored block with its header

static inline uint64_t gz_slot_symbols(const GzCfg &c) { return std::max<uint64_t>(c.ratio * c.chunk, 65536); }
static inline uint32_t gz_slot_segs(const GzCfg &c) { return (uint32_t)std::min<uint64_t>(c.chunk / 8 + 4, GZ_MAX_SEGS_PER_CHUNK); }

// What a recorder sees of a round, after `finish`: the accepted links, their segments and the segments' CRCs, the byte of the file the
// round's bit offsets count from, the text offset of the round's first byte and whether the stream is inside a member at the first link
struct GzRound { uint64_t R0, text_base; const GzLink *links; uint32_t nl; const GzSeg *segs; const uint32_t *seg_crc; bool in_member; };

// The recorder of a census that leaves a seek map (fx_seek.h FX_SEEK_GZIP): it keeps the entry table.  Entry 0 is the
// first link of the file (bit 0, an empty window); after that an accepted link becomes an entry when its text offset is at least `spacing`
// behind the previous entry's.  A link's text CRC is the fold of its segments' CRCs, an entry's the fold of its links'.  The windows of
// the round's new entries come from the backend in one call: bool windows_out(const uint32_t *link, uint32_t k, uint8_t *dst) -- window
// of link[i] (as `finish` left it) to dst + i * GZ_WIN
template <class D> struct GzSeekRec {
    FxSeekMap *m;
    uint64_t spacing;
    bool round(D &dev, const GzRound &r) {
        std::vector<uint32_t> pick;
        bool in = r.in_member;
        for (uint32_t k = 0; k < r.nl; ++k) {
            const GzLink &l = r.links[k];
            const uint64_t off = r.text_base + l.out_off;
            ++m->gz_links;
            if (m->ent.empty() || off >= m->ent.back().off + spacing) {
                m->ent.push_back(FxGzEntry{r.R0 * 8 + l.start, off, 0, 0, in ? l.valid : 0, in ? 1u : 0u, 0});
                pick.push_back(k);
            }
            FxGzEntry &e = m->ent.back();
            for (uint32_t s = l.seg0; s < l.seg0 + l.nseg; ++s) {
                const GzSeg &g = r.segs[s];
                e.crc = inf_crc_shift(e.crc, g.o1 - g.o0) ^ r.seg_crc[s];
                e.len += g.o1 - g.o0;
                if (g.flags & GZ_SEG_HEAD) in = true;
                if (g.flags & GZ_SEG_TRAIL) in = false;
            }
        }
        if (pick.empty()) return true;
        const size_t at = m->ent_win.size();
        m->ent_win.resize(at + pick.size() * (size_t)GZ_WIN);
        return dev.windows_out(pick.data(), (uint32_t)pick.size(), &m->ent_win[at]);
    }
};
struct GzNoRec { template <class D> bool round(D &, const GzRound &) { return true; } };

// D (the decode backend):
//   bool load(const uint8_t *d, uint64_t off, uint32_t n)         the round's bytes d[off, off + n)
//   void prefetch(const uint8_t *d, uint64_t off, uint32_t n)     a hint: the next round will likely lie inside d[off, off + n)
//                                                                  (the device stages it while the current round decodes)
//   bool find(uint32_t chunk, uint32_t nc, uint32_t lim, uint32_t *cand)   cand[c], 0 < c < nc: the smallest candidate bit
//                                                                  offset in [8 c chunk, 8 min((c+1) chunk, lim)), or GZ_NONE
//   bool decode(const GzTask *t, uint32_t nt, bool eof, GzRes *res) (t[i].big > 0: into extra buffer big - 1 of the round at
//                                                                  sym_off / seg_off; every task of one call in the same buffer,
//                                                                  made by the backend for that call)
//   bool launch(const GzTask *t, uint32_t nt, bool eof), bool wait(GzRes *res)   decode in two steps (host work in between)
//   bool segs(const GzTask &t, uint32_t n, GzSeg *out)            the task's segment records
//   bool finish(const GzLink *l, uint32_t nl, const GzSeg *s, uint32_t ns, uint64_t out_bytes, uint32_t *seg_crc,
//               uint32_t *marker_err, const uint8_t **bytes)       windows, resolve, segment CRCs (marker_err: 1 + the first
//                                                                  link with a bad marker, or 0); the bytes' host copy may
//                                                                  still be in flight:
//   bool bytes_ready()                                             waits for it
// sink(bytes, n) -> bool (false: stop with GZ_RUN_DEVICE)
// rec: a recorder (rec->round(dev, GzRound) after every round's member checks; false: stop with GZ_RUN_DEVICE), or null: nothing more is asked of the backend
// Returns GZ_RUN_OK, GZ_RUN_TOO_MANY, GZ_RUN_DEVICE, or an INF_E_* / GZ_E_* status (*bad_off: file offset of the chunk).
template <class D, class Sink, class Rec = GzNoRec>
static int gz_run(D &dev, const uint8_t *d, uint64_t n, GzCfg cfg, Sink &&sink, GzStats &st, uint64_t *bad_off, Rec *rec = nullptr) {
    memset(&st, 0, sizeof st);
    cfg.chunk = std::min<uint64_t>(std::max<uint64_t>(cfg.chunk, 64), (uint64_t)64 << 20);
    cfg.ratio = std::min<uint64_t>(std::max<uint64_t>(cfg.ratio, 1), 64);
    const uint64_t S = gz_slot_symbols(cfg);
    const uint32_t SG = gz_slot_segs(cfg);
    // device memory stays bounded: at most GZ_SLOT_BUDGET bytes of slots per round
    const uint64_t max_round = std::max<uint64_t>(1, GZ_SLOT_BUDGET / (2 * S)) * cfg.chunk;
    cfg.round = std::min<uint64_t>(std::min<uint64_t>(std::max<uint64_t>(cfg.round, cfg.chunk), (uint64_t)256 << 20), max_round);
    const uint64_t overhang = cfg.chunk + ((uint64_t)1 << 20);
    uint64_t pos = 0;                        // absolute bit offset where the next round starts (a true boundary)
    bool in_member = false;                  // the stream is inside a member there
    uint32_t valid = 0;                      // bytes of the carried window that belong to that member
    uint32_t mcrc = 0; uint64_t msize = 0;   // that member's CRC and size so far
    uint64_t text_base = 0;                  // text bytes of the rounds before this one
    const uint8_t *pend = nullptr; uint64_t pend_n = 0;      // the previous round's bytes, delivered while this round decodes
    auto flush = [&]() -> bool {
        if (!pend_n) return true;
        if (!dev.bytes_ready() || !sink(pend, pend_n)) return false;
        st.bytes_out += pend_n; pend_n = 0;
        return true;
    };
    if (bad_off) *bad_off = 0;
    if (n == 0) return GZ_E_HEADER;
    for (;;) {
        const uint64_t R0 = pos >> 3;
        const uint32_t sb = (uint32_t)(pos & 7);
        const uint64_t lim64 = std::min<uint64_t>(cfg.round, n - R0);
        const bool final = R0 + lim64 == n;
        const uint64_t L = final ? lim64 : std::min<uint64_t>(n - R0, lim64 + overhang);
        const bool eof = R0 + L == n;
        const uint32_t lim = (uint32_t)lim64, nc = (uint32_t)((lim64 + cfg.chunk - 1) / cfg.chunk);
        if (lim == 0) return INF_E_INPUT;
        if (!dev.load(d, R0, (uint32_t)L)) return GZ_RUN_DEVICE;
        std::vector<uint32_t> cand(nc, GZ_NONE);
        cand[0] = sb;
        if (nc > 1 && !dev.find((uint32_t)cfg.chunk, nc, lim, cand.data())) return GZ_RUN_DEVICE;
        std::vector<uint32_t> surv;
        for (uint32_t c = 0; c < nc; ++c) if (cand[c] != GZ_NONE) surv.push_back(c);
        const uint32_t ns = (uint32_t)surv.size();
        std::vector<GzTask> task(ns);
        for (uint32_t j = 0; j < ns; ++j) {
            const uint32_t a = surv[j], b = j + 1 < ns ? surv[j + 1] : nc;
            task[j] = GzTask{cand[a], j + 1 < ns ? cand[b] : (final ? GZ_NONE : 8 * lim), (uint32_t)std::min<uint64_t>((b - a) * S, 0x7FFFFFFFu),
                             (b - a) * SG, (uint64_t)a * S, a * SG, 0};
        }
        st.chunks += nc; st.speculative += ns - 1;
        std::vector<GzRes> res(ns);
        if (!dev.launch(task.data(), ns, eof)) return GZ_RUN_DEVICE;
        // while the round decodes: stage the next round's bytes (it starts within a chunk before this round's nominal end, or
        // within the overhang after it) and deliver the previous round's
        if (!final) {
            const uint64_t off = R0 + lim64 - std::min<uint64_t>(lim64, cfg.chunk + 16);
            dev.prefetch(d, off, (uint32_t)std::min<uint64_t>(n - off, cfg.chunk + 16 + cfg.round + overhang));
        }
        if (!flush()) return GZ_RUN_DEVICE;
        if (!dev.wait(res.data())) return GZ_RUN_DEVICE;
        uint32_t n_big = 0;
        // repair in one batch: a chunk whose predecessor did not stop at its candidate is decoded again, all of them in one
        // launch, from where that predecessor stopped, into a buffer of their own (the first decode is kept: the predecessor
        // may be the false one).  The walk takes whichever of the two starts where the chain arrives.
        std::vector<GzTask> alt_t(ns);
        std::vector<GzRes> alt_r(ns);
        std::vector<uint8_t> has_alt(ns, 0);
        {
            std::vector<uint32_t> idx;
            std::vector<GzTask> fix;
            uint64_t so = 0; uint32_t go = 0;
            for (uint32_t j = 1; j < ns; ++j) {
                const GzRes &p = res[j - 1];
                if (p.status == INF_OK && !p.eof && p.end_bit != task[j].start && p.end_bit < task[j].stop) {
                    GzTask f = task[j];
                    f.start = p.end_bit; f.sym_off = so; f.seg_off = go;
                    so += f.cap; go += f.seg_cap;
                    idx.push_back(j); fix.push_back(f);
                }
            }
            if (!fix.empty()) {
                const uint32_t big = ++n_big;
                for (GzTask &f : fix) f.big = big;
                std::vector<GzRes> fr(fix.size());
                if (!dev.decode(fix.data(), (uint32_t)fix.size(), eof, fr.data())) return GZ_RUN_DEVICE;
                for (size_t i = 0; i < idx.size(); ++i) { alt_t[idx[i]] = fix[i]; alt_r[idx[i]] = fr[i]; has_alt[idx[i]] = 1; }
                st.redecoded += idx.size();
            }
        }
        // the chain walk
        std::vector<GzLink> links;
        std::vector<GzSeg> segs;
        uint32_t expect = sb;
        bool done = false;
        uint64_t out_bytes = 0;
        for (uint32_t j = 0; j < ns && !done; ++j) {
            GzTask t = task[j];
            GzRes r = res[j];
            if (t.start != expect) {                             // the finder's start is not where the chain arrives: rejected
                ++st.rejected;
                if (has_alt[j] && alt_t[j].start == expect) { t = alt_t[j]; r = alt_r[j]; }
                else {
                    ++st.redecoded;
                    t.start = expect;
                    if (!dev.decode(&t, 1, eof, &r)) return GZ_RUN_DEVICE;
                }
            }
            if (r.status == GZ_E_OVERFLOW || r.status == GZ_E_SEGS) {
                ++st.overflow_retries;
                GzTask big = t;
                big.cap = (uint32_t)std::min<uint64_t>((uint64_t)t.cap * GZ_RETRY_FACTOR, 0x7FFFFFFFu);
                big.seg_cap = t.seg_cap * GZ_RETRY_FACTOR; big.big = ++n_big; big.sym_off = 0; big.seg_off = 0;
                if (!dev.decode(&big, 1, eof, &r)) return GZ_RUN_DEVICE;
                if (r.status == GZ_E_OVERFLOW || r.status == GZ_E_SEGS) return GZ_RUN_TOO_MANY;
                t = big;
            }
            // ran out of the round's bytes (not the input's): the next round starts here.  A first chunk that does is one
            // block longer than the overhang, which the device does not prove.  Anything else short of input is damage.
            if (r.status == INF_E_INPUT && !eof && (uint64_t)r.end_bit + 8ull * GZ_STORED_MAX >= 8 * L) {
                if (j == 0) return GZ_RUN_TOO_MANY;
                break;
            }
            if (r.status != INF_OK) { if (bad_off) *bad_off = R0 + (t.start >> 3); return (int)r.status; }
            GzLink l{t.sym_off, out_bytes, t.big, r.n_sym, 0, (uint32_t)segs.size(), r.n_seg, t.start};
            segs.resize(segs.size() + r.n_seg);
            if (r.n_seg && !dev.segs(t, r.n_seg, &segs[l.seg0])) return GZ_RUN_DEVICE;
            // the window of this chunk: `valid` bytes of its member; then what the next chunk's window holds of its member
            l.valid = valid;
            uint32_t last_head = GZ_NONE;
            for (uint32_t s = 0; s < l.nseg; ++s) if (segs[l.seg0 + s].flags & GZ_SEG_HEAD) last_head = segs[l.seg0 + s].o0;
            const uint64_t v = last_head == GZ_NONE ? (uint64_t)valid + l.n_sym : (uint64_t)l.n_sym - last_head;
            valid = (uint32_t)std::min<uint64_t>(v, GZ_WIN);
            links.push_back(l);
            out_bytes += l.n_sym;
            expect = r.end_bit;
            done = r.eof != 0;
        }
        if (links.empty()) return GZ_RUN_TOO_MANY;
        if (!done && final) return INF_E_INPUT;                  // (the last chunk of the last round runs to the end)
        std::vector<uint32_t> seg_crc(segs.size(), 0);
        uint32_t marker_err = 0;
        const uint8_t *bytes = nullptr;
        if (!dev.finish(links.data(), (uint32_t)links.size(), segs.data(), (uint32_t)segs.size(), out_bytes, seg_crc.data(), &marker_err, &bytes))
            return GZ_RUN_DEVICE;
        if (marker_err) { if (bad_off) *bad_off = R0 + (links[marker_err - 1].start >> 3); return GZ_E_MARKER; }
        const bool in0 = in_member;
        // member checks: every segment's CRC folded into its member's
        for (uint32_t s = 0; s < segs.size(); ++s) {
            const GzSeg &g = segs[s];
            if (g.flags & GZ_SEG_HEAD) { if (in_member) return GZ_E_HEADER; in_member = true; mcrc = 0; msize = 0; }
            else if (!in_member) return GZ_E_HEADER;
            const uint64_t len = g.o1 - g.o0;
            mcrc = inf_crc_shift(mcrc, len) ^ seg_crc[s];
            msize += len;
            if (g.flags & GZ_SEG_TRAIL) {
                if (mcrc != g.crc || (uint32_t)msize != g.isize) {
                    if (bad_off) { *bad_off = R0; for (const GzLink &k : links) if (s >= k.seg0) *bad_off = R0 + (k.start >> 3); }
                    return GZ_E_CRC;
                }
                in_member = false; ++st.members;
            }
        }
        if (rec && !rec->round(dev, GzRound{R0, text_base, links.data(), (uint32_t)links.size(), segs.data(), seg_crc.data(), in0})) return GZ_RUN_DEVICE;
        text_base += out_bytes;
        pend = bytes; pend_n = out_bytes;
        if (done) return !flush() ? (int)GZ_RUN_DEVICE : in_member ? (int)INF_E_INPUT : (int)GZ_RUN_OK;
        const uint64_t next = R0 * 8 + expect;
        if (next <= pos) return GZ_RUN_TOO_MANY;                 // (no progress: cannot happen with a nonempty chain)
        pos = next;
        if (pos >= 8 * n) return !flush() ? (int)GZ_RUN_DEVICE : in_member ? (int)INF_E_INPUT : (int)GZ_RUN_OK;
    }
}
