// cram_round.h -- the host side of the CRAM device ingest, shared by the library (host_cram.inl; hipcc) and the host twin
// (cram_twin.cpp; g++): DESIGN section 22.
//   cram_walk     the container walk: lrge::io::cram::parse_with under the WalkBases policy -- the host reader's own record loop,
//                 so names, lengths and flags are the host's one for one; no base is read, every record becomes an offset into its
//                 slice's BA block.  Whatever the walk cannot prove, and every error the host code raises, is a reason text.
//   rans_head     the head of one BA block parsed with the host reader's own table code (cram::Cursor, cram::Nx16): a RansBlk and
//                 its table words, run-symbol flags, PACK map and run lengths for the device.  A form the device does not take is
//                 an Err naming it.
//   cram_run      the rounds: the blocks whose compressed bytes fit `round_bytes` go up together with their descriptors and are
//                 decoded by one launch of the backend `Dev`, which leaves each block's bytes at its offset in the dense store.
//   cram_sampled  the sampled ingest: census, selected open, census with a map and mapped open over the same walk,
//                 heads and rounds, with a backend that decodes into a scratch and keeps the chosen reads only (at the end of this file).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "../../include/lrge_io.hpp"
#include "rans_core.h"
#include "fx_seek.h"

struct CramStats {
    uint64_t containers = 0, slices = 0, records = 0;
    uint64_t ba_raw = 0, ba_rans4x8 = 0, ba_ransnx16 = 0;      // BA blocks by method (a slice without bases has none)
    uint64_t order1_blocks = 0, global_table_blocks = 0;
    uint64_t comp_bytes = 0, raw_bytes = 0;                    // the BA blocks' bytes, compressed and not
    uint64_t rounds = 0, walk_us = 0, decode_us = 0;
};
#define CRAM_STAT_WORDS 13
static inline void cram_stats_words(const CramStats &s, uint64_t *v) {
    const uint64_t w[CRAM_STAT_WORDS] = {s.containers, s.slices, s.records, s.ba_raw, s.ba_rans4x8, s.ba_ransnx16, s.order1_blocks, s.global_table_blocks,
                                         s.comp_bytes, s.raw_bytes, s.rounds, s.walk_us, s.decode_us};
    memcpy(v, w, sizeof w);
}

static inline const char *rans_status_name(uint32_t s) {
    switch (s) {
    case RANS_OK: return "ok";
    case RANS_E_EXHAUSTED: return "compressed data exhausted";
    case RANS_E_STATE: return "a state starts below the coder's lower bound";
    case RANS_E_END: return "bad end state";
    case RANS_E_NO_TABLE: return "an order-1 context without a table";
    case RANS_E_RUNS: return "run lengths that do not fit the data";
    case RANS_E_HEAD: return "a stream head the device does not take";
    default: return "unknown status";
    }
}

static inline uint64_t cram_now_us() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- the walk ----
struct CramWalk {
    lrge::io::cram::WalkBases w;
    std::string names;                      // the identifiers, back to back
    std::vector<uint64_t> name_off;         // [n + 1]
    std::vector<uint64_t> ba_out;           // [slices + 1]: where a slice's bases start in the dense store
};

// which identifiers a walk keeps (the sampled ingest): those of the ordinals sel[0, k), strictly ascending --
// none for k = 0, the census -- so the host memory for names scales with the sample.  names / name_off then hold the kept ones only
struct CramNames { const uint32_t *sel; uint64_t k; };

// false: `why` says what the device path does not prove (or what the host reader reports).  keep == nullptr: every identifier
static inline bool cram_walk(const uint8_t *d, uint64_t n, CramWalk &cw, std::string &why, const CramNames *keep = nullptr) {
    using namespace lrge::io;
    if (detect_compression_format(std::string((const char *)d, (size_t)(n < 8 ? n : 8))) != CompressionFormat::None) { why = "CRAM behind a compression format"; return false; }
    cw.name_off.assign(1, 0);
    uint64_t ord = 0, at = 0;
    try {
        cram::parse_with(d, (size_t)n, [&](const std::string &name, const std::string &) {
            const uint64_t i = ord++;
            if (keep) { if (at >= keep->k || keep->sel[at] != i) return; ++at; }
            cw.names += name; cw.name_off.push_back(cw.names.size());
        }, MAPPED_MSG, cw.w);
    } catch (const std::exception &e) { why = e.what(); return false; }
    cw.ba_out.assign(1, 0);
    for (const auto &b : cw.w.ba) cw.ba_out.push_back(cw.ba_out.back() + (uint64_t)b.raw_size);
    return true;
}

// ---- the stream heads ----
// what a round carries beside its compressed bytes
struct RansTables {
    std::vector<uint16_t> tabs;
    std::vector<uint8_t> aux;
    std::vector<uint32_t> runs;
    void clear() { tabs.clear(); aux.clear(); runs.clear(); }
};

namespace cram_detail {
using lrge::io::cram::Cursor;
using lrge::io::cram::Err;
using lrge::io::cram::Nx16;

// alphabet (present[256]) and rows (F[row][256], rows indexed by symbol; order 0: row 0) to the table words of block b
static inline void put_model(RansBlk &b, RansTables &t, const bool *present, const std::vector<std::vector<uint32_t>> &F) {
    std::vector<int> alpha;
    for (int j = 0; j < 256; ++j) if (present[j]) alpha.push_back(j);
    b.A = (uint16_t)alpha.size();
    b.ctx0 = present[0] ? 0 : RANS_NO_CTX;                      // (symbol 0 is the alphabet's first when it is there)
    b.tab_off = (uint32_t)t.tabs.size();
    for (int j : alpha) t.tabs.push_back((uint16_t)j);
    if (!b.order) { for (int j : alpha) t.tabs.push_back((uint16_t)F[0][(size_t)j]); return; }
    for (int i : alpha) for (int j : alpha) t.tabs.push_back(F[(size_t)i].empty() ? (uint16_t)0 : (uint16_t)F[(size_t)i][(size_t)j]);
}

// rANS 4x8: the frequencies of one table as rans4x8_decode's read_table reads them
static inline void table_4x8(Cursor &c, std::vector<uint32_t> &F) {
    F.assign(256, 0);
    bool seen[256] = {false};
    unsigned x = 0, rle = 0, j = c.u8();
    do {
        unsigned f = c.u8();
        if (f >= 128) f = ((f & 127) << 8) | c.u8();
        if (x + f > 4096) throw Err("CRAM: rANS frequencies exceed 4096");
        if (seen[j]) throw Err("CRAM: a rANS 4x8 table lists a symbol twice (not taken by the device)");
        seen[j] = true; F[j] = f; x += f;
        if (!rle && c.left() && j + 1 == *c.p) { j = c.u8(); rle = c.u8(); }
        else if (rle) { --rle; ++j; if (j > 255) throw Err("CRAM: rANS symbol run past 255"); }
        else j = c.u8();
    } while (j);
    if (x != 4096) throw Err("CRAM: a rANS 4x8 table whose frequencies sum to " + std::to_string(x) + ", not 4096 (a short table: not taken by the device)");
}

static inline void head_4x8(Cursor &c, const uint8_t *base, int64_t raw_size, RansBlk &b, RansTables &t) {
    const unsigned order = c.u8();
    const uint32_t csz = c.u32le(), usz = c.u32le();
    if (order > 1) throw Err("CRAM: rANS order " + std::to_string(order));
    if (c.left() < csz) throw Err("CRAM: truncated rANS stream");
    if ((uint64_t)usz > ((uint64_t)c.left() + 16) * 24000) throw Err("CRAM: rANS size field exceeds what the stream can hold");
    if ((int64_t)usz != raw_size) throw Err("CRAM: block size mismatch after decompression");
    b.codec = 4; b.order = (uint8_t)order; b.N = 4; b.shift = 12; b.n_sym = usz;
    if (usz == 0) { b.codec = 0; return; }
    bool present[256] = {false};
    std::vector<std::vector<uint32_t>> F(256);
    if (order == 0) {
        table_4x8(c, F[0]);
        for (int j = 0; j < 256; ++j) present[j] = F[0][(size_t)j] != 0;
    } else {
        unsigned rle = 0, i = c.u8();
        do {
            if (!F[i].empty()) throw Err("CRAM: a rANS 4x8 stream lists a context twice (not taken by the device)");
            table_4x8(c, F[i]);
            present[i] = true;
            for (int j = 0; j < 256; ++j) if (F[i][(size_t)j]) present[j] = true;
            if (!rle && c.left() && i + 1 == *c.p) { i = c.u8(); rle = c.u8(); }
            else if (rle) { --rle; ++i; if (i > 255) throw Err("CRAM: rANS context run past 255"); }
            else i = c.u8();
        } while (i);
    }
    put_model(b, t, present, F);
    b.in_off = (uint64_t)(c.p - base); b.in_len = (uint32_t)c.left();
}

// the frequencies Nx16::finish leaves for a row: scaled up to 1 << shift
static inline void finish_row(uint32_t *Fin, unsigned shift, std::vector<uint32_t> &F) {
    std::unique_ptr<Nx16::Tab> tab(new Nx16::Tab());
    Nx16::finish(*tab, Fin, shift);
    F.assign(256, 0);
    for (int j = 0; j < 256; ++j) F[(size_t)j] = tab->F[j];
}

// the body of an entropy-coded Nx16 stream of `len` symbols, as Nx16::decode0 / decode1 read it, up to its states
static inline void body_nx16(Cursor &c, const uint8_t *base, uint32_t len, bool order1, int N, RansBlk &b, RansTables &t, std::string &keep) {
    b.codec = 5; b.order = order1; b.N = (uint8_t)N; b.shift = 12; b.n_sym = len;
    if (!len) { b.codec = 0; return; }
    bool A[256];
    std::vector<std::vector<uint32_t>> F(256);
    if (!order1) {
        Nx16::alphabet(c, A);
        uint32_t Fin[256] = {0};
        for (int j = 0; j < 256; ++j) if (A[j]) Fin[j] = Nx16::u7(c);
        finish_row(Fin, 12, F[0]);
    } else {
        const unsigned comp = c.u8(), shift = comp >> 4;
        if (shift < 1 || shift > 12) throw Err("CRAM: rANS Nx16 order-1 table of " + std::to_string(shift) + " bits");
        b.shift = (uint8_t)shift;
        auto read_tabs = [&](Cursor &tc) {
            Nx16::alphabet(tc, A);
            for (int i = 0; i < 256; ++i) {
                if (!A[i]) continue;
                uint32_t Fin[256] = {0};
                unsigned run = 0;
                for (int j = 0; j < 256; ++j) {
                    if (!A[j]) continue;
                    if (run) { --run; continue; }
                    Fin[j] = Nx16::u7(tc);
                    if (!Fin[j]) run = tc.u8();
                }
                bool any = false;
                for (int j = 0; j < 256; ++j) any |= Fin[j] != 0;
                if (any) finish_row(Fin, shift, F[(size_t)i]);
            }
        };
        if (comp & 1) {                                               // the table went through the order-0 coder: decoded here, on the host
            const uint32_t ulen = Nx16::u7(c), clen = Nx16::u7(c);
            if (c.left() < clen) throw Err("CRAM: truncated rANS Nx16 table");
            if ((uint64_t)ulen > ((uint64_t)clen + 16) * 24000) throw Err("CRAM: rANS Nx16 table size exceeds what its bytes can hold");
            Cursor sub(c.p, clen); c.skip(clen);
            keep = Nx16::decode0(sub, ulen, 4);
            Cursor tc((const unsigned char *)keep.data(), keep.size());
            read_tabs(tc);
        } else read_tabs(c);
    }
    put_model(b, t, A, F);
    b.in_off = (uint64_t)(c.p - base); b.in_len = (uint32_t)c.left();
}

static inline void head_nx16(Cursor &c, const uint8_t *base, int64_t raw_size, RansBlk &b, RansTables &t) {
    const unsigned flags = c.u8();
    size_t len;
    const size_t known = (size_t)raw_size;
    if (flags & 0x10) len = known;
    else { len = Nx16::u7(c); if (len != known) throw Err("CRAM: rANS Nx16 stream size differs from its container's"); }
    const int N = (flags & 0x04) ? 32 : 4;
    if (flags & 0x08) throw Err("CRAM: a BA block in rANS Nx16 STRIPE form (for integers, not bases: not taken by the device)");
    if ((uint64_t)len > ((uint64_t)c.left() + 16) * 24000ull * 8ull * 255ull) throw Err("CRAM: rANS Nx16 size field exceeds what the stream can hold");
    const size_t final_len = len;
    b.aux_off = (uint32_t)t.aux.size();
    t.aux.resize(t.aux.size() + 256 + 16, 0);
    unsigned per = 1;
    if (flags & 0x80) {
        unsigned n = c.u8();
        if (n == 0) n = 256;
        if (n <= 1) per = 0; else if (n <= 2) per = 8; else if (n <= 4) per = 4; else if (n <= 16) per = 2; else per = 1;
        if (n <= 16) for (unsigned i = 0; i < n; ++i) t.aux[b.aux_off + 256 + i] = (uint8_t)c.u8();
        len = Nx16::u7(c);
        if (per >= 2 && len != (final_len + per - 1) / per) throw Err("CRAM: rANS Nx16 packed length does not match");
        if (per == 1 && len != final_len) throw Err("CRAM: rANS Nx16 packed length does not match");
        if (per != 1) { b.xform |= RANS_X_PACK; b.per = (uint8_t)per; }
    }
    const size_t packed_len = len;
    b.packed_len = (uint32_t)packed_len;
    if (flags & 0x40) {
        std::string rmeta;
        const uint32_t umeta = Nx16::u7(c);
        len = Nx16::u7(c);
        if (umeta & 1) { const size_t n = umeta >> 1; if (c.left() < n) throw Err("CRAM: truncated rANS Nx16 run lengths"); rmeta.assign((const char *)c.p, n); c.skip(n); }
        else {
            const uint32_t cmeta = Nx16::u7(c);
            if (c.left() < cmeta) throw Err("CRAM: truncated rANS Nx16 run lengths");
            if ((uint64_t)(umeta >> 1) > ((uint64_t)cmeta + 16) * 24000) throw Err("CRAM: rANS Nx16 run-length size exceeds what its bytes can hold");
            Cursor sub(c.p, cmeta); c.skip(cmeta);
            rmeta = Nx16::decode0(sub, umeta >> 1, 4);
        }
        if (len > packed_len) throw Err("CRAM: rANS Nx16 literals exceed the data");
        // the run symbols as 256 flags, the run lengths as plain words: as many as the metadata holds whole
        Cursor m((const unsigned char *)rmeta.data(), rmeta.size());
        unsigned n = m.u8(); if (n == 0) n = 256;
        for (unsigned i = 0; i < n; ++i) t.aux[b.aux_off + m.u8()] = 1;
        b.runs_off = (uint32_t)t.runs.size();
        while (m.left()) {
            uint32_t v = 0; int k = 0; bool whole = false;
            while (m.left() && k < 5) { const unsigned x = m.u8(); ++k; v = (v << 7) | (x & 0x7f); if (!(x & 0x80)) { whole = true; break; } }
            if (!whole) break;
            t.runs.push_back(v);
        }
        b.n_runs = (uint32_t)t.runs.size() - b.runs_off;
        b.xform |= RANS_X_RLE;
    }
    if ((uint64_t)len > ((uint64_t)c.left() + 16) * 24000) throw Err("CRAM: rANS Nx16 size field exceeds what the stream can hold");
    if (len >> 31) throw Err("CRAM: a rANS Nx16 stream of 2^31 symbols or more");
    if (flags & 0x20) {
        if (c.left() < len) throw Err("CRAM: truncated rANS Nx16 stream");
        b.codec = 0; b.n_sym = (uint32_t)len; b.in_off = (uint64_t)(c.p - base); b.in_len = (uint32_t)len;
        return;
    }
    std::string keep;
    body_nx16(c, base, (uint32_t)len, (flags & 0x01) != 0, N, b, t, keep);
}
}  // namespace cram_detail

// The head of one block of method `method` (0 raw, 4 rANS 4x8, 5 rANS Nx16): d[0, n) its bytes, raw_size its decompressed size.
// in_off is left relative to d.  Throws lrge::io::cram::Err for what the host reader reports and for what the device does not take.
static inline void rans_head(int method, const uint8_t *d, size_t n, int64_t raw_size, RansBlk &b, RansTables &t) {
    using namespace cram_detail;
    memset(&b, 0, sizeof b);
    b.out_len = (uint32_t)raw_size; b.packed_len = (uint32_t)raw_size;
    if (raw_size < 0 || raw_size >> 31) throw Err("CRAM: a BA block of 2^31 bytes or more");
    Cursor c(d, n);
    switch (method) {
    case 0:
        if ((int64_t)n != raw_size) throw Err("CRAM: block size mismatch after decompression");
        b.codec = 0; b.n_sym = (uint32_t)n; b.in_off = 0; b.in_len = (uint32_t)n;
        return;
    case 4: head_4x8(c, d, raw_size, b, t); return;
    case 5: head_nx16(c, d, raw_size, b, t); return;
    case 1: throw Err("CRAM: a BA block in gzip (not taken by the device)");
    case 2: throw Err("CRAM: a BA block in bzip2 (not taken by the device)");
    case 3: throw Err("CRAM: a BA block in lzma (not taken by the device)");
    case 6: throw Err("CRAM: a BA block in the adaptive arithmetic coder (arith: not taken by the device)");
    case 7: throw Err("CRAM: a BA block in fqzcomp (not taken by the device)");
    case 8: throw Err("CRAM: a BA block in the name tokeniser (tok3: not taken by the device)");
    default: throw Err("CRAM: unknown block compression method " + std::to_string(method));
    }
}

// ---- the rounds ----
struct RansStream { const uint8_t *d; size_t n; int method; int64_t raw_size; uint64_t out_off; };

// Dev: bool round(const uint8_t *in, size_t in_bytes, const RansBlk *blk, uint32_t m, const RansTables &t, uint64_t tmp_bytes, uint32_t *status)
//      -- the m blocks decoded into the dense store, a status word each; false: the backend failed (its own error)
// status[i] (optional): per stream, RANS_E_HEAD where the head was refused (`why` keeps the first reason).  Returns the index of the
// first stream whose status is not OK plus one, 0: all decoded, -1: the backend failed.  stop_at_first: a refused head ends the call
template <class Dev>
static inline int64_t cram_run(Dev &dev, const std::vector<RansStream> &s, uint64_t round_bytes, bool stop_at_first, CramStats &st, uint32_t *status, std::string &why) {
    int64_t first_bad = 0;
    std::vector<uint8_t> in;
    std::vector<RansBlk> blk;
    std::vector<size_t> who;
    std::vector<uint32_t> rst;
    RansTables t;
    size_t i = 0;
    while (i < s.size()) {
        in.clear(); blk.clear(); who.clear(); t.clear();
        uint64_t tmp = 0;
        size_t j = i;
        for (; j < s.size() && (blk.empty() || in.size() + s[j].n <= round_bytes); ++j) {
            RansBlk b;
            const size_t tabs0 = t.tabs.size(), aux0 = t.aux.size(), runs0 = t.runs.size();
            try { rans_head(s[j].method, s[j].d, s[j].n, s[j].raw_size, b, t); }
            catch (const std::exception &e) {
                t.tabs.resize(tabs0); t.aux.resize(aux0); t.runs.resize(runs0);
                if (why.empty()) why = e.what();
                if (status) status[j] = RANS_E_HEAD;
                if (!first_bad) first_bad = (int64_t)j + 1;
                if (stop_at_first) return first_bad;
                continue;
            }
            if (s[j].method == 0) ++st.ba_raw; else if (s[j].method == 4) ++st.ba_rans4x8; else ++st.ba_ransnx16;
            if (b.codec && b.order) ++st.order1_blocks;
            if (b.codec && b.n_sym && rans_model_words(b) > RANS_LDS_U16) {       // searched where it lies, in global memory: the rows go up cumulative
                ++st.global_table_blocks;
                uint16_t *rows = t.tabs.data() + b.tab_off + b.A;
                for (uint32_t r = 0; r < (b.order ? (uint32_t)b.A : 1u); ++r) { uint32_t x = 0; for (uint32_t k = 0; k < b.A; ++k) { x += rows[r * b.A + k]; rows[r * b.A + k] = (uint16_t)x; } }
            }
            st.comp_bytes += s[j].n; st.raw_bytes += (uint64_t)s[j].raw_size;
            b.in_off += in.size(); b.out_off = s[j].out_off;
            in.insert(in.end(), s[j].d, s[j].d + s[j].n);
            in.resize((in.size() + 3) & ~(size_t)3, 0);
            if (b.xform) {
                b.tmp_off = tmp; tmp += ((uint64_t)b.n_sym + 3) & ~(uint64_t)3;
                if (b.xform == (RANS_X_RLE | RANS_X_PACK)) { b.tmp2_off = tmp; tmp += ((uint64_t)b.packed_len + 3) & ~(uint64_t)3; }
            }
            blk.push_back(b); who.push_back(j);
        }
        i = j;
        if (blk.empty()) continue;
        ++st.rounds;
        rst.assign(blk.size(), 0);
        const uint64_t t0 = cram_now_us();
        if (!dev.round(in.data(), in.size(), blk.data(), (uint32_t)blk.size(), t, tmp, rst.data())) return -1;
        st.decode_us += cram_now_us() - t0;
        for (size_t k = 0; k < blk.size(); ++k) {
            if (status) status[who[k]] = rst[k];
            if (rst[k] && (!first_bad || (int64_t)who[k] + 1 < first_bad)) {
                first_bad = (int64_t)who[k] + 1;
                if (why.empty() || stop_at_first) why = std::string("CRAM: BA block ") + std::to_string(who[k]) + ": " + rans_status_name(rst[k]);
            }
        }
        if (first_bad && stop_at_first) return first_bad;
    }
    return first_bad;
}

// the streams of a walk: one per slice that has a BA block
static inline std::vector<RansStream> cram_streams(const CramWalk &cw) {
    std::vector<RansStream> s;
    for (size_t k = 0; k < cw.w.ba.size(); ++k) {
        const auto &b = cw.w.ba[k];
        if (b.data || b.raw_size) s.push_back(RansStream{b.data, b.size, b.method, b.raw_size, cw.ba_out[k]});
    }
    return s;
}

// ---- the sampled ingest: the same walk, heads and rounds with another sink ----
// A second backend decodes a round into a scratch block of the round's raw size and copies the chosen reads' ranges from there to
// a dense store of exactly the chosen bases.  What is shared by the device (host_cram.inl) and the twin (cram_twin.cpp) is here: the
// plan of a selection, the descriptors rebased to the scratch, the copy table of a round, the round size that fits the budget, the
// seek map of kind FX_SEEK_CRAM and the four calls' common course (cram_sampled).
struct CramCopy { uint64_t src, dst, len; };        // (the layout of FxRunCopy, k_fastx.h: k_fx_runs takes the table as it is)

// sel[0, k): strictly ascending, every ordinal below the walk's records (the caller has checked both)
struct CramKeepPlan {
    std::vector<uint64_t> dst;            // [k + 1]: where chosen read j lies in the dense store; dst[k]: the chosen bases
    std::vector<uint64_t> first;          // [slices + 1]: the chosen reads of slice s are j in [first[s], first[s + 1])
    std::vector<RansStream> streams;      // the BA blocks the pass decodes, in file order
    std::vector<uint32_t> slice_of;       // ... and the slice of each
    uint64_t runs = 0;                    // stretches of consecutive slices among them, as the planner of fx_seek.h merges runs
};

// touched_only: the mapped open -- only the BA blocks of slices that hold a chosen read with bases; else every BA block of the file
static inline void cram_keep_plan(const CramWalk &cw, const uint32_t *sel, uint64_t k, bool touched_only, CramKeepPlan &p) {
    const size_t n_slices = cw.w.ba.size();
    p = CramKeepPlan();
    p.dst.assign(1, 0);
    p.first.assign(n_slices + 1, 0);
    std::vector<uint8_t> touched(n_slices, 0);
    for (uint64_t j = 0; j < k; ++j) {
        const auto &r = cw.w.recs[sel[j]];
        p.dst.push_back(p.dst.back() + r.len);
        ++p.first[r.slice + 1];
        if (r.len) touched[r.slice] = 1;
    }
    for (size_t s = 0; s < n_slices; ++s) p.first[s + 1] += p.first[s];
    uint32_t prev = 0;
    for (size_t s = 0; s < n_slices; ++s) {
        const auto &b = cw.w.ba[s];
        if (!(b.data || b.raw_size) || (touched_only && !touched[s])) continue;
        if (p.streams.empty() || prev + 1 != (uint32_t)s) ++p.runs;
        p.streams.push_back(RansStream{b.data, b.size, b.method, b.raw_size, cw.ba_out[s]});
        p.slice_of.push_back((uint32_t)s);
        prev = (uint32_t)s;
    }
}

// the m blocks of a round (copies of the descriptors) placed back to back in a scratch of the returned size: scr[a] is where block a starts
static inline uint64_t cram_rebase(RansBlk *b, uint32_t m, uint64_t *scr) {
    uint64_t o = 0;
    for (uint32_t a = 0; a < m; ++a) { scr[a] = o; b[a].out_off = o; o += b[a].out_len; }
    return o;
}

// the copies of a round whose blocks are streams [at, at + m) of the plan: every chosen read with bases, scratch to store; neighbours
// on both sides are one copy
static inline void cram_round_copies(const CramWalk &cw, const CramKeepPlan &p, const uint32_t *sel, size_t at, uint32_t m, const uint64_t *scr, std::vector<CramCopy> &out) {
    out.clear();
    for (uint32_t a = 0; a < m; ++a) {
        const uint32_t s = p.slice_of[at + a];
        for (uint64_t j = p.first[s]; j < p.first[s + 1]; ++j) {
            const auto &r = cw.w.recs[sel[j]];
            if (!r.len) continue;
            const CramCopy c = {scr[a] + r.off, p.dst[j], r.len};
            if (!out.empty() && out.back().src + out.back().len == c.src && out.back().dst + out.back().len == c.dst) out.back().len += c.len;
            else out.push_back(c);
        }
    }
}

// the largest round cram_run forms over s at `round_bytes`: its compressed bytes as they go up (padded to words) plus its raw bytes
static inline uint64_t cram_largest_round(const std::vector<RansStream> &s, uint64_t round_bytes, uint64_t *raw_max = nullptr) {
    uint64_t best = 0, best_raw = 0;
    for (size_t i = 0, j; i < s.size(); i = j) {
        uint64_t in = 0, raw = 0;
        for (j = i; j < s.size() && (j == i || in + s[j].n <= round_bytes); ++j) { in = (in + s[j].n + 3) & ~(uint64_t)3; raw += (uint64_t)s[j].raw_size; }
        best = std::max(best, in + raw); best_raw = std::max(best_raw, raw);
    }
    if (raw_max) *raw_max = best_raw;
    return best;
}

// The round size of a pass that has `room` bytes beside its store: option CRAM_ROUND_BYTES where its largest round fits, else halved
// until it does -- at 1 every block is a round of its own.  0: a single block does not fit
static inline uint64_t cram_fit_round(const std::vector<RansStream> &s, uint64_t round_bytes, uint64_t room) {
    for (uint64_t r = round_bytes;; r = r / 2) {
        if (cram_largest_round(s, r) <= room) return r;
        if (r <= 1) return 0;
    }
}

// the seek map of a CRAM (fx_seek.h, kind FX_SEEK_CRAM): one point per slice in which a record starts -- that record's ordinal, the
// slice's base offset, the file offset of its BA block (0: it has none); n_blocks: the slices, text_bytes: the bases
static inline void cram_seek_map(const CramWalk &cw, const uint8_t *d, uint64_t len, FxSeekMap &m) {
    m = FxSeekMap();
    m.kind = FX_SEEK_CRAM; m.fmt = cw.w.recs.empty() ? FX_FMT_EMPTY : FX_FMT_FASTA; m.stride = 0;
    m.file_len = len; m.records = cw.w.recs.size(); m.bases = m.text_bytes = cw.ba_out.back(); m.n_blocks = cw.w.ba.size();
    for (size_t i = 0; i < cw.w.recs.size(); ++i) {
        const uint32_t s = cw.w.recs[i].slice;
        if (i && cw.w.recs[i - 1].slice == s) continue;
        m.pts.push_back(FxSeekPoint{i, cw.ba_out[s], cw.w.ba[s].data ? (uint64_t)(cw.w.ba[s].data - d) : 0, 0, 0, s});
    }
}

static inline bool cram_same_points(const FxSeekMap &a, const FxSeekMap &b) {
    if (a.pts.size() != b.pts.size()) return false;
    for (size_t i = 0; i < a.pts.size(); ++i)
        if (a.pts[i].ord != b.pts[i].ord || a.pts[i].off != b.pts[i].off || a.pts[i].c_off != b.pts[i].c_off || a.pts[i].blk != b.pts[i].blk) return false;
    return true;
}

// One of the four sampled calls over file d[0, len).  sel[0, k): strictly ascending (checked by the caller); mapped: `map` is the
// map of an earlier census, and only the touched blocks are decoded; else `map` (optional) is filled.
// Sink: bool begin(const CramWalk &, const CramKeepPlan &, const uint32_t *sel, uint64_t k) -- the store of plan.dst[k] bytes; false: its own error
//       and the Dev of cram_run, whose rounds it decodes into its scratch and copies from (cram_rebase, cram_round_copies).
enum { CRAM_S_OK = 0, CRAM_S_UNPROVEN, CRAM_S_ORDINAL, CRAM_S_OTHER_INPUT, CRAM_S_MISFIT, CRAM_S_OVER_CAP, CRAM_S_BACKEND };
struct CramSampled {
    CramWalk cw;
    CramKeepPlan plan;
    CramStats st;
    uint64_t round_bytes = 0, seek[4] = {0, 0, 0, 0};
    uint32_t bad_ordinal = 0;
};
template <class Sink>
static inline int cram_sampled(Sink &sink, const uint8_t *d, uint64_t len, const uint32_t *sel, uint64_t k, bool mapped, FxSeekMap *map, uint64_t min_blocks, uint64_t round_bytes,
                               uint64_t cap, CramSampled &o, std::string &why) {
    if (mapped && (map->kind != FX_SEEK_CRAM || map->file_len != len)) return CRAM_S_OTHER_INPUT;
    const CramNames keep = {sel, k};
    const uint64_t w0 = cram_now_us();
    if (!cram_walk(d, len, o.cw, why, &keep)) return CRAM_S_UNPROVEN;
    o.st.walk_us = cram_now_us() - w0;
    o.st.containers = o.cw.w.containers; o.st.slices = o.cw.w.ba.size(); o.st.records = o.cw.w.recs.size();
    const uint64_t n = o.cw.w.recs.size();
    if (n >> 32) { why = "2^32 CRAM records or more"; return CRAM_S_UNPROVEN; }
    if (o.cw.names.size() >> 32) { why = "4 GiB of identifiers or more"; return CRAM_S_UNPROVEN; }
    if (cram_streams(o.cw).size() < min_blocks) { why = "fewer BA blocks than CRAM_MIN_BLOCKS"; return CRAM_S_UNPROVEN; }
    FxSeekMap now;
    if (mapped || map) cram_seek_map(o.cw, d, len, now);
    if (mapped && (map->records != now.records || map->bases != now.bases || map->n_blocks != now.n_blocks)) return CRAM_S_OTHER_INPUT;
    for (uint64_t j = 0; j < k; ++j) if (sel[j] >= n) { o.bad_ordinal = sel[j]; return CRAM_S_ORDINAL; }
    if (mapped && !cram_same_points(*map, now)) { why = "other slices than the map's"; return CRAM_S_MISFIT; }
    cram_keep_plan(o.cw, sel, k, mapped, o.plan);
    if (o.plan.dst.back() > cap || !(o.round_bytes = cram_fit_round(o.plan.streams, round_bytes, cap - o.plan.dst.back()))) return CRAM_S_OVER_CAP;
    if (!sink.begin(o.cw, o.plan, sel, k)) return CRAM_S_BACKEND;
    const int64_t bad = cram_run(sink, o.plan.streams, o.round_bytes, true, o.st, nullptr, why);
    if (bad < 0) return CRAM_S_BACKEND;
    if (bad) return CRAM_S_UNPROVEN;
    if (mapped) { o.seek[0] = o.plan.runs; o.seek[1] = o.st.raw_bytes; o.seek[2] = o.st.comp_bytes; o.seek[3] = o.plan.streams.size(); }
    else if (map) *map = now;
    return CRAM_S_OK;
}
