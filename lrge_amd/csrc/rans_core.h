// rans_core.h -- the rANS 4x8 / rANS Nx16 block decode of the CRAM base blocks, shared by the device (k_cram.h; hipcc) and the host
// twin (cram_twin.cpp; g++): DESIGN section 22.  One wavefront decodes one block.  Lanes 0..N-1 hold the N interleaved states; at
// every step the lanes that must renormalise rank themselves with one ballot and take consecutive input bytes (4x8: up to two a
// state) or 16-bit words (Nx16) in lane order, which is the order the format defines.  The stream head -- order, N, shift, sizes,
// PACK map, frequency tables, RLE metadata -- was parsed on the host (cram_round.h) into a RansBlk plus table words; here are the
// symbol steps, the end-state rule and the RLE / PACK expansions behind them.
//
// The code is written once over an `Env`: lanes [lane0(), lane1()) of the 64 run in this thread (the device: its own lane; the
// twin: all 64, phase by phase), NV per-lane values live in it, ballot() and excl_scan() join the lanes, sync() orders the block's
// stores to global memory before its later loads.  Every load from the compressed bytes is bounded by the block's in_len and every
// store by the lengths of the descriptor: a stream that asks for more is a status, never an access outside.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RANS_HD __host__ __device__ __forceinline__
#else
#define RANS_HD static inline
#endif

enum {
    RANS_OK = 0,
    RANS_E_EXHAUSTED = 1,      // the states or a renormalisation need bytes behind the block's end
    RANS_E_STATE = 2,          // a state starts below the coder's lower bound
    RANS_E_END = 3,            // rANS Nx16: a state does not end at 1 << 15
    RANS_E_NO_TABLE = 4,       // an order-1 context without a table (or a slot no symbol owns)
    RANS_E_RUNS = 5,           // RLE: runs beyond the data, not adding up to it, or more run symbols than run lengths
    RANS_E_HEAD = 16,          // (host) the stream head was refused before any launch: lrge_hip_last_error names the reason
};

#define RANS_LDS_U16 24576u    // the model's room in LDS, in 16-bit words (48 KiB); a larger one is searched in global memory
#define RANS_NO_CTX 0xFFFFu

#define RANS_X_RLE 1u
#define RANS_X_PACK 2u

// one block.  Offsets: in_off into the round's compressed bytes, out_off into the dense output, tmp_off / tmp2_off into the round's
// scratch, tab_off into the round's table words (alphabet[A], then the rows of A frequencies: 1 row, order 1: A rows, row r the
// context alphabet[r]; a row of zeros: no table; a model above RANS_LDS_U16 words comes with its rows already cumulative), aux_off into the round's bytes (256 run-symbol flags, then the 16-byte PACK map),
// runs_off into the round's run lengths
struct RansBlk {
    uint64_t in_off, out_off, tmp_off, tmp2_off;
    uint32_t in_len;           // bytes from in_off to the block's end: the states, then the renormalisation bytes
    uint32_t n_sym;            // symbols to decode (codec 0: bytes to copy)
    uint32_t out_len;          // the block's raw size
    uint32_t packed_len;       // bytes behind the RLE expansion (= in front of the PACK expansion)
    uint32_t tab_off, aux_off, runs_off, n_runs;
    uint16_t A, ctx0;          // alphabet size; order 1: the row of symbol 0, the first context (RANS_NO_CTX: it has none)
    uint8_t codec;             // 0: stored bytes, 4: rANS 4x8, 5: rANS Nx16
    uint8_t order, N, shift;
    uint8_t xform;             // RANS_X_RLE | RANS_X_PACK
    uint8_t per;               // PACK: symbols per byte, 8 / 4 / 2, or 0: a single symbol, no data at all
    uint8_t pad[2];
};

RANS_HD uint32_t rans_popc64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(v);
#else
    return (uint32_t)__builtin_popcountll(v);
#endif
}
RANS_HD uint32_t rans_below(uint64_t mask, uint32_t lane) { return rans_popc64(mask & (((uint64_t)1 << lane) - 1)); }

// slot m of a row of A inclusive cumulative frequencies: the symbol's index, its frequency and its start, by a binary search for the
// first entry above m (an entry of frequency 0 repeats the one in front of it and is never that).  false: no symbol owns m
RANS_HD bool rans_find_cum(const uint16_t *row, uint32_t A, uint32_t m, uint32_t *j, uint32_t *f, uint32_t *c) {
    uint32_t lo = 0, hi = A;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (row[mid] > m) hi = mid; else lo = mid + 1;
    }
    if (lo == A) return false;
    const uint32_t start = lo ? row[lo - 1] : 0u;
    *j = lo; *f = row[lo] - start; *c = start;
    return true;
}

// the model's words: the alphabet and the rows
RANS_HD uint32_t rans_model_words(const RansBlk &b) { return (uint32_t)b.A * (1u + (b.order ? (uint32_t)b.A : 1u)); }

// alphabet and rows from the table words `src` into LDS `dst`, the rows as inclusive cumulative frequencies: a row a lane
template <class Env> RANS_HD void rans_model_load(Env &env, const RansBlk &b, const uint16_t *src, uint16_t *dst) {
    const uint32_t A = b.A, rows = b.order ? A : 1u;
    for (uint32_t l = env.lane0(); l < env.lane1(); ++l) {
        for (uint32_t i = l; i < A; i += 64) dst[i] = src[i];
        for (uint32_t r = l; r < rows; r += 64) {
            uint32_t x = 0;
            for (uint32_t i = 0; i < A; ++i) { x += src[A + r * A + i]; dst[A + r * A + i] = (uint16_t)x; }
        }
    }
    env.sync();
}

// the entropy decode of block b: n_sym symbols to dst.  model: alphabet + rows of inclusive cumulative frequencies
template <class Env> RANS_HD uint32_t rans_decode_block(Env &env, const uint8_t *in, const RansBlk &b, const uint16_t *model, uint8_t *dst) {
    const uint32_t N = b.N, n = b.n_sym, A = b.A, shift = b.shift, mask = (1u << shift) - 1, low = b.codec == 4 ? 1u << 23 : 1u << 15;
    const uint32_t l0 = env.lane0(), l1 = env.lane1();
    if (4 * N > b.in_len) return RANS_E_EXHAUSTED;
    const uint8_t *p = in + b.in_off;
    const uint16_t *alpha = model, *rows = model + A;
    uint32_t R[Env::NV], last[Env::NV], idx[Env::NV];
    bool f[Env::NV], g[Env::NV];
    const uint32_t q = b.order ? n / N : 0;
    const uint32_t steps = b.order ? q + (n - q * N) : (n + N - 1) / N;
    for (uint32_t l = l0; l < l1; ++l) {
        const uint32_t k = l - l0;
        R[k] = l < N ? (uint32_t)p[4 * l] | (uint32_t)p[4 * l + 1] << 8 | (uint32_t)p[4 * l + 2] << 16 | (uint32_t)p[4 * l + 3] << 24 : low;
        f[k] = R[k] < low;
        idx[k] = b.order ? l * q : l;
        last[k] = b.ctx0;
    }
    if (env.ballot(f)) return RANS_E_STATE;
    uint32_t pos = 4 * N;
    for (uint32_t t = 0; t < steps; ++t) {
        for (uint32_t l = l0; l < l1; ++l) {
            const uint32_t k = l - l0;
            const bool act = l < N && (b.order ? (t < q || l == N - 1) : idx[k] < n);
            f[k] = false; g[k] = act;
            if (!act) continue;
            const uint32_t m = R[k] & mask, row = b.order ? last[k] : 0;
            uint32_t j = 0, fr = 0, c = 0;
            if (row >= A || !rans_find_cum(rows + row * A, A, m, &j, &fr, &c)) { f[k] = true; continue; }
            dst[idx[k]] = (uint8_t)alpha[j];
            idx[k] += b.order ? 1 : N;
            R[k] = fr * (R[k] >> shift) + m - c;
            last[k] = j;
        }
        if (env.ballot(f)) return RANS_E_NO_TABLE;
        if (b.codec == 4) {                   // up to two bytes a state: a state's bytes are consecutive
            for (uint32_t l = l0; l < l1; ++l) { const uint32_t k = l - l0; f[k] = g[k] && R[k] < low; g[k] = g[k] && R[k] < (1u << 15); }
            const uint64_t m1 = env.ballot(f), m2 = env.ballot(g);
            const uint32_t total = rans_popc64(m1) + rans_popc64(m2);
            if (pos + total > b.in_len) return RANS_E_EXHAUSTED;
            for (uint32_t l = l0; l < l1; ++l) {
                const uint32_t k = l - l0, at = pos + rans_below(m1, l) + rans_below(m2, l);
                if (f[k]) R[k] = R[k] << 8 | p[at];
                if (g[k]) R[k] = R[k] << 8 | p[at + 1];
            }
            pos += total;
        } else {                              // one 16-bit word a state
            for (uint32_t l = l0; l < l1; ++l) { const uint32_t k = l - l0; f[k] = g[k] && R[k] < low; }
            const uint64_t m1 = env.ballot(f);
            const uint32_t total = 2 * rans_popc64(m1);
            if (pos + total > b.in_len) return RANS_E_EXHAUSTED;
            for (uint32_t l = l0; l < l1; ++l) {
                const uint32_t k = l - l0, at = pos + 2 * rans_below(m1, l);
                if (f[k]) R[k] = R[k] << 16 | (uint32_t)p[at] | (uint32_t)p[at + 1] << 8;
            }
            pos += total;
        }
    }
    if (b.codec == 5) {                       // the integrity rule: a decoder that took every symbol back ends where the encoder began
        for (uint32_t l = l0; l < l1; ++l) f[l - l0] = l < N && R[l - l0] != low;
        if (env.ballot(f)) return RANS_E_END;
    }
    return RANS_OK;
}

// RLE: the n literals of src to dst, a literal of a run symbol (flag[literal]) 1 + runs[its rank among such literals] times; the
// result must be exactly `want` bytes.  64 literals a step, their places by a scan of the copies
template <class Env> RANS_HD uint32_t rans_expand_rle(Env &env, const uint8_t *src, uint32_t n, const uint8_t *flag, const uint32_t *runs, uint32_t n_runs, uint8_t *dst,
                                                      uint32_t want) {
    const uint32_t l0 = env.lane0(), l1 = env.lane1();
    uint64_t done = 0, copies[Env::NV], at[Env::NV];
    uint32_t used = 0;
    bool f[Env::NV], g[Env::NV];
    for (uint32_t base = 0; base < n; base += 64) {
        for (uint32_t l = l0; l < l1; ++l) { const uint32_t k = l - l0, i = base + l; f[k] = i < n && flag[src[i]]; }
        const uint64_t mr = env.ballot(f);
        for (uint32_t l = l0; l < l1; ++l) {
            const uint32_t k = l - l0, i = base + l, r = used + rans_below(mr, l);
            g[k] = f[k] && r >= n_runs;
            copies[k] = i < n ? (uint64_t)1 + (f[k] && !g[k] ? runs[r] : 0u) : 0;
        }
        if (env.ballot(g)) return RANS_E_RUNS;
        used += rans_popc64(mr);
        const uint64_t total = env.excl_scan(copies, at);
        if (done + total > want) return RANS_E_RUNS;
        for (uint32_t l = l0; l < l1; ++l) {
            const uint32_t k = l - l0, i = base + l;
            if (i >= n) continue;
            const uint8_t v = src[i];
            uint8_t *d = dst + done + at[k];
            for (uint64_t c = 0; c < copies[k]; ++c) d[c] = v;
        }
        done += total;
    }
    return done == want ? (uint32_t)RANS_OK : (uint32_t)RANS_E_RUNS;
}

// PACK: n_out symbols from the packed bytes of src, `per` of them a byte, low bits first, through the 16-byte map; per == 0: one
// symbol, no data
template <class Env> RANS_HD void rans_expand_pack(Env &env, const uint8_t *src, uint32_t per, const uint8_t *pmap, uint8_t *dst, uint32_t n_out) {
    const uint32_t l0 = env.lane0(), l1 = env.lane1();
    if (per == 0) {
        for (uint32_t l = l0; l < l1; ++l) for (uint32_t i = l; i < n_out; i += 64) dst[i] = pmap[0];
        return;
    }
    const uint32_t bits = 8 / per, msk = (1u << bits) - 1, n_in = (n_out + per - 1) / per;
    for (uint32_t l = l0; l < l1; ++l)
        for (uint32_t i = l; i < n_in; i += 64) {
            const uint32_t v = src[i];
            for (uint32_t k = 0; k < per && i * per + k < n_out; ++k) dst[i * per + k] = pmap[(v >> (k * bits)) & msk];
        }
}

// one block, whole: the entropy decode (or the copy of stored bytes) and the expansions behind it.  lds: RANS_LDS_U16 words (the
// model goes there when it fits); tabs / aux / runs / tmp: the round's
template <class Env> RANS_HD uint32_t rans_block(Env &env, const uint8_t *in, const RansBlk &b, const uint16_t *tabs, const uint8_t *aux, const uint32_t *runs, uint16_t *lds,
                                                 uint32_t lds_words, uint8_t *tmp, uint8_t *out) {
    uint8_t *final = out + b.out_off;
    uint8_t *dst = b.xform ? tmp + b.tmp_off : final;
    if (b.codec == 0) {
        if (b.n_sym > b.in_len) return RANS_E_EXHAUSTED;
        for (uint32_t l = env.lane0(); l < env.lane1(); ++l) for (uint32_t i = l; i < b.n_sym; i += 64) dst[i] = in[b.in_off + i];
    } else if (b.n_sym) {
        const uint16_t *model = tabs + b.tab_off;
        if (rans_model_words(b) <= lds_words) { rans_model_load(env, b, model, lds); model = lds; }      // (else the host left its rows cumulative)
        const uint32_t st = rans_decode_block(env, in, b, model, dst);
        if (st) return st;
    }
    if (!b.xform) return RANS_OK;
    env.sync();
    const uint8_t *src = dst;
    uint32_t n = b.n_sym;
    if (b.xform & RANS_X_RLE) {
        uint8_t *d = (b.xform & RANS_X_PACK) ? tmp + b.tmp2_off : final;
        const uint32_t st = rans_expand_rle(env, src, n, aux + b.aux_off, runs + b.runs_off, b.n_runs, d, b.packed_len);
        if (st) return st;
        env.sync();
        src = d; n = b.packed_len;
    }
    if (b.xform & RANS_X_PACK) rans_expand_pack(env, src, b.per, aux + b.aux_off + 256, final, b.out_len);
    return RANS_OK;
}
