// paf_core.h -- the rules of a PAF line, written to compile for the device (hipcc: k_paf.h) as well as for
// the host twin (paf_twin.cpp; g++).  No HIP types, no snprintf.  A line is what lrge_amd/paf.py: paf_lines and lrge::paf_lines
// (include/lrge_hip.hpp) write -- mapping.rs:10-54 field order, :81-177 serialisers -- plus one line feed:
//
//   qname  [qlen qs qe strand]  tname  [tlen rs re mlen blen 0 tp:A:S cm:i: s1:i: dv:f: rl:i:]
//
// The two identifiers are copied; the 15 fields between and behind them are the FIXED part: field f's text is a literal prefix
// (it starts with the tab that separates it from what stands in front of it), the value's characters, and a literal suffix (the tab
// in front of tname behind the strand, the line feed behind rl).  Fields 0..3 stand between the names, 4..14 behind tname.
//
// dv travels as a u32 CODE per chain: 0 prints "0" (dv < FLT_EPSILON: mapping.rs:136-147), r + 1 prints r / 10^4 with four
// decimals, r = dv * 10^4 rounded to an integer exactly as "%.4f" rounds the float (exact decimal value, ties to even).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PAF_HD __host__ __device__ __forceinline__
#else
#define PAF_HD static inline
#endif

// ---- one record, as the chain kernels leave it (lrge_hip_chain: 12 dwords) ----
#define PAF_REC_DWORDS 12u
#define PAF_R_QUERY 0u
#define PAF_R_TARGET 1u
#define PAF_R_REV 2u
#define PAF_R_SCORE 3u
#define PAF_R_CNT 4u
#define PAF_R_QS 5u
#define PAF_R_QE 6u
#define PAF_R_RS 7u
#define PAF_R_RE 8u
#define PAF_R_MLEN 9u
#define PAF_R_BLEN 10u
#define PAF_R_NSEEDS 11u

// ---- the fixed part ----
#define PAF_N_FIELDS 15u
#define PAF_F_QLEN 0u
#define PAF_F_QS 1u
#define PAF_F_QE 2u
#define PAF_F_STRAND 3u
#define PAF_F_TLEN 4u      // first field behind tname
#define PAF_F_RS 5u
#define PAF_F_RE 6u
#define PAF_F_MLEN 7u
#define PAF_F_BLEN 8u
#define PAF_F_MAPQ 9u
#define PAF_F_TP 10u
#define PAF_F_CM 11u
#define PAF_F_S1 12u
#define PAF_F_DV 13u
#define PAF_F_RL 14u

// what a field's value is
#define PAF_V_NONE 0u      // prefix only
#define PAF_V_U32 1u
#define PAF_V_I32 2u
#define PAF_V_STRAND 3u    // '+' / '-'
#define PAF_V_DV 4u        // from the dv code

// widths: characters of the widest value of each kind
#define PAF_W_U32 10u      // 4294967295
#define PAF_W_I32 11u      // -2147483648
#define PAF_W_DV 6u        // 1.0000 (dv <= 1: it is 1 - p, p >= 0)
#define PAF_TEXT_MAX 16u   // a value's characters travel in two u64

PAF_HD constexpr uint32_t paf_field_kind(uint32_t f) {
    return (f == PAF_F_QLEN || f == PAF_F_TLEN) ? PAF_V_U32 : f == PAF_F_STRAND ? PAF_V_STRAND : (f == PAF_F_MAPQ || f == PAF_F_TP) ? PAF_V_NONE
           : f == PAF_F_DV ? PAF_V_DV : PAF_V_I32;
}
// characters in front of the value (the separating tab included) and behind it
PAF_HD constexpr uint32_t paf_prefix_len(uint32_t f) {
    return f == PAF_F_MAPQ ? 2u : f == PAF_F_TP ? 7u : (f == PAF_F_CM || f == PAF_F_S1 || f == PAF_F_DV || f == PAF_F_RL) ? 6u : 1u;
}
PAF_HD constexpr uint32_t paf_suffix_len(uint32_t f) { return (f == PAF_F_STRAND || f == PAF_F_RL) ? 1u : 0u; }
PAF_HD constexpr uint32_t paf_value_max(uint32_t f) {
    return paf_field_kind(f) == PAF_V_U32 ? PAF_W_U32 : paf_field_kind(f) == PAF_V_I32 ? PAF_W_I32 : paf_field_kind(f) == PAF_V_DV ? PAF_W_DV
           : paf_field_kind(f) == PAF_V_STRAND ? 1u : 0u;
}
PAF_HD constexpr uint32_t paf_field_max(uint32_t f) { return paf_prefix_len(f) + paf_value_max(f) + paf_suffix_len(f); }
PAF_HD constexpr uint32_t paf_fixed_sum(uint32_t f) { return f == 0 ? 0u : paf_fixed_sum(f - 1) + paf_field_max(f - 1); }
// the bound of everything in a line except the two names, the line feed included
constexpr uint32_t PAF_FIXED_BOUND = paf_fixed_sum(PAF_N_FIELDS);
constexpr uint32_t PAF_FIELD_BOUND = 6u + PAF_W_I32 + 1u;      // the widest single field (rl)
static_assert(PAF_FIXED_BOUND == 170u, "the fixed part of a PAF line: 15 fields at their widest");
static_assert(paf_field_max(PAF_F_RL) == PAF_FIELD_BOUND && paf_field_max(PAF_F_CM) < PAF_FIELD_BOUND, "rl is the widest field");

// byte j of field f's prefix: "\t", "\t0", "\ttp:A:S", "\tcm:i:", "\ts1:i:", "\tdv:f:", "\trl:i:"
PAF_HD uint8_t paf_prefix_byte(uint32_t f, uint32_t j) {
    if (j == 0) return (uint8_t)'\t';
    if (f == PAF_F_MAPQ) return (uint8_t)'0';
    if (f == PAF_F_TP) return (uint8_t)("tp:A:S"[j - 1]);
    if (j >= 3) return (uint8_t)(j != 4 ? ':' : f == PAF_F_DV ? 'f' : 'i');      // "xx:i:" -- dv has f in place of i
    const uint32_t two = f == PAF_F_CM ? ('c' | 'm' << 8) : f == PAF_F_S1 ? ('s' | '1' << 8) : f == PAF_F_DV ? ('d' | 'v' << 8) : ('r' | 'l' << 8);
    return (uint8_t)(two >> (8 * (j - 1)));
}
PAF_HD uint8_t paf_suffix_byte(uint32_t f) { return (uint8_t)(f == PAF_F_STRAND ? '\t' : '\n'); }

// ---- a value's characters: character j in byte j, lo first ----
struct PafText { uint64_t lo, hi; uint32_t n; };
PAF_HD void paf_text_push(PafText &t, uint8_t c) {
    if (t.n < 8) t.lo |= (uint64_t)c << (8 * t.n); else t.hi |= (uint64_t)c << (8 * (t.n - 8));
    ++t.n;
}
PAF_HD uint8_t paf_text_byte(const PafText &t, uint32_t j) { return (uint8_t)(j < 8 ? t.lo >> (8 * j) : t.hi >> (8 * (j - 8))); }
PAF_HD uint32_t paf_u32_digits(uint32_t v) {
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u
           : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
// decimal of v, at least min_digits wide (zero-padded), appended to t
PAF_HD void paf_text_u32(PafText &t, uint32_t v, uint32_t min_digits) {
    uint32_t nd = paf_u32_digits(v);
    if (nd < min_digits) nd = min_digits;
    uint32_t div = 1;
    for (uint32_t i = 1; i < nd; ++i) div *= 10u;
    for (uint32_t i = 0; i < nd; ++i) { const uint32_t d = v / div; paf_text_push(t, (uint8_t)('0' + d)); v -= d * div; div /= 10u; }
}
PAF_HD void paf_text_i32(PafText &t, int32_t v) {
    uint32_t mag = (uint32_t)v;
    if (v < 0) { paf_text_push(t, (uint8_t)'-'); mag = 0u - mag; }      // (INT32_MIN: 2147483648)
    paf_text_u32(t, mag, 1);
}

// ---- dv ----
#define PAF_FLT_EPSILON 1.1920929e-07f
#define PAF_DV_NAN 0xFFFFFFFFu      // not a number, or above 1: never printed, the chain counts as unproven
// %.4f of a float as an integer number of 1e-4 steps: dv = m * 2^-s exactly, m < 2^24, so m * 10^4 < 2^38 and the quotient by 2^s,
// the remainder and the half decide the rounding exactly (ties to even, as glibc's printf rounds the exact decimal expansion)
PAF_HD uint32_t paf_round_1e4(float dv, int half_up) {
    uint32_t bits;
    memcpy(&bits, &dv, 4);
    const uint32_t ex = (bits >> 23) & 0xFFu;
    const uint64_t m = ex ? ((bits & 0x7FFFFFu) | 0x800000u) : (bits & 0x7FFFFFu);
    const int e = (int)(ex ? ex : 1u) - 150;          // dv = m * 2^e
    const uint64_t N = m * 10000u;
    if (e >= 0) return 0xFFFFFFFEu;                   // (dv >= 2^23: far outside what 1 - p can be; paf_dv_code_ex never asks)
    const int s = -e;
    if (s > 62) return 0u;                            // N < 2^38 is below half a step
    const uint64_t q = N >> s, rem = N & ((1ull << s) - 1ull), half = 1ull << (s - 1);
    return (uint32_t)q + ((rem > half || (rem == half && (half_up || (q & 1ull)))) ? 1u : 0u);
}
// half_up != 0: round-half-up in place of ties-to-even -- the near miss the CPU test must be able to tell apart (never the product)
PAF_HD uint32_t paf_dv_code_ex(float dv, int half_up) {
    if (dv != dv || dv > 1.0f) return PAF_DV_NAN;     // (1 - p with p >= 0 is at most 1: PAF_W_DV rests on it)
    if (dv < PAF_FLT_EPSILON) return 0u;              // the -1 of a query without a kept seed included
    return paf_round_1e4(dv, half_up) + 1u;
}
PAF_HD uint32_t paf_dv_code(float dv) { return paf_dv_code_ex(dv, 0); }
PAF_HD void paf_text_dv(PafText &t, uint32_t code) {
    if (code == 0u) { paf_text_push(t, (uint8_t)'0'); return; }
    const uint32_t r = code - 1u;
    paf_text_u32(t, r / 10000u, 1);
    paf_text_push(t, (uint8_t)'.');
    paf_text_u32(t, r % 10000u, 4);
}
PAF_HD uint32_t paf_dv_width(uint32_t code) { return code == 0u ? 1u : paf_u32_digits((code - 1u) / 10000u) + 5u; }

// mm_est_err (mm2:esterr.c) in the arithmetic of paf.chain_dv: the ingredients of one chain.
// state 0: no kept seed, dv = -1;  1: n_match >= n_tot, dv = 0;  2: dv = (float)(1.0 - pow(x, y))
struct PafEst { int state; double x, y; };
PAF_HD PafEst paf_est(int32_t cnt, int32_t n_seeds, int32_t qs, int32_t rs, int32_t re, uint32_t qlen, uint32_t tlen, uint64_t sum_span, uint32_t n_kept) {
    PafEst r; r.state = 0; r.x = 0.0; r.y = 0.0;
    if (n_kept == 0u) return r;
    const float avg_k = (float)sum_span / (float)n_kept;
    int64_t n_tot = n_seeds;
    if ((float)qs > avg_k && (float)rs > avg_k) ++n_tot;
    if ((float)((int64_t)qlen - qs) > avg_k && (float)((int64_t)tlen - re) > avg_k) ++n_tot;
    if ((int64_t)cnt >= n_tot) { r.state = 1; return r; }
    r.state = 2; r.x = (double)cnt / (double)n_tot; r.y = 1.0 / (double)avg_k;
    return r;
}
PAF_HD float paf_dv_of_p(double p) { return (float)(1.0 - p); }

// The proof of a dv code.  The host lines take p from glibc's pow, the device from the ROCm device library's; neither is
// correctly rounded.  The map p -> code is monotone (p up, dv down, code down), so the codes at both ends of a window around p
// that holds every value either library may return decide it: equal codes there, and whatever the other library returned prints
// the same characters.  PAF_POW_ULPS_HOST: glibc manual, "Errors in Math Functions", pow on x86_64: 1 ulp.  PAF_POW_ULPS_DEVICE:
// no bound for the device library's double pow is documented in the tree this was written against; 4 is assumed, NOT verified.
#define PAF_POW_ULPS_HOST 1.0
#define PAF_POW_ULPS_DEVICE 4.0
#define PAF_POW_ULPS (PAF_POW_ULPS_HOST + PAF_POW_ULPS_DEVICE)
PAF_HD double paf_ulp(double p) {
    uint64_t b;
    memcpy(&b, &p, 8);
    const uint64_t ex = (b >> 52) & 0x7FFull;
    uint64_t u = ex > 52 ? (ex - 52) << 52 : 1ull;    // 2^(e - 52); below 2^-970 the smallest subnormal (dv is 1 there whatever the window)
    double r;
    memcpy(&r, &u, 8);
    return r;
}
// 1: the window [p - w ulp(p), p + w ulp(p)] holds a code boundary (or p is not a number): the chain is unproven
PAF_HD int paf_p_unproven(double p, double w) {
    if (p != p) return 1;
    const double d = w * paf_ulp(p);
    return paf_dv_code(paf_dv_of_p(p - d)) != paf_dv_code(paf_dv_of_p(p + d)) ? 1 : 0;
}
// the dv code of one chain and whether it is proven; `pw` is the library's pow
#define PAF_CHAIN_DV(est, pw, code, unproven)                                                     \
    do {                                                                                          \
        (unproven) = 0;                                                                           \
        if ((est).state == 0) (code) = paf_dv_code(-1.0f);                                        \
        else if ((est).state == 1) (code) = paf_dv_code(0.0f);                                    \
        else { const double p_ = pw((est).x, (est).y); (code) = paf_dv_code(paf_dv_of_p(p_)); (unproven) = paf_p_unproven(p_, PAF_POW_ULPS); } \
        if ((code) == PAF_DV_NAN) (unproven) = 1;                                                 \
    } while (0)

// ---- one field: its value's characters and its width; the length step and the write step both go through here ----
// v: the field's value (a record dword, a read length, the dv code, rl; unused for mapq / tp).  Returns the field's width.
PAF_HD uint32_t paf_field(uint32_t f, uint32_t v, PafText &t) {
    t.lo = 0; t.hi = 0; t.n = 0;
    const uint32_t kind = paf_field_kind(f);
    if (kind == PAF_V_U32) paf_text_u32(t, v, 1);
    else if (kind == PAF_V_I32) paf_text_i32(t, (int32_t)v);
    else if (kind == PAF_V_STRAND) paf_text_push(t, (uint8_t)(v ? '-' : '+'));
    else if (kind == PAF_V_DV) paf_text_dv(t, v);
    return paf_prefix_len(f) + t.n + paf_suffix_len(f);
}
// the width alone (the length step needs no characters)
PAF_HD uint32_t paf_field_width(uint32_t f, uint32_t v) {
    const uint32_t kind = paf_field_kind(f);
    const uint32_t w = kind == PAF_V_U32 ? paf_u32_digits(v) : kind == PAF_V_I32 ? ((int32_t)v < 0 ? 1u + paf_u32_digits(0u - v) : paf_u32_digits(v))
                       : kind == PAF_V_STRAND ? 1u : kind == PAF_V_DV ? paf_dv_width(v) : 0u;
    return paf_prefix_len(f) + w + paf_suffix_len(f);
}
// byte j of the field, 0 <= j < its width
PAF_HD uint8_t paf_field_byte(uint32_t f, const PafText &t, uint32_t j) {
    const uint32_t pl = paf_prefix_len(f);
    return j < pl ? paf_prefix_byte(f, j) : j < pl + t.n ? paf_text_byte(t, j - pl) : paf_suffix_byte(f);
}
// which record dword field f prints (PAF_REC_DWORDS: none of them -- a read length, the dv code, rl, or no value)
PAF_HD uint32_t paf_field_rec_dword(uint32_t f) {
    return f == PAF_F_QS ? PAF_R_QS : f == PAF_F_QE ? PAF_R_QE : f == PAF_F_STRAND ? PAF_R_REV : f == PAF_F_RS ? PAF_R_RS : f == PAF_F_RE ? PAF_R_RE
           : f == PAF_F_MLEN ? PAF_R_MLEN : f == PAF_F_BLEN ? PAF_R_BLEN : f == PAF_F_CM ? PAF_R_CNT : f == PAF_F_S1 ? PAF_R_SCORE : PAF_REC_DWORDS;
}
// the value of field f of one line
PAF_HD uint32_t paf_field_value(uint32_t f, const uint32_t *rec, uint32_t qlen, uint32_t tlen, uint32_t code, int32_t rl) {
    const uint32_t d = paf_field_rec_dword(f);
    return d < PAF_REC_DWORDS ? rec[d] : f == PAF_F_QLEN ? qlen : f == PAF_F_TLEN ? tlen : f == PAF_F_DV ? code : f == PAF_F_RL ? (uint32_t)rl : 0u;
}
// the width of the fixed part of one line
PAF_HD uint32_t paf_fixed_width(const uint32_t *rec, uint32_t qlen, uint32_t tlen, uint32_t code, int32_t rl) {
    uint32_t w = 0;
    for (uint32_t f = 0; f < PAF_N_FIELDS; ++f) w += paf_field_width(f, paf_field_value(f, rec, qlen, tlen, code, rl));
    return w;
}
