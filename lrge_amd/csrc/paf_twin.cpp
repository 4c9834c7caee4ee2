// paf_twin.cpp -- the PAF writer of k_paf.h / host_paf.inl as loops on the CPU (g++), over the same core
// (paf_core.h): the measure step per chain, the exclusive scan of one slice, and the write step with its 15 field lanes, its row
// and its 64-lane copies run as loops, every store guarded by the line's own byte range.  The CPU suite holds it to paf.paf_lines
// (tests/test_paf_twin.py); tools/paf_check.cpp drives it from heap blocks of exact size under the host sanitizers.
// TEST INFRASTRUCTURE, not part of the product library.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "paf_core.h"

namespace {
const uint32_t ROW_BYTES = 192;      // PAF_ROW_BYTES of k_paf.h
static_assert(ROW_BYTES >= PAF_FIXED_BOUND, "the row holds the fixed part");

struct In {
    const uint32_t *rec; const uint32_t *q_len, *t_len; const uint64_t *q_name_off, *t_name_off; const uint8_t *q_names, *t_names;
    const int32_t *rl; const uint64_t *sum_span; const uint32_t *n_kept;
};

// k_paf_measure, one chain
void measure(const In &in, uint64_t i, uint32_t *code_out, uint32_t *len_out, uint64_t *unproven) {
    const uint32_t *rec = in.rec + i * PAF_REC_DWORDS;
    const uint32_t q = rec[PAF_R_QUERY], t = rec[PAF_R_TARGET];
    const uint32_t qlen = in.q_len[q], tlen = in.t_len[t];
    const PafEst est = paf_est((int32_t)rec[PAF_R_CNT], (int32_t)rec[PAF_R_NSEEDS], (int32_t)rec[PAF_R_QS], (int32_t)rec[PAF_R_RS], (int32_t)rec[PAF_R_RE], qlen, tlen,
                               in.sum_span[q], in.n_kept[q]);
    uint32_t code; int bad;
    PAF_CHAIN_DV(est, pow, code, bad);
    *unproven += (uint64_t)bad;
    code_out[i] = code;
    len_out[i] = (uint32_t)(in.q_name_off[q + 1] - in.q_name_off[q]) + (uint32_t)(in.t_name_off[t + 1] - in.t_name_off[t]) + paf_fixed_width(rec, qlen, tlen, code, in.rl[q]);
}

// paf_wave_copy: 64 lanes, 64 bytes a step, nothing at or behind `end`
void wave_copy(uint8_t *dst, const uint8_t *src, uint32_t n, const uint8_t *end) {
    for (uint32_t step = 0; step < n; step += 64)
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t j = step + lane;
            if (j < n && dst + j < end) dst[j] = src[j];
        }
}

// k_paf_write, one line
void write_line(const In &in, uint64_t i, uint32_t li, const uint32_t *code, const uint32_t *off, uint8_t *out) {
    uint8_t row[ROW_BYTES];
    const uint32_t *rec = in.rec + i * PAF_REC_DWORDS;
    const uint32_t q = rec[PAF_R_QUERY], t = rec[PAF_R_TARGET];
    uint32_t w[PAF_N_FIELDS], pos[PAF_N_FIELDS];
    PafText tx[PAF_N_FIELDS];
    for (uint32_t f = 0; f < PAF_N_FIELDS; ++f)      // the field lanes
        w[f] = paf_field(f, paf_field_value(f, rec, in.q_len[q], in.t_len[t], code[i], in.rl[q]), tx[f]);
    uint32_t acc = 0;
    for (uint32_t f = 0; f < PAF_N_FIELDS; ++f) { pos[f] = acc; acc += w[f]; }      // the wave prefix sum
    for (uint32_t f = 0; f < PAF_N_FIELDS; ++f)
        for (uint32_t j = 0; j < w[f]; ++j)
            if (pos[f] + j < ROW_BYTES) row[pos[f] + j] = paf_field_byte(f, tx[f], j);
    const uint32_t len_a = pos[PAF_F_TLEN], len_f = acc;
    const uint64_t qa = in.q_name_off[q], ta = in.t_name_off[t];
    const uint32_t qnl = (uint32_t)(in.q_name_off[q + 1] - qa), tnl = (uint32_t)(in.t_name_off[t + 1] - ta);
    uint8_t *dst = out + off[li];
    const uint8_t *end = out + off[li + 1];
    wave_copy(dst, in.q_names + qa, qnl, end);
    wave_copy(dst + qnl, row, len_a, end);
    wave_copy(dst + qnl + len_a, in.t_names + ta, tnl, end);
    wave_copy(dst + qnl + len_a + tnl, row + len_a, len_f - len_a, end);
}
}  // namespace

extern "C" {

// The whole formatter.  rec: n records of 12 dwords; q_len / rl / sum_span / n_kept: nq entries; t_len: nt; the name tables as
// lrge_hip_paf_text takes them.  piece_bytes: PAF_PIECE_BYTES.  out: room for out_cap bytes; *out_bytes: what the text needs (written
// only when it fits).  slice_end[0..*n_slices): the byte at which every slice ends (at most slice_cap are recorded).
// 0; -10: stats[0] chains unproven, nothing written; -9: a record names a read outside its set, offsets that do not ascend.
// stats: {unproven, slices, bound, lines}
int paf_twin_format(const uint32_t *rec, uint64_t n, uint32_t nq, uint32_t nt, const uint32_t *q_len, const uint32_t *t_len, const uint8_t *q_names,
                    const uint64_t *q_name_off, const uint8_t *t_names, const uint64_t *t_name_off, const int32_t *rl, const uint64_t *sum_span,
                    const uint32_t *n_kept, uint64_t piece_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes, uint64_t *slice_end,
                    uint64_t slice_cap, uint64_t *n_slices, uint64_t stats[4]) {
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    *out_bytes = 0; *n_slices = 0;
    uint64_t q_longest = 0, t_longest = 0;
    for (uint32_t r = 0; r < nq; ++r) { if (q_name_off[r + 1] < q_name_off[r]) return -9; if (q_name_off[r + 1] - q_name_off[r] > q_longest) q_longest = q_name_off[r + 1] - q_name_off[r]; }
    for (uint32_t r = 0; r < nt; ++r) { if (t_name_off[r + 1] < t_name_off[r]) return -9; if (t_name_off[r + 1] - t_name_off[r] > t_longest) t_longest = t_name_off[r + 1] - t_name_off[r]; }
    for (uint64_t i = 0; i < n; ++i) if (rec[i * PAF_REC_DWORDS + PAF_R_QUERY] >= nq || rec[i * PAF_REC_DWORDS + PAF_R_TARGET] >= nt) return -9;
    if (n == 0) return 0;
    const In in{rec, q_len, t_len, q_name_off, t_name_off, q_names, t_names, rl, sum_span, n_kept};
    std::vector<uint32_t> code(n), len(n);
    uint64_t unproven = 0, total = 0;
    for (uint64_t i = 0; i < n; ++i) { measure(in, i, code.data(), len.data(), &unproven); total += len[i]; }
    stats[0] = unproven;
    if (unproven) return -10;
    const uint64_t bound = q_longest + t_longest + PAF_FIXED_BOUND;
    uint64_t per_slice = piece_bytes / bound;
    if (per_slice < 1) per_slice = 1;
    if (per_slice > n) per_slice = n;
    stats[2] = bound; stats[3] = n;
    *out_bytes = total;
    if (total > out_cap) return 0;
    uint64_t at = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += per_slice) {
        const uint32_t m = (uint32_t)(n - i0 < per_slice ? n - i0 : per_slice);
        std::vector<uint32_t> off((size_t)m + 1);
        uint32_t acc = 0;
        for (uint32_t j = 0; j < m; ++j) { off[j] = acc; acc += len[i0 + j]; }      // scan_exclusive_u32
        off[m] = acc;
        std::vector<uint8_t> text(acc);                                             // the slice's text: a block of exactly its size
        for (uint32_t li = 0; li < m; ++li) write_line(in, i0 + li, li, code.data(), off.data(), text.data());
        if (acc) memcpy(out + at, text.data(), acc);
        at += acc;
        if (*n_slices < slice_cap) slice_end[*n_slices] = at;
        ++*n_slices;
    }
    stats[1] = *n_slices;
    return at == total ? 0 : -100;
}

// the dv code of a float (half_up != 0: the near miss -- round-half-up in place of ties-to-even) and its characters (at most 16)
uint32_t paf_twin_dv_code(float dv, int half_up) { return paf_dv_code_ex(dv, half_up); }
uint32_t paf_twin_dv_text(uint32_t code, uint8_t out[16]) {
    PafText t; t.lo = 0; t.hi = 0; t.n = 0;
    paf_text_dv(t, code);
    for (uint32_t j = 0; j < t.n && j < 16; ++j) out[j] = paf_text_byte(t, j);
    return t.n;
}
// the proof of a p: 1 when [p - w ulp(p), p + w ulp(p)] holds a code boundary; the w the product uses; the code at p
int paf_twin_p_unproven(double p, double w) { return paf_p_unproven(p, w); }
double paf_twin_pow_ulps(void) { return PAF_POW_ULPS; }
uint32_t paf_twin_code_of_p(double p) { return paf_dv_code(paf_dv_of_p(p)); }
uint32_t paf_twin_fixed_bound(void) { return PAF_FIXED_BOUND; }

}  // extern "C"
