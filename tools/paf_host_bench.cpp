// paf_host_bench.cpp -- the host path of overlaps.paf (lrge::paf_lines of include/lrge_hip.hpp, what -C runs without --gpu-paf) with a
// clock around each of its steps, for tools/paf_bench.py: the counting call of lrge_hip_chains, the filling call, lrge_hip_paf_stats,
// the formatter (lrge::paf_format_lines) and the file write.  Built by lrge_amd.build.build_paf_host_bench (g++, links liblrge_hip.so).
// BENCH INFRASTRUCTURE, not part of the product library.
#include <chrono>
#include <fstream>

#include "../include/lrge_hip.hpp"

static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// names as lrge_hip_paf_text takes them; us: {chains (count), chains (fill), paf_stats, format, file write}; out: {lines, bytes}
extern "C" int paf_host_bench(lrge_hip_ctx *ctx, const lrge_hip_index *ix, const lrge_hip_seqset *qs, int dual, const char *q_names, const uint64_t *q_off,
                              uint32_t nq, const uint32_t *q_len, const char *t_names, const uint64_t *t_off, uint32_t nt, const uint32_t *t_len,
                              const char *path, double us[5], uint64_t out[2]) {
    std::vector<std::string> qn_s(nq), tn_s(nt);
    for (uint32_t i = 0; i < nq; ++i) qn_s[i].assign(q_names + q_off[i], q_names + q_off[i + 1]);
    for (uint32_t i = 0; i < nt; ++i) tn_s[i].assign(t_names + t_off[i], t_names + t_off[i + 1]);
    std::vector<const std::string *> qn, tn;
    for (auto &s : qn_s) qn.push_back(&s);
    for (auto &s : tn_s) tn.push_back(&s);
    const std::vector<uint32_t> qlen(q_len, q_len + nq), tlen(t_len, t_len + nt);
    double t0 = now_us();
    uint64_t n = 0;
    int rc = lrge_hip_chains(ctx, ix, qs, dual, nullptr, 0, &n);
    if (rc) return rc;
    double t1 = now_us();
    std::vector<lrge_hip_chain> ch(n ? n : 1);
    rc = lrge_hip_chains(ctx, ix, qs, dual, ch.data(), n, &n);
    if (rc) return rc;
    double t2 = now_us();
    std::vector<int32_t> rl(nq + 1); std::vector<uint64_t> ss(nq + 1); std::vector<uint32_t> nk(nq + 1);
    rc = lrge_hip_paf_stats(ctx, ix, qs, rl.data(), ss.data(), nk.data());
    if (rc) return rc;
    double t3 = now_us();
    const std::vector<std::string> lines = lrge::paf_format_lines(ch.data(), n, rl.data(), ss.data(), nk.data(), qn, qlen, tn, tlen);
    double t4 = now_us();
    uint64_t bytes = 0;
    {
        std::ofstream pf(path, std::ios::binary);
        if (!pf) return LRGE_ERR_PAF_WRITE;
        for (auto &l : lines) { pf << l << "\n"; bytes += l.size() + 1; }      // (as tools/lrge_hip_cli.cpp writes them)
        pf.close();
        if (!pf) return LRGE_ERR_PAF_WRITE;
    }
    double t5 = now_us();
    us[0] = t1 - t0; us[1] = t2 - t1; us[2] = t3 - t2; us[3] = t4 - t3; us[4] = t5 - t4;
    out[0] = lines.size(); out[1] = bytes;
    return LRGE_OK;
}
