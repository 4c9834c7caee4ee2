// paf_check.cpp -- a stand-alone driver of the PAF writer's host twin (csrc/paf_twin.cpp over csrc/paf_core.h) for runs under the
// host sanitizers, which cannot see code loaded into an interpreter:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lrge_amd/csrc tools/paf_check.cpp -o paf_check
//   ./paf_check CASES
// CASES is what tests/test_paf_twin.py writes: "PAFC", a u32 count, then per case {u64 n, u32 nq, u32 nt, u64 piece bytes, u64 query
// name bytes, u64 target name bytes, u64 text bytes} and the arrays in the order of paf_twin_format's arguments, the expected text
// (paf.paf_lines plus line feeds) last.  Every array and the output go through heap blocks of their exact size, so a load or store
// outside them is reported.  The dv cases are generated here and held to printf's "%.4f": FLT_EPSILON, the exact ties k / 32 and
// 0.99995f with both neighbours, -1, 0, 100 000 floats of [0, 1), 10 000 of [2^-23, 2^-10).  The exit status is 1 when anything differs.
// TEST INFRASTRUCTURE, not part of the product library.
#include <float.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../lrge_amd/csrc/paf_twin.cpp"

static uint64_t g_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }
static uint64_t cases = 0, bad = 0;

// a heap block of exactly `bytes` bytes holding a copy of p (one byte when empty: the pointer must still be valid)
struct Block {
    uint8_t *p;
    Block(const uint8_t *src, uint64_t bytes) : p((uint8_t *)malloc(bytes ? bytes : 1)) { if (bytes && src) memcpy(p, src, bytes); }
    ~Block() { free(p); }
    Block(const Block &) = delete; Block &operator=(const Block &) = delete;
};

static void check_dv(float x) {
    ++cases;
    uint8_t got[16];
    const uint32_t n = paf_twin_dv_text(paf_twin_dv_code(x, 0), got);
    char exp[64];
    if (x < FLT_EPSILON) snprintf(exp, sizeof exp, "0"); else snprintf(exp, sizeof exp, "%.4f", (double)x);
    if (std::string((const char *)got, n) != exp) { if (bad++ < 10) fprintf(stderr, "paf_check: dv %.9g prints %.*s, printf %s\n", (double)x, (int)n, (const char *)got, exp); }
}
static void check_dv3(float x) { check_dv(nextafterf(x, -2.0f)); check_dv(x); check_dv(nextafterf(x, 2.0f)); }

static bool run_case(const uint8_t *&at, const uint8_t *end, uint32_t ci) {
    struct Head { uint64_t n; uint32_t nq, nt; uint64_t piece, qn_bytes, tn_bytes, text_bytes; } __attribute__((packed));
    if ((uint64_t)(end - at) < sizeof(Head)) return false;
    Head h;
    memcpy(&h, at, sizeof h); at += sizeof h;
    const uint64_t sizes[11] = {h.n * 48, (uint64_t)h.nq * 4, (uint64_t)h.nt * 4, ((uint64_t)h.nq + 1) * 8, ((uint64_t)h.nt + 1) * 8, h.qn_bytes, h.tn_bytes,
                                (uint64_t)h.nq * 4, (uint64_t)h.nq * 8, (uint64_t)h.nq * 4, h.text_bytes};
    uint64_t need = 0;
    for (uint64_t s : sizes) need += s;
    if ((uint64_t)(end - at) < need) return false;
    const uint8_t *src[11];
    for (int i = 0; i < 11; ++i) { src[i] = at; at += sizes[i]; }
    Block rec(src[0], sizes[0]), qlen(src[1], sizes[1]), tlen(src[2], sizes[2]), qoff(src[3], sizes[3]), toff(src[4], sizes[4]), qn(src[5], sizes[5]),
        tn(src[6], sizes[6]), rl(src[7], sizes[7]), ss(src[8], sizes[8]), nk(src[9], sizes[9]);
    Block out(nullptr, h.text_bytes);
    std::vector<uint64_t> ends(h.n ? h.n : 1);
    uint64_t out_bytes = 0, n_slices = 0, st[4];
    const int rc = paf_twin_format((const uint32_t *)rec.p, h.n, h.nq, h.nt, (const uint32_t *)qlen.p, (const uint32_t *)tlen.p, qn.p, (const uint64_t *)qoff.p, tn.p,
                                   (const uint64_t *)toff.p, (const int32_t *)rl.p, (const uint64_t *)ss.p, (const uint32_t *)nk.p, h.piece, out.p, h.text_bytes,
                                   &out_bytes, ends.data(), ends.size(), &n_slices, st);
    ++cases;
    bool ok = rc == 0 && out_bytes == h.text_bytes && (h.text_bytes == 0 || memcmp(out.p, src[10], h.text_bytes) == 0);
    for (uint64_t s = 0; ok && s < n_slices; ++s) ok = ends[s] > 0 && ends[s] <= h.text_bytes && out.p[ends[s] - 1] == '\n';
    if (!ok) { ++bad; fprintf(stderr, "paf_check: case %u (piece %llu): rc %d, %llu bytes for %llu expected, %llu slices\n", ci, (unsigned long long)h.piece, rc,
                              (unsigned long long)out_bytes, (unsigned long long)h.text_bytes, (unsigned long long)n_slices); }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: paf_check CASES\n"); return 2; }
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) { fprintf(stderr, "paf_check: cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> file;
    uint8_t buf[1 << 16];
    for (size_t k; (k = fread(buf, 1, sizeof buf, fh)) > 0;) file.insert(file.end(), buf, buf + k);
    fclose(fh);
    if (file.size() < 8 || memcmp(file.data(), "PAFC", 4) != 0) { fprintf(stderr, "paf_check: %s is no case file\n", argv[1]); return 2; }
    uint32_t n_cases;
    memcpy(&n_cases, file.data() + 4, 4);
    const uint8_t *at = file.data() + 8, *end = file.data() + file.size();
    for (uint32_t ci = 0; ci < n_cases; ++ci)
        if (!run_case(at, end, ci)) { fprintf(stderr, "paf_check: case %u is cut short\n", ci); return 2; }

    check_dv3(FLT_EPSILON); check_dv3(0.03125f); check_dv3(0.09375f); check_dv3(0.15625f); check_dv3(0.99995f);
    check_dv(-1.0f); check_dv(0.0f); check_dv(1.0f);
    for (int i = 0; i < 100000; ++i) check_dv((float)(rnd() >> 40) * (1.0f / 16777216.0f));
    for (int i = 0; i < 10000; ++i) check_dv(ldexpf(1.0f + (float)(rnd() >> 41) * (1.0f / 8388608.0f), -23 + (int)(rnd() % 13)));
    // the near miss must be told apart: round-half-up differs on two of the three ties
    {
        uint8_t a[16], b[16];
        int differ = 0;
        for (float t : {0.03125f, 0.09375f, 0.15625f}) {
            const uint32_t na = paf_twin_dv_text(paf_twin_dv_code(t, 0), a), nb = paf_twin_dv_text(paf_twin_dv_code(t, 1), b);
            differ += na != nb || memcmp(a, b, na) != 0;
        }
        ++cases;
        if (differ != 2) { ++bad; fprintf(stderr, "paf_check: round-half-up differs on %d of the 3 ties (2 expected)\n", differ); }
    }
    printf("paf_check: %s, %llu checks over %u formatter cases, %llu differ\n", bad ? "FAILED" : "ok", (unsigned long long)cases, n_cases, (unsigned long long)bad);
    return bad ? 1 : 0;
}
