// name_lsd_check.cpp -- a stand-alone driver of the LSD identifier ranking's host twin (csrc/names_lsd_twin.cpp over
// csrc/name_lsd_round.h and csrc/name_lsd.h) for runs under the host sanitizers, which cannot see code loaded into an interpreter:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lrge_amd/csrc tools/name_lsd_check.cpp -o name_lsd_check
//   ./name_lsd_check
// The case families of tests/test_names_lsd_twin.py, generated here: empty and single lists, equal names of every length 0..26,
// prefix chains, pairs parting at every byte 0..24 with bytes 0x00 / 0x7f / 0x80 / 0xff there, trailing zero bytes, lengths around
// the word boundaries, heavy ties, a 21-byte shared prefix, r00000060-style names, index lists with repeats and in reverse, two
// lists ranked together, 5 000 UUID-like and PacBio-like names, every blob alignment, and the verdicts.  The names and offsets are
// passed in heap blocks of their exact size, so a load or store outside them is reported.  Each result is held to a comparison
// sort; the exit status is 1 when one differs.
// TEST INFRASTRUCTURE, not part of the product library.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "../lrge_amd/csrc/names_lsd_twin.cpp"

typedef std::vector<std::string> Names;

static uint64_t g_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }
static uint64_t cases = 0, bad = 0;

static std::vector<uint32_t> reference(const Names &sel) {
    std::vector<uint32_t> order(sel.size()), rank(sel.size());
    for (size_t i = 0; i < sel.size(); ++i) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return sel[a] < sel[b]; });   // std::string: byte-wise on unsigned bytes
    uint32_t r = 0;
    for (size_t j = 0; j < order.size(); ++j) {
        if (j && sel[order[j]] != sel[order[j - 1]]) r = (uint32_t)j;
        rank[order[j]] = r;
    }
    return rank;
}

// rc of the twin on idx (NULL: all) over exact-size heap copies; ranks into `got`
static int run(const Names &names, const std::vector<uint32_t> *idx, std::vector<uint32_t> &got, uint64_t st[4], uint64_t max_bytes = 0) {
    size_t total = 0;
    for (const auto &s : names) total += s.size();
    std::unique_ptr<char[]> blob(new char[total ? total : 1]);
    std::unique_ptr<uint64_t[]> off(new uint64_t[names.size() + 1]);
    size_t o = 0;
    for (size_t i = 0; i < names.size(); ++i) { off[i] = o; if (!names[i].empty()) memcpy(blob.get() + o, names[i].data(), names[i].size()); o += names[i].size(); }
    off[names.size()] = o;
    const uint64_t n = idx ? idx->size() : names.size();
    std::unique_ptr<uint32_t[]> ix(new uint32_t[idx && n ? n : 1]), out(new uint32_t[n ? n : 1]);
    if (idx) for (size_t i = 0; i < n; ++i) ix[i] = (*idx)[i];
    const int rc = names_lsd_twin_ranks(blob.get(), off.get(), names.size(), idx ? ix.get() : nullptr, n, out.get(), st, max_bytes);
    got.assign(out.get(), out.get() + (rc == 0 ? n : 0));
    return rc;
}

static void check(const char *what, const Names &names, const std::vector<uint32_t> *idx = nullptr) {
    ++cases;
    Names sel;
    if (idx) for (uint32_t i : *idx) sel.push_back(names[i]); else sel = names;
    std::vector<uint32_t> got;
    uint64_t st[4];
    const int rc = run(names, idx, got, st);
    size_t lmax = 0;
    for (const auto &s : sel) lmax = std::max(lmax, s.size());
    const uint64_t W = (lmax + 7) / 8;
    const bool ok = rc == 0 && got == reference(sel) && st[1] == W && st[0] == (sel.size() >= 2 ? W + 1 : 0) && st[2] == std::set<std::string>(sel.begin(), sel.end()).size();
    if (!ok) { ++bad; fprintf(stderr, "FAILED: %s (rc %d, %zu entries, sorts %llu, W %llu, distinct %llu)\n", what, rc, sel.size(), (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2]); }
}

static void expect_rc(const char *what, int rc, int want) {
    ++cases;
    if (rc != want) { ++bad; fprintf(stderr, "FAILED: %s: verdict %d, expected %d\n", what, rc, want); }
}

static std::string uuid() {
    static const char h[] = "0123456789abcdef";
    std::string s;
    for (int i = 0; i < 36; ++i) s += (i == 8 || i == 13 || i == 18 || i == 23) ? '-' : h[rnd() & 15];
    return s;
}
static std::string pacbio() { return "m64011_190830_220126/" + std::to_string(1 + rnd() % 180000000) + "/ccs"; }
static void shuffle(Names &v) { for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[rnd() % i]); }

int main() {
    std::vector<uint32_t> none;
    check("empty", Names());
    check("empty selection", Names{"abc", "x"}, &none);
    for (const char *s : {"", "a", "abcdefg", "abcdefgh"}) check("single", Names{s});
    check("single of 40", Names{std::string(40, 'q')});
    for (size_t ln = 0; ln <= 26; ++ln) check("all equal", Names(5, std::string(ln, 'z')));
    for (size_t top = 0; top <= 20; ++top) {
        Names v;
        for (size_t k = 0; k <= top; ++k) v.push_back(std::string(k, 'a'));
        shuffle(v);
        check("prefix chain", v);
    }
    const unsigned char odd[] = {0x00, 0x7f, 0x80, 0xff};
    for (size_t k = 0; k <= 24; ++k) {
        const std::string p(k, 'p');
        check("pair", Names{p + "B", p + "A"});
        check("pair with tail", Names{p + "Btail", p + "Atail"});
        check("pair, one ends", Names{p + "A", p});
        for (unsigned char x : odd) for (unsigned char y : odd) check("odd bytes at the parting position", Names{p + (char)x + "t", p + (char)y + "t", p});
    }
    check("trailing zero bytes", Names{std::string("ab\0\0", 4), "ab", std::string("ab\0", 3), std::string("ab\0\0", 4), "ab", "a", std::string("ab\0\0\0\0\0\0\0", 9), std::string("ab\0\0\0\0\0\0", 8)});
    for (size_t ln : {7, 8, 9, 15, 16, 17}) {
        Names v;
        for (int i = 0; i < 40; ++i) { std::string s; for (size_t j = 0; j < ln; ++j) s += (rnd() & 1) ? 'x' : 'y'; v.push_back(s); }
        v.push_back(v[0].substr(0, ln - 1)); v.push_back(v[1] + "x"); v.push_back(v[2].substr(0, ln - 1) + std::string(1, '\0')); v.push_back(v[3]);
        check("word boundaries", v);
    }
    {
        Names pool, v;
        for (int i = 0; i < 10; ++i) { std::string s; for (uint64_t j = rnd() % 13; j > 0; --j) s += (rnd() & 1) ? 'a' : 'b'; pool.push_back(s); }
        for (int i = 0; i < 1000; ++i) v.push_back(pool[rnd() % 10]);
        check("heavy ties", v);
    }
    {
        Names v;
        for (int i = 60; i < 75; ++i) { char b[16]; snprintf(b, sizeof b, "r%08d", i); v.push_back(b); }
        check("r-style", v);
        std::reverse(v.begin(), v.end());
        check("r-style reversed", v);
    }
    {
        Names v;
        for (int i = 0; i < 400; ++i) v.push_back(pacbio());
        for (int i = 0; i < 300; ++i) v.push_back(uuid());
        v.push_back("dup"); v.push_back("dup"); v.push_back("du"); v.push_back("");
        check("shared prefix", Names(v.begin(), v.begin() + 400));
        std::vector<uint32_t> rep, rev, qt;
        for (int i = 0; i < 900; ++i) rep.push_back((uint32_t)(rnd() % v.size()));
        for (size_t i = v.size(); i > 0; --i) rev.push_back((uint32_t)(i - 1));
        check("repeats", v, &rep);
        check("reverse order", v, &rev);
        // two lists ranked together: the concatenation, split by the caller
        for (int i = 0; i < 120; ++i) qt.push_back((uint32_t)(rnd() % v.size()));
        for (int i = 0; i < 200; ++i) qt.push_back((uint32_t)(rnd() % v.size()));
        check("queries then targets", v, &qt);
    }
    {
        Names u, p;
        for (int i = 0; i < 5000; ++i) { u.push_back(uuid()); p.push_back(pacbio()); }
        check("5000 UUID-like", u);
        check("5000 PacBio-like", p);
    }
    for (size_t lead = 0; lead < 8; ++lead) {
        Names v{std::string(lead, '#')};
        for (int i = 0; i < 50; ++i) v.push_back(uuid());
        v.push_back("ab"); v.push_back(std::string("ab\0", 3)); v.push_back("abcdefgh"); v.push_back("abcdefghi"); v.push_back("");
        std::vector<uint32_t> sel;
        for (size_t i = 1; i < v.size(); ++i) sel.push_back((uint32_t)i);
        check("alignment, lead unselected", v, &sel);
        check("alignment, lead selected", v);
    }
    // the verdicts
    std::vector<uint32_t> got;
    uint64_t st[4];
    std::vector<uint32_t> out_of_range{0, 3};
    expect_rc("index out of range", run(Names{"a", "b", "c"}, &out_of_range, got, st), -9);
    expect_rc("Lmax 257", run(Names{std::string(257, 'x'), "y"}, nullptr, got, st), -10);
    expect_rc("Lmax 256", run(Names{std::string(256, 'x'), "y", std::string(255, 'x')}, nullptr, got, st), 0);
    ++cases;
    if (st[0] != 33 || st[1] != 32 || got != std::vector<uint32_t>{1, 2, 0}) { ++bad; fprintf(stderr, "FAILED: Lmax 256: sorts %llu, W %llu\n", (unsigned long long)st[0], (unsigned long long)st[1]); }
    expect_rc("a cap of its own", run(Names{std::string(40, 'x'), "y"}, nullptr, got, st, 39), -10);
    {
        const uint64_t off[4] = {0, 1, 2, 3};
        uint32_t out[4];
        expect_rc("n = 2^32", names_lsd_twin_ranks("abc", off, 3, nullptr, 1ULL << 32, out, nullptr, 0), -3);
        expect_rc("no list, n != n_names", names_lsd_twin_ranks("abc", off, 3, nullptr, 2, out, nullptr, 0), -9);
        const uint64_t bad_off[4] = {0, 2, 1, 3};
        expect_rc("offsets not monotone", names_lsd_twin_ranks("abc", bad_off, 3, nullptr, 3, out, nullptr, 0), -9);
    }
    printf("%llu cases, %llu failed\n", (unsigned long long)cases, (unsigned long long)bad);
    if (!bad) printf("name_lsd_check: ok\n");
    return bad != 0;
}
