// zstd_slide_check.cpp -- a stand-alone driver of the sliding mode of the Zstandard decode's host twin (csrc/zs_twin.cpp over
// csrc/zs_round.h and csrc/zs_core.h) for runs under the host sanitizers, which cannot see code loaded into an
// interpreter:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lrge_amd/csrc tools/zstd_slide_check.cpp -o zstd_slide_check
//   ./zstd_slide_check DIR
// DIR holds cases written by tests/test_zstd_slide_twin.py, in the layout of tools/zstd_check.cpp: NAME.zst beside NAME.plain (the
// text libzstd gives: the sliding twin must give it at rounds of 1, 2, 3 and 0 blocks, with and without the checksums, with the
// statistics of the twin that keeps the whole text) or beside NAME.status (the decimal ZS_E_* status both must refuse it with, at
// the same byte offset); NAME.edit holds a stream with a damaged byte, which the twin may take or refuse.  Every input is passed in
// a heap block of its exact size, and every round's work text [history | round] is a heap block of its exact size (zs_twin.cpp), so
// a load in front of the history or behind the round is reported.  The exit status is 1 when a case differs.
// TEST INFRASTRUCTURE, not part of the product library.
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <string>
#include <vector>

#include "../lrge_amd/csrc/zs_twin.cpp"

static bool slurp(const std::string &path, std::vector<uint8_t> &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    out.clear();
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + k);
    fclose(f);
    return true;
}

static bool ends_with(const std::string &s, const char *suffix) {
    const std::string t(suffix);
    return s.size() >= t.size() && s.compare(s.size() - t.size(), t.size(), t) == 0;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: zstd_slide_check DIR\n"); return 2; }
    const std::string dir = argv[1];
    DIR *d = opendir(dir.c_str());
    if (!d) { fprintf(stderr, "zstd_slide_check: cannot open %s\n", dir.c_str()); return 2; }
    std::vector<std::string> names, edits;
    while (dirent *e = readdir(d)) {
        const std::string n = e->d_name;
        if (ends_with(n, ".zst")) names.push_back(n.substr(0, n.size() - 4));
        if (ends_with(n, ".edit")) edits.push_back(n);
    }
    closedir(d);
    uint64_t cases = 0, bad = 0;
    const uint64_t rounds[4] = {1, 2, 3, 0};
    for (const std::string &name : names) {
        std::vector<uint8_t> comp, want;
        if (!slurp(dir + "/" + name + ".zst", comp)) { ++bad; continue; }
        std::unique_ptr<uint8_t[]> exact(new uint8_t[comp.size() ? comp.size() : 1]);
        if (!comp.empty()) memcpy(exact.get(), comp.data(), comp.size());
        const bool accept = slurp(dir + "/" + name + ".plain", want);
        int status = 0;
        if (!accept) {
            std::vector<uint8_t> s;
            if (!slurp(dir + "/" + name + ".status", s)) { fprintf(stderr, "zstd_slide_check: %s has neither .plain nor .status\n", name.c_str()); ++bad; continue; }
            status = atoi(std::string(s.begin(), s.end()).c_str());
        }
        for (uint64_t round : rounds)
            for (int checksum = 1; checksum >= 0; --checksum) {
                uint64_t stats[9], whole[9], slide[4], off = 0, whole_off = 0;
                const int whole_rc = zs_twin_inflate(exact.get(), comp.size(), round, checksum, 0, whole, &whole_off);
                const int rc = zs_twin_inflate_sliding(exact.get(), comp.size(), round, checksum, stats, &off, slide);
                ++cases;
                bool good = rc == whole_rc && (rc == 0 || off == whole_off);
                if (accept) {
                    std::vector<uint8_t> out(zs_twin_result(nullptr));
                    zs_twin_result(out.data());
                    good = good && rc == 0 && out == want && !memcmp(stats, whole, sizeof stats) && slide[0] == stats[7] && slide[2] <= slide[1] + want.size();
                } else good = good && (rc == status || (!checksum && status == ZS_E_CHECKSUM && rc == 0));
                if (!good) { fprintf(stderr, "zstd_slide_check: %s round %llu checksum %d: rc %d (offset %llu), whole text rc %d (offset %llu)\n", name.c_str(), (unsigned long long)round, checksum, rc, (unsigned long long)off, whole_rc, (unsigned long long)whole_off); ++bad; }
            }
    }
    for (const std::string &name : edits) {
        std::vector<uint8_t> comp;
        if (!slurp(dir + "/" + name, comp)) { ++bad; continue; }
        std::unique_ptr<uint8_t[]> exact(new uint8_t[comp.size() ? comp.size() : 1]);
        if (!comp.empty()) memcpy(exact.get(), comp.data(), comp.size());
        uint64_t off = 0;
        (void)zs_twin_inflate_sliding(exact.get(), comp.size(), 1 + cases % 3, 1, nullptr, &off, nullptr);
        ++cases;
    }
    printf("zstd_slide_check: %s, %llu runs over %zu streams and %zu edited streams, %llu differ\n", bad ? "FAILED" : "ok", (unsigned long long)cases, names.size(), edits.size(),
           (unsigned long long)bad);
    return bad ? 1 : 0;
}
