// xz_check.cpp -- a stand-alone driver of the xz decode's host twin (csrc/xz_twin.cpp over csrc/xz_round.h and
// csrc/xz_core.h) for runs under the host sanitizers, which cannot see code loaded into an interpreter:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lrge_amd/csrc tools/xz_check.cpp -o xz_check
//   ./xz_check DIR
// DIR holds cases written by tests/test_xz_twin.py: NAME.xz beside NAME.plain (the text liblzma gives: the twin must give it at
// rounds of 0, 1 and 2 blocks, at one chunk per launch and at the default, with and without the checks) or beside NAME.status (the decimal XZ_E_* status the twin must
// refuse it with); NAME.edit holds a stream with a damaged byte, which the twin may take or refuse.  Every input is passed in a
// heap block of its exact size, so a load outside it is reported.  The exit status is 1 when a case differs.
// TEST INFRASTRUCTURE, not part of the product library.
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <string>
#include <vector>

#include "../lrge_amd/csrc/xz_twin.cpp"

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
    if (argc != 2) { fprintf(stderr, "usage: xz_check DIR\n"); return 2; }
    const std::string dir = argv[1];
    DIR *d = opendir(dir.c_str());
    if (!d) { fprintf(stderr, "xz_check: cannot open %s\n", dir.c_str()); return 2; }
    std::vector<std::string> names, edits;
    while (dirent *e = readdir(d)) {
        const std::string n = e->d_name;
        if (ends_with(n, ".xz")) names.push_back(n.substr(0, n.size() - 3));
        if (ends_with(n, ".edit")) edits.push_back(n);
    }
    closedir(d);
    uint64_t cases = 0, bad = 0;
    for (const std::string &name : names) {
        std::vector<uint8_t> comp, want;
        if (!slurp(dir + "/" + name + ".xz", comp)) { ++bad; continue; }
        std::unique_ptr<uint8_t[]> exact(new uint8_t[comp.size() ? comp.size() : 1]);
        if (!comp.empty()) memcpy(exact.get(), comp.data(), comp.size());
        const bool accept = slurp(dir + "/" + name + ".plain", want);
        int status = 0;
        if (!accept) {
            std::vector<uint8_t> s;
            if (!slurp(dir + "/" + name + ".status", s)) { fprintf(stderr, "xz_check: %s has neither .plain nor .status\n", name.c_str()); ++bad; continue; }
            status = atoi(std::string(s.begin(), s.end()).c_str());
        }
        for (uint64_t round = 0; round < 3; ++round)
            for (int check = 1; check >= 0; --check) {
                uint64_t stats[8], off = 0;
                const uint64_t launch = (round + check) & 1;            // one chunk per launch, or the default
                const int rc = xz_twin_inflate(exact.get(), comp.size(), round, launch, check, 0, 0, stats, &off);
                ++cases;
                bool good;
                if (accept) {
                    std::vector<uint8_t> out(xz_twin_result(nullptr));
                    xz_twin_result(out.data());
                    good = rc == 0 && out == want && stats[7] == want.size();
                } else good = rc == status || (!check && status == XZ_E_CHECK && rc == 0);
                if (!good) { fprintf(stderr, "xz_check: %s round %llu check %d: rc %d (offset %llu)\n", name.c_str(), (unsigned long long)round, check, rc, (unsigned long long)off); ++bad; }
            }
    }
    for (const std::string &name : edits) {
        std::vector<uint8_t> comp;
        if (!slurp(dir + "/" + name, comp)) { ++bad; continue; }
        std::unique_ptr<uint8_t[]> exact(new uint8_t[comp.size() ? comp.size() : 1]);
        if (!comp.empty()) memcpy(exact.get(), comp.data(), comp.size());
        uint64_t off = 0;
        (void)xz_twin_inflate(exact.get(), comp.size(), cases % 3, cases % 2, 1, 0, 0, nullptr, &off);
        ++cases;
    }
    printf("xz_check: %s, %llu runs over %zu streams and %zu edited streams, %llu differ\n", bad ? "FAILED" : "ok", (unsigned long long)cases, names.size(), edits.size(),
           (unsigned long long)bad);
    return bad ? 1 : 0;
}
