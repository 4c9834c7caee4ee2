// cram_check.cpp -- the host twin of the CRAM device ingest as a stand-alone program, for a sanitizer build:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o cram_check tools/cram_check.cpp -lz -ldl
//   ./cram_check DIR
// DIR holds s_<method>_<name>.in / .out pairs (one rANS stream as a CRAM block body and its plain bytes) and f_<name>.cram files
// (tests/test_cram_twin.py dumps them).  Every stream goes through the twin's batch decode alone and must give its plain bytes;
// every file goes through the walk and the rounds, whole and one block a round, and must either be refused or give the bases the host
// reader gives (both run here: lrge::io::cram::parse).  Every buffer the block decode touches is a heap block of its exact size
// (cram_twin.cpp), so a step outside one ends the run.  Exit code 0: all held.
#include <dirent.h>

#include <cstdio>
#include <string>
#include <vector>

#include "../lrge_amd/csrc/cram_twin.cpp"

static std::string slurp(const std::string &p) { return lrge::io::slurp(p); }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: cram_check DIR\n"); return 2; }
    const std::string dir = argv[1];
    std::vector<std::string> names;
    if (DIR *d = opendir(dir.c_str())) {
        while (dirent *e = readdir(d)) names.push_back(e->d_name);
        closedir(d);
    }
    int streams = 0, files = 0, refused = 0, bad = 0;
    for (const std::string &n : names) {
        if (n.size() > 5 && n.compare(0, 2, "s_") == 0 && n.compare(n.size() - 3, 3, ".in") == 0) {
            const std::string comp = slurp(dir + "/" + n), plain = slurp(dir + "/" + n.substr(0, n.size() - 3) + ".out");
            cram_twin_stream s{0, (uint32_t)comp.size(), (uint32_t)plain.size(), (uint32_t)atoi(n.c_str() + 2), 0};
            std::vector<uint8_t> out(plain.size() + 1);
            uint64_t st[CRAM_STAT_WORDS];
            const int rc = cram_twin_rans_decode((const uint8_t *)comp.data(), comp.size(), &s, 1, out.data(), plain.size(), 0, st);
            if (rc || s.status || memcmp(out.data(), plain.data(), plain.size()) != 0) { printf("STREAM %s: rc %d status %u %s\n", n.c_str(), rc, s.status, cram_twin_why()); ++bad; }
            ++streams;
        } else if (n.size() > 7 && n.compare(0, 2, "f_") == 0) {
            const std::string file = slurp(dir + "/" + n);
            std::vector<std::pair<std::string, std::string>> host;
            bool host_ok = true;
            try {
                const std::string data = lrge::io::decompress(file);
                if (lrge::io::sniff(data) != lrge::io::Kind::Cram) host_ok = false;
                else lrge::io::cram::parse(data, [&](const std::string &a, const std::string &b) { host.emplace_back(a, b); }, lrge::io::MAPPED_MSG);
            } catch (const std::exception &) { host_ok = false; }
            for (uint64_t round_bytes : {(uint64_t)0, (uint64_t)1}) {
                uint64_t st[CRAM_STAT_WORDS];
                if (cram_twin_open((const uint8_t *)file.data(), file.size(), round_bytes, 0, st)) { ++refused; continue; }
                const uint64_t k = cram_twin_count();
                std::vector<uint32_t> len(k + 1);
                std::vector<uint64_t> noff(k + 1), boff(k + 1);
                std::string nm(cram_twin_name_bytes() + 1, '\0');
                std::vector<uint8_t> bases(cram_twin_base_bytes() + 1);
                cram_twin_table(len.data(), noff.data(), &nm[0], boff.data(), bases.data());
                bool same = host_ok && k == host.size();
                for (uint64_t i = 0; same && i < k; ++i)
                    same = host[i].first == nm.substr(noff[i], noff[i + 1] - noff[i]) && host[i].second == std::string((const char *)bases.data() + boff[i], len[i]);
                if (!same) { printf("FILE %s: the twin's records are not the host reader's\n", n.c_str()); ++bad; }
            }
            ++files;
        }
    }
    printf("%d streams ok, %d files walked (%d opens refused), %d bad\n", streams, files, refused, bad);
    return bad ? 1 : (streams && files ? 0 : 3);
}
