// cram_check.cpp -- the host twin of the CRAM device ingest as a stand-alone program, for a sanitizer build:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o cram_check tools/cram_check.cpp -lz -ldl
//   ./cram_check DIR
// DIR holds s_<method>_<name>.in / .out pairs (one rANS stream as a CRAM block body and its plain bytes) and f_<name>.cram files
// (tests/test_cram_twin.py dumps them).  Every stream goes through the twin's batch decode alone and must give its plain bytes;
// every file goes through the walk and the rounds, whole and one block a round, and must either be refused or give the bases the host
// reader gives (both run here: lrge::io::cram::parse).  Every buffer the block decode touches is a heap block of its exact size
// (cram_twin.cpp), so a step outside one ends the run.  Every file that opens also goes through the four calls of the sampled ingest
// (cram_twin_sampled) -- the census, every third read and the last selected, the census with a map and the mapped
// open of the same reads -- whose round scratch is a heap block of exactly the round's raw size and whose store one of exactly the
// chosen bases: the kept reads must be the host reader's.  Exit code 0: all held.
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
    int streams = 0, files = 0, refused = 0, bad = 0, sampled = 0;
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
                // the sampled ingest of the same file at the same round size
                std::vector<uint32_t> sel;
                for (uint64_t i = 0; i < k; ++i) if (i % 3 == 0 || i + 1 == k) sel.push_back((uint32_t)i);
                uint64_t cs[4];
                const uint8_t *fd = (const uint8_t *)file.data();
                if (!same || cram_twin_sampled(0, fd, file.size(), nullptr, 0, round_bytes, 0, 0, cs) || cs[0] != k || cs[1] != cram_twin_base_bytes() ||
                    cram_twin_sampled(2, fd, file.size(), nullptr, 0, round_bytes, 0, 0, cs) || cs[0] != k) { printf("FILE %s: the census disagrees with the open\n", n.c_str()); ++bad; continue; }
                for (int what : {1, 3}) {
                    bool kept_same = cram_twin_sampled(what, fd, file.size(), sel.data(), sel.size(), round_bytes, 0, 0, cs) == 0 && cram_twin_kept() == sel.size();
                    if (kept_same) {
                        std::vector<uint32_t> sl(sel.size() + 1);
                        std::vector<uint64_t> so(sel.size() + 1), sb(sel.size() + 1);
                        std::string sn(cram_twin_kept_name_bytes() + 1, '\0');
                        uint64_t stats[CRAM_STAT_WORDS], seek[4], mem[4];
                        cram_twin_sampled_stats(stats, seek, mem);
                        std::vector<uint8_t> store(mem[0] + 1);
                        cram_twin_kept_table(sel.data(), sl.data(), so.data(), &sn[0], sb.data(), store.data());
                        for (uint64_t j = 0; kept_same && j < sel.size(); ++j)
                            kept_same = host[sel[j]].first == sn.substr(so[j], so[j + 1] - so[j]) && host[sel[j]].second == std::string((const char *)store.data() + sb[j], sl[j]);
                    }
                    if (!kept_same) { printf("FILE %s: the %s open's reads are not the host reader's\n", n.c_str(), what == 1 ? "selected" : "mapped"); ++bad; }
                    else ++sampled;
                }
            }
            ++files;
        }
    }
    printf("%d streams ok, %d files walked (%d opens refused), %d sampled opens ok, %d bad\n", streams, files, refused, sampled, bad);
    return bad ? 1 : (streams && files ? 0 : 3);
}
