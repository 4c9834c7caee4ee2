// window_twin_check.cpp -- a stand-alone driver of the windowed host twins (csrc/fastx_twin.cpp, csrc/bam_twin.cpp,
// csrc/sam_twin.cpp over csrc/win_twin.h) for runs under the host sanitizers, which cannot see code loaded into an interpreter:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lrge_amd/csrc tools/window_twin_check.cpp -o window_twin_check
//   ./window_twin_check case1.bam case2.sam case3.fq ...
// Every *.bam file goes through bam_twin_windowed at segments 64, 257 and 4096, every *.sam file through sam_twin_windowed, every
// other file through fastx_twin_windowed at tiles 64 and 4096, at windows 64, 257, 3001 and 20000 and pieces 1, 61, the window and
// the whole text; a window above the text must give the resident twin's record count.  Every FASTA / FASTQ run is followed by the
// two passes of the selected ingest (fastx_twin_census, fastx_twin_selected) on the same text, window and piece.  Prints the verdict counts; the exit
// status is 1 when the verdicts of one file disagree.
// TEST INFRASTRUCTURE, not part of the product library.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../lrge_amd/csrc/fastx_twin.cpp"
#include "../lrge_amd/csrc/bam_twin.cpp"
#include "../lrge_amd/csrc/sam_twin.cpp"

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    uint8_t buf[1 << 16];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

// The two passes of the selected ingest over a FASTA / FASTQ text whose windowed run gave verdict `rc` and table `all`: the
// census has the same verdict and counts its records and bases; every third record, the first and the last selected give the
// same verdict and those records; a selection past the end is invalid.  Returns the disagreements
static uint64_t fastx_selected(const char *path, const std::vector<uint8_t> &t, uint64_t tile, uint64_t window, uint64_t piece, int rc, const std::vector<FxRec> &all) {
    uint64_t bad = 0, bases = 0, cs[4], ss[4];
    for (const FxRec &r : all) bases += r.seq_len;
    const auto fail = [&](const char *what) { ++bad; fprintf(stderr, "%s: tile %llu window %llu piece %llu: %s\n", path, (unsigned long long)tile, (unsigned long long)window, (unsigned long long)piece, what); };
    const int crc = fastx_twin::fastx_twin_census(t.data(), t.size(), tile, window, piece, cs);
    if (crc != rc || (!rc && (cs[0] != all.size() || cs[1] != bases || cs[2] != t.size()))) fail("the census disagrees with the windowed run");
    std::vector<uint32_t> sel;
    for (uint64_t i = 0; i < all.size(); ++i) if (i % 3 == 0 || i + 1 == all.size()) sel.push_back((uint32_t)i);
    const int src = fastx_twin::fastx_twin_selected(t.data(), t.size(), tile, window, piece, sel.data(), sel.size());
    if (src != rc) fail("the selected run has another verdict");
    if (!src) {
        const uint64_t k = fastx_twin::fastx_twin_windowed_count();
        std::vector<FxRec> tab(k);
        fastx_twin::fastx_twin_windowed_table(tab.data());
        fastx_twin::fastx_twin_select_stats(ss);
        uint64_t kept = 0;
        bool same = k == sel.size();
        for (uint64_t j = 0; j < k && same; ++j) {
            std::vector<uint8_t> out(tab[j].seq_len + 1);
            same = tab[j].name_off == all[sel[j]].name_off && tab[j].seq_len == all[sel[j]].seq_len && fastx_twin::fastx_twin_windowed_seq(j, out.data()) == tab[j].seq_len;
            kept += tab[j].seq_len;
        }
        if (!same || ss[0] != all.size() || ss[1] != k || ss[2] != bases || ss[3] != kept) fail("the selected run kept other records");
        sel.push_back((uint32_t)all.size());
        if (fastx_twin::fastx_twin_selected(t.data(), t.size(), tile, window, piece, sel.data(), sel.size()) != WIN_TWIN_INVALID) fail("an ordinal past the records is not invalid");
    }
    return bad;
}

int main(int argc, char **argv) {
    const uint64_t windows[] = {64, 257, 3001, 20000}, segs[] = {64, 257, 4096}, tiles[] = {64, 4096};
    uint64_t runs = 0, proven = 0, bad = 0;
    for (int a = 1; a < argc; ++a) {
        const std::string path = argv[a];
        const auto ends = [&](const char *x) { return path.size() > 4 && path.compare(path.size() - 4, 4, x) == 0; };
        const bool is_bam = ends(".bam"), is_sam = ends(".sam");
        const std::vector<uint8_t> t = slurp(argv[a]);
        const uint64_t n = t.size();
        int first = -100;
        uint64_t first_count = 0;
        // (S: the segment of BAM, the tile of FASTA / FASTQ; SAM has neither and runs once)
        const std::vector<uint64_t> params = is_bam ? std::vector<uint64_t>(segs, segs + 3) : is_sam ? std::vector<uint64_t>(1, 0) : std::vector<uint64_t>(tiles, tiles + 2);
        for (uint64_t S : params) {
            for (uint64_t w = 0; w <= 4; ++w) {
                const uint64_t window = w < 4 ? windows[w] : n + 1;
                const uint64_t pieces[] = {1, 61, window, n ? n : 1};
                for (uint64_t piece : pieces) {
                    const int rc = is_bam ? bam_twin::bam_twin_windowed(t.data(), n, S, window, piece) : is_sam ? sam_twin::sam_twin_windowed(t.data(), n, window, piece)
                                                                                                                 : fastx_twin::fastx_twin_windowed(t.data(), n, S, window, piece);
                    const uint64_t count = (is_bam ? bam_twin::bam_twin_windowed_count : is_sam ? sam_twin::sam_twin_windowed_count : fastx_twin::fastx_twin_windowed_count)();
                    std::vector<FxRec> tab(count);
                    (is_bam ? bam_twin::bam_twin_windowed_table : is_sam ? sam_twin::sam_twin_windowed_table : fastx_twin::fastx_twin_windowed_table)(tab.data());
                    for (uint64_t i = 0; i < count && i <= 50; ++i) {          // the decode of every record reads the store
                        std::vector<uint8_t> out(tab[i].seq_len + 1);
                        if (is_bam) bam_twin::bam_twin_windowed_seq(i, (uint32_t)i & 3, out.data());
                        else (is_sam ? sam_twin::sam_twin_windowed_seq : fastx_twin::fastx_twin_windowed_seq)(i, out.data());
                    }
                    if (!is_bam && !is_sam) bad += fastx_selected(argv[a], t, S, window, piece, rc, tab);
                    ++runs; proven += rc == 0;
                    if (first == -100) { first = rc; first_count = count; }
                    else if (rc != first || count != first_count) { ++bad; fprintf(stderr, "%s: S %llu window %llu piece %llu: verdict %d, %llu records; first %d, %llu\n", argv[a], (unsigned long long)S, (unsigned long long)window, (unsigned long long)piece, rc, (unsigned long long)count, first, (unsigned long long)first_count); }
                }
            }
        }
    }
    printf("%llu runs, %llu proven, %llu disagreements\n", (unsigned long long)runs, (unsigned long long)proven, (unsigned long long)bad);
    return bad != 0;
}
