// window_twin_check.cpp -- a stand-alone driver of the windowed host twins (csrc/fastx_twin.cpp, csrc/bam_twin.cpp,
// csrc/sam_twin.cpp over csrc/win_twin.h) for runs under the host sanitizers, which cannot see code loaded into an interpreter:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lrge_amd/csrc tools/window_twin_check.cpp -o window_twin_check
//   ./window_twin_check case1.bam case2.sam case3.fq ...
// Every *.bam file goes through bam_twin_windowed at segments 64, 257 and 4096, every *.sam file through sam_twin_windowed, every
// other file through fastx_twin_windowed at tiles 64 and 4096, at windows 64, 257, 3001 and 20000 and pieces 1, 61, the window and
// the whole text; a window above the text must give the resident twin's record count.  Prints the verdict counts; the exit
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
