// window_twin_check.cpp -- a stand-alone driver of the windowed host twins (csrc/fastx_twin.cpp, csrc/bam_twin.cpp,
// csrc/sam_twin.cpp over csrc/win_twin.h) for runs under the host sanitizers, which cannot see code loaded into an interpreter:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lrge_amd/csrc tools/window_twin_check.cpp -o window_twin_check
//   ./window_twin_check case1.bam case2.sam case3.fq ...
// Every *.bam file goes through bam_twin_windowed at segments 64, 257 and 4096, every *.sam file through sam_twin_windowed, every
// other file through fastx_twin_windowed at tiles 64 and 4096, at windows 64, 257, 3001 and 20000 and pieces 1, 61, the window and
// the whole text; a window above the text must give the resident twin's record count.  Every FASTA / FASTQ run is followed by the
// two passes of the selected ingest (fastx_twin_census, fastx_twin_selected) on the same text, window and piece, and by the seek map
// (fastx_twin_census_map at strides 1, 64, 3000 and above the text, fastx_twin_seek_plan for the plain text and for BGZF blocks of 3000 text
// bytes, fastx_twin_mapped).  Every BAM run is followed by the same passes of its own twin (bam_twin_census, bam_twin_selected,
// bam_twin_census_map at strides 1, 36, 3000 and above the text, bam_twin_seek_plan, bam_twin_mapped), every SAM run by those of sam_twin.cpp (sam_twin_census, sam_twin_selected,
// sam_twin_census_map at strides 1, 64, 3000 and above the text, sam_twin_seek_plan, sam_twin_mapped).  Prints the
// Every *.gz file (plain or multi-member gzip of FASTA / FASTQ) goes through the seek map of gzip: fastx_twin_gz_census_map
// at chunks 64 and 1024 and spacings 1, 4096 and above the text, every entry decoded alone from its seed at the four staging skews against its
// slice of the text, the plan, and fastx_twin_gz_mapped against fastx_twin_selected on the text.
// Every *.bz2 file goes through the seek map of bzip2: fastx_twin_bz_census_map at rounds of 1 block and of all and
// spacings 1, 4096 and above the text, every block entered at every mark alone and by all lanes at the four staging skews against its
// slice of the text, the plan, and fastx_twin_bz_mapped against fastx_twin_selected on the text.  Prints the
// verdict counts; the exit status is 1 when the verdicts of one file disagree.
// TEST INFRASTRUCTURE, not part of the product library.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
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

// The seek map over a text whose windowed run gave verdict `rc` and table `all` (name_off in the whole text): the census with a map
// has the same verdict and counts; its points are strictly ascending records of `all` at their header bytes, the first record 0; the
// plan of every third record and the last brings whole runs, for the plain text and for made-up BGZF blocks of 3000 text bytes;
// the mapped run gives the records of the selected run.  Returns the disagreements
static uint64_t fastx_seek(const char *path, const std::vector<uint8_t> &t, uint64_t tile, uint64_t window, uint64_t piece, int rc, const std::vector<FxRec> &all) {
    uint64_t bad = 0;
    const auto fail = [&](const char *what, uint64_t stride) { ++bad; fprintf(stderr, "%s: tile %llu window %llu piece %llu stride %llu: %s\n", path, (unsigned long long)tile, (unsigned long long)window, (unsigned long long)piece, (unsigned long long)stride, what); };
    const uint64_t strides[] = {1, 64, 3000, (uint64_t)t.size() + 1};
    for (uint64_t stride : strides) {
        uint64_t cs[4], ps[4];
        const int crc = fastx_twin::fastx_twin_census_map(t.data(), t.size(), tile, window, piece, stride, cs);
        if (crc != rc || (!rc && cs[0] != all.size())) { fail("the census with a map disagrees with the windowed run", stride); continue; }
        if (rc) continue;
        const uint64_t np = fastx_twin::fastx_twin_map_points(nullptr, nullptr, 0);
        std::vector<uint64_t> ord(np + 1), off(np + 1);
        fastx_twin::fastx_twin_map_points(ord.data(), off.data(), np);
        bool good = all.empty() ? np == 0 : np > 0 && ord[0] == 0;
        for (uint64_t i = 0; i < np && good; ++i) good = ord[i] < all.size() && off[i] == all[ord[i]].name_off - 1 && (!i || (ord[i] > ord[i - 1] && off[i] / stride > off[i - 1] / stride));
        if (!good) { fail("the points are not first record starts of their cells", stride); continue; }
        std::vector<uint32_t> sel;
        for (uint64_t i = 0; i < all.size(); ++i) if (i % 3 == 0 || i + 1 == all.size()) sel.push_back((uint32_t)i);
        // the plan on the plain text, and on blocks of 3000 text bytes whose members are 100 bytes longer than half their text
        if (fastx_twin::fastx_twin_seek_plan(nullptr, nullptr, 0, 0, sel.data(), sel.size(), ps) || ps[1] > t.size() || ps[1] != ps[2] || ps[3]) fail("the plan of the plain text", stride);
        std::vector<uint32_t> c_len, isize;
        uint64_t file_len = 0;
        for (uint64_t o = 0; o < t.size(); o += 3000) { isize.push_back((uint32_t)std::min<uint64_t>(3000, t.size() - o)); c_len.push_back(isize.back() / 2 + 100); file_len += c_len.back(); }
        isize.push_back(0); c_len.push_back(28); file_len += 28;    // (the empty block at the end of a BGZF file)
        uint64_t bs[4];
        if (fastx_twin::fastx_twin_seek_plan(c_len.data(), isize.data(), c_len.size(), file_len, sel.data(), sel.size(), bs) || bs[0] != ps[0] || bs[1] != ps[1] || bs[2] > file_len ||
            bs[3] > c_len.size() || (!sel.empty() && (!bs[3] || bs[2] < 28)))
            fail("the plan of the BGZF blocks", stride);
        const int mrc = fastx_twin::fastx_twin_mapped(t.data(), t.size(), tile, window, piece, sel.data(), sel.size());
        if (mrc) { fail("the mapped run is not proven", stride); continue; }
        const uint64_t k = fastx_twin::fastx_twin_windowed_count();
        std::vector<FxRec> tab(k);
        fastx_twin::fastx_twin_windowed_table(tab.data());
        bool same = k == sel.size();
        for (uint64_t j = 0; j < k && same; ++j) {
            std::vector<uint8_t> out(tab[j].seq_len + 1);
            same = tab[j].name_off == all[sel[j]].name_off && tab[j].seq_len == all[sel[j]].seq_len && fastx_twin::fastx_twin_windowed_seq(j, out.data()) == tab[j].seq_len;
        }
        if (!same) fail("the mapped run kept other records", stride);
        sel.push_back((uint32_t)all.size());
        if (fastx_twin::fastx_twin_mapped(t.data(), t.size(), tile, window, piece, sel.data(), sel.size()) != WIN_TWIN_INVALID) fail("an ordinal past the records is not invalid", stride);
    }
    return bad;
}

// The sampled ingest of a BAM text whose windowed run gave verdict `rc` and table `all` (name_off in the whole text): census and
// selection as fastx_selected checks them (the store holds packed bytes), then the map -- its points are records' block_size fields,
// the first record 0 --, the plan on the plain text and on made-up BGZF blocks, and the mapped run, which gives the selected run's
// records and store.  Returns the disagreements
static uint64_t bam_sampled(const char *path, const std::vector<uint8_t> &t, uint64_t S, uint64_t window, uint64_t piece, int rc, const std::vector<FxRec> &all) {
    using namespace bam_twin;
    uint64_t bad = 0, bases = 0, cs[4], ss[4];
    for (const FxRec &r : all) bases += r.seq_len;
    const auto fail = [&](const char *what, uint64_t stride) { ++bad; fprintf(stderr, "%s: S %llu window %llu piece %llu stride %llu: %s\n", path, (unsigned long long)S, (unsigned long long)window, (unsigned long long)piece, (unsigned long long)stride, what); };
    const int crc = bam_twin_census(t.data(), t.size(), S, window, piece, cs);
    if (crc != rc || (!rc && (cs[0] != all.size() || cs[1] != bases || cs[2] != t.size()))) fail("the census disagrees with the windowed run", 0);
    std::vector<uint32_t> sel;
    for (uint64_t i = 0; i < all.size(); ++i) if (i % 3 == 0 || i + 1 == all.size()) sel.push_back((uint32_t)i);
    // the table and the store of the run that just ended against the selection; `store`: filled, or compared when it is given filled
    std::vector<uint8_t> store;
    const auto kept_right = [&](bool compare) {
        const uint64_t k = bam_twin_windowed_count();
        std::vector<FxRec> tab(k);
        bam_twin_windowed_table(tab.data());
        bam_twin_windowed_select_stats(ss);
        uint64_t kept = 0, span = 0;
        bool same = k == sel.size();
        for (uint64_t j = 0; j < k && same; ++j) {
            std::vector<uint8_t> out(tab[j].seq_len + 1);
            same = tab[j].name_off == all[sel[j]].name_off && tab[j].seq_len == all[sel[j]].seq_len && tab[j].seq_off == span && tab[j].seq_span == ((uint64_t)tab[j].seq_len + 1) / 2 &&
                   bam_twin_windowed_seq(j, (uint32_t)j & 3, out.data()) == tab[j].seq_len;
            kept += tab[j].seq_len; span += tab[j].seq_span;
        }
        std::vector<uint8_t> st(bam_twin_windowed_store(nullptr) + 1);
        st.resize(bam_twin_windowed_store(st.data()));
        if (compare) same = same && st == store; else store = st;
        return same && st.size() == span && ss[0] == all.size() && ss[1] == k && ss[2] == bases && ss[3] == kept;
    };
    const int src = bam_twin_selected(t.data(), t.size(), S, window, piece, sel.data(), sel.size());
    if (src != rc) fail("the selected run has another verdict", 0);
    if (src || rc) return bad;
    if (!kept_right(false)) fail("the selected run kept other records", 0);
    sel.push_back((uint32_t)all.size());
    if (bam_twin_selected(t.data(), t.size(), S, window, piece, sel.data(), sel.size()) != WIN_TWIN_INVALID) fail("an ordinal past the records is not invalid", 0);
    sel.pop_back();
    const uint64_t strides[] = {1, 36, 3000, (uint64_t)t.size() + 1};
    for (uint64_t stride : strides) {
        uint64_t ps[4], bs[4];
        if (bam_twin_census_map(t.data(), t.size(), S, window, piece, stride, cs) || cs[0] != all.size() || cs[1] != bases) { fail("the census with a map disagrees with the windowed run", stride); continue; }
        const uint64_t np = bam_twin_map_points(nullptr, nullptr, 0);
        std::vector<uint64_t> ord(np + 1), off(np + 1);
        bam_twin_map_points(ord.data(), off.data(), np);
        bool good = all.empty() ? np == 0 : np > 0 && ord[0] == 0;
        for (uint64_t i = 0; i < np && good; ++i) good = ord[i] < all.size() && off[i] == all[ord[i]].name_off - 36 && (!i || (ord[i] > ord[i - 1] && off[i] / stride > off[i - 1] / stride));
        if (!good) { fail("the points are not first record starts of their cells", stride); continue; }
        if (bam_twin_seek_plan(nullptr, nullptr, 0, 0, sel.data(), sel.size(), ps) || ps[1] > t.size() || ps[1] != ps[2] || ps[3]) fail("the plan of the plain text", stride);
        std::vector<uint32_t> c_len, isize;
        uint64_t file_len = 0;
        for (uint64_t o = 0; o < t.size(); o += 3000) { isize.push_back((uint32_t)std::min<uint64_t>(3000, t.size() - o)); c_len.push_back(isize.back() / 2 + 100); file_len += c_len.back(); }
        isize.push_back(0); c_len.push_back(28); file_len += 28;    // (the empty block at the end of a BGZF file)
        if (bam_twin_seek_plan(c_len.data(), isize.data(), c_len.size(), file_len, sel.data(), sel.size(), bs) || bs[0] != ps[0] || bs[1] != ps[1] || bs[2] > file_len ||
            bs[3] > c_len.size() || (!sel.empty() && (!bs[3] || bs[2] < 28)))
            fail("the plan of the BGZF blocks", stride);
        if (bam_twin_mapped(t.data(), t.size(), S, window, piece, sel.data(), sel.size())) { fail("the mapped run is not proven", stride); continue; }
        if (!kept_right(true)) fail("the mapped run kept other records", stride);
        sel.push_back((uint32_t)all.size());
        if (bam_twin_mapped(t.data(), t.size(), S, window, piece, sel.data(), sel.size()) != WIN_TWIN_INVALID) fail("an ordinal past the records is not invalid", stride);
        sel.pop_back();
    }
    return bad;
}

// The sampled ingest of a SAM text whose windowed run gave verdict `rc` and table `all` (name_off in the whole text), as bam_sampled:
// census and selection (the store holds the chosen bases), then the map -- its points are first bytes of record lines, the first
// record 0 --, the plan on the plain text and on made-up BGZF blocks, and the mapped run, which gives the selected run's records and
// store.  Returns the disagreements
static uint64_t sam_sampled(const char *path, const std::vector<uint8_t> &t, uint64_t window, uint64_t piece, int rc, const std::vector<FxRec> &all) {
    using namespace sam_twin;
    uint64_t bad = 0, bases = 0, cs[4], ss[4];
    for (const FxRec &r : all) bases += r.seq_len;
    const auto fail = [&](const char *what, uint64_t stride) { ++bad; fprintf(stderr, "%s: window %llu piece %llu stride %llu: %s\n", path, (unsigned long long)window, (unsigned long long)piece, (unsigned long long)stride, what); };
    const int crc = sam_twin_census(t.data(), t.size(), window, piece, cs);
    if (crc != rc || (!rc && (cs[0] != all.size() || cs[1] != bases || cs[2] != t.size()))) fail("the census disagrees with the windowed run", 0);
    std::vector<uint32_t> sel;
    for (uint64_t i = 0; i < all.size(); ++i) if (i % 3 == 0 || i + 1 == all.size()) sel.push_back((uint32_t)i);
    std::vector<uint8_t> store;
    const auto kept_right = [&](bool compare) {
        const uint64_t k = sam_twin_windowed_count();
        std::vector<FxRec> tab(k);
        sam_twin_windowed_table(tab.data());
        sam_twin_windowed_select_stats(ss);
        uint64_t kept = 0;
        bool same = k == sel.size();
        for (uint64_t j = 0; j < k && same; ++j) {
            std::vector<uint8_t> out(tab[j].seq_len + 1);
            same = tab[j].name_off == all[sel[j]].name_off && tab[j].seq_len == all[sel[j]].seq_len && tab[j].seq_off == kept && tab[j].seq_span == tab[j].seq_len &&
                   sam_twin_windowed_seq(j, out.data()) == tab[j].seq_len;
            kept += tab[j].seq_len;
        }
        std::vector<uint8_t> st(sam_twin_windowed_store(nullptr) + 1);
        st.resize(sam_twin_windowed_store(st.data()));
        if (compare) same = same && st == store; else store = st;
        return same && st.size() == kept && ss[0] == all.size() && ss[1] == k && ss[2] == bases && ss[3] == kept;
    };
    const int src = sam_twin_selected(t.data(), t.size(), window, piece, sel.data(), sel.size());
    if (src != rc) fail("the selected run has another verdict", 0);
    if (src || rc) return bad;
    if (!kept_right(false)) fail("the selected run kept other records", 0);
    sel.push_back((uint32_t)all.size());
    if (sam_twin_selected(t.data(), t.size(), window, piece, sel.data(), sel.size()) != WIN_TWIN_INVALID) fail("an ordinal past the records is not invalid", 0);
    sel.pop_back();
    const uint64_t strides[] = {1, 64, 3000, (uint64_t)t.size() + 1};
    for (uint64_t stride : strides) {
        uint64_t ps[4], bs[4];
        if (sam_twin_census_map(t.data(), t.size(), window, piece, stride, cs) || cs[0] != all.size() || cs[1] != bases) { fail("the census with a map disagrees with the windowed run", stride); continue; }
        const uint64_t np = sam_twin_map_points(nullptr, nullptr, 0);
        std::vector<uint64_t> ord(np + 1), off(np + 1);
        sam_twin_map_points(ord.data(), off.data(), np);
        bool good = all.empty() ? np == 0 : np > 0 && ord[0] == 0;
        for (uint64_t i = 0; i < np && good; ++i) good = ord[i] < all.size() && off[i] == all[ord[i]].name_off && (!i || (ord[i] > ord[i - 1] && off[i] / stride > off[i - 1] / stride));
        if (!good) { fail("the points are not first record starts of their cells", stride); continue; }
        if (sam_twin_seek_plan(nullptr, nullptr, 0, 0, sel.data(), sel.size(), ps) || ps[1] > t.size() || ps[1] != ps[2] || ps[3]) fail("the plan of the plain text", stride);
        std::vector<uint32_t> c_len, isize;
        uint64_t file_len = 0;
        for (uint64_t o = 0; o < t.size(); o += 3000) { isize.push_back((uint32_t)std::min<uint64_t>(3000, t.size() - o)); c_len.push_back(isize.back() / 2 + 100); file_len += c_len.back(); }
        isize.push_back(0); c_len.push_back(28); file_len += 28;    // (the empty block at the end of a BGZF file)
        if (sam_twin_seek_plan(c_len.data(), isize.data(), c_len.size(), file_len, sel.data(), sel.size(), bs) || bs[0] != ps[0] || bs[1] != ps[1] || bs[2] > file_len ||
            bs[3] > c_len.size() || (!sel.empty() && (!bs[3] || bs[2] < 28)))
            fail("the plan of the BGZF blocks", stride);
        if (sam_twin_mapped(t.data(), t.size(), window, piece, sel.data(), sel.size())) { fail("the mapped run is not proven", stride); continue; }
        if (!kept_right(true)) fail("the mapped run kept other records", stride);
        sel.push_back((uint32_t)all.size());
        if (sam_twin_mapped(t.data(), t.size(), window, piece, sel.data(), sel.size()) != WIN_TWIN_INVALID) fail("an ordinal past the records is not invalid", stride);
        sel.pop_back();
    }
    return bad;
}

// The seek map of a gzip file: returns the disagreements
static uint64_t gzip_seek(const char *path, const std::vector<uint8_t> &d) {
    uint64_t bad = 0;
    const auto fail = [&](const char *what, uint64_t chunk, uint64_t spacing) { ++bad; fprintf(stderr, "%s: gzip seek, chunk %llu spacing %llu: %s\n", path, (unsigned long long)chunk, (unsigned long long)spacing, what); };
    for (uint64_t chunk : {(uint64_t)64, (uint64_t)1024})
        for (uint64_t sp = 0; sp < 3; ++sp) {
            uint64_t cs[4];
            uint64_t spacing = sp == 0 ? 1 : 4096;
            int rc = fastx_twin::fastx_twin_gz_census_map(d.data(), d.size(), chunk, (uint64_t)256 << 20, 64, spacing, 64, 3001, 4096, 512, cs);
            if (sp == 2) { spacing = fastx_twin::fastx_twin_gz_text(nullptr) + 1; rc = fastx_twin::fastx_twin_gz_census_map(d.data(), d.size(), chunk, (uint64_t)256 << 20, 64, spacing, 64, 3001, 4096, 512, cs); }
            std::vector<uint8_t> text((size_t)fastx_twin::fastx_twin_gz_text(nullptr) + 1);
            const uint64_t n = fastx_twin::fastx_twin_gz_text(text.data());
            const uint64_t ne = fastx_twin::fastx_twin_gz_entries(nullptr, 0);
            std::vector<uint64_t> ent(6 * ne + 6);
            fastx_twin::fastx_twin_gz_entries(ent.data(), ne);
            if (!ne || ent[0] || ent[1]) { fail("entry 0 is not the start of the file", chunk, spacing); continue; }
            for (uint64_t i = 0; i < ne; ++i) {
                const uint64_t off = ent[6 * i + 1], len = ent[6 * i + 2];
                if (off + len > n || (i + 1 < ne && ent[6 * i + 7] != off + len) || (i + 1 == ne && off + len != n)) { fail("the entries do not tile the text", chunk, spacing); break; }
                std::vector<uint8_t> out((size_t)len + 1);
                for (uint32_t skew = 0; skew < 4; ++skew)
                    if (fastx_twin::fastx_twin_gz_entry(d.data(), d.size(), i, skew, out.data()) || memcmp(out.data(), text.data() + off, (size_t)len)) { fail("an entry decoded from its seed is not its text", chunk, spacing); break; }
            }
            if (rc) continue;                      // (a text that is no FASTA / FASTQ: the entries are the gzip side's alone)
            std::vector<uint32_t> sel;
            for (uint64_t i = 0; i < cs[0]; i += 3) sel.push_back((uint32_t)i);
            if (cs[0] && sel.back() != cs[0] - 1) sel.push_back((uint32_t)(cs[0] - 1));
            uint64_t ps[4], ms[4];
            if (fastx_twin::fastx_twin_seek_plan(nullptr, nullptr, 0, 0, sel.data(), sel.size(), ps) || ps[1] > n || ps[2] > d.size() || ps[3] > ne) fail("the plan", chunk, spacing);
            if (fastx_twin::fastx_twin_gz_mapped(d.data(), d.size(), 64, 3001, 4096, sel.data(), sel.size())) { fail("the mapped pass is not proven", chunk, spacing); continue; }
            fastx_twin::fastx_twin_plan_stats(ms);
            if (memcmp(ps, ms, sizeof ps)) fail("the mapped pass brought something else than the plan", chunk, spacing);
            const uint64_t k = fastx_twin::fastx_twin_windowed_count();
            std::vector<FxRec> tab(k);
            fastx_twin::fastx_twin_windowed_table(tab.data());
            std::vector<std::vector<uint8_t>> seqs(k);
            for (uint64_t j = 0; j < k; ++j) { seqs[j].resize(tab[j].seq_len + 1); fastx_twin::fastx_twin_windowed_seq(j, seqs[j].data()); }
            if (fastx_twin::fastx_twin_selected(text.data(), n, 64, 3001, 4096, sel.data(), sel.size()) || fastx_twin::fastx_twin_windowed_count() != k) { fail("the selected pass differs", chunk, spacing); continue; }
            std::vector<FxRec> want(k);
            fastx_twin::fastx_twin_windowed_table(want.data());
            for (uint64_t j = 0; j < k; ++j) {
                std::vector<uint8_t> out(want[j].seq_len + 1);
                fastx_twin::fastx_twin_windowed_seq(j, out.data());
                if (want[j].name_off != tab[j].name_off || want[j].seq_len != tab[j].seq_len || memcmp(out.data(), seqs[j].data(), want[j].seq_len)) { fail("a record of the mapped pass differs", chunk, spacing); break; }
            }
        }
    return bad;
}

// The seek map of a bzip2 file: returns the disagreements
static uint64_t bzip2_seek(const char *path, const std::vector<uint8_t> &d) {
    uint64_t bad = 0;
    const auto fail = [&](const char *what, uint64_t round, uint64_t spacing) { ++bad; fprintf(stderr, "%s: bzip2 seek, round %llu spacing %llu: %s\n", path, (unsigned long long)round, (unsigned long long)spacing, what); };
    for (uint64_t round : {(uint64_t)1, (uint64_t)0})
        for (uint64_t sp = 0; sp < 3; ++sp) {
            uint64_t cs[4];
            uint64_t spacing = sp == 0 ? 1 : 4096;
            int rc = fastx_twin::fastx_twin_bz_census_map(d.data(), d.size(), round, spacing, 64, 3001, 4096, 512, cs);
            if (sp == 2) { spacing = fastx_twin::fastx_twin_gz_text(nullptr) + 1; rc = fastx_twin::fastx_twin_bz_census_map(d.data(), d.size(), round, spacing, 64, 3001, 4096, 512, cs); }
            std::vector<uint8_t> text((size_t)fastx_twin::fastx_twin_gz_text(nullptr) + 1);
            const uint64_t n = fastx_twin::fastx_twin_gz_text(text.data());
            const uint64_t nb = fastx_twin::fastx_twin_bz_blocks(nullptr, 0), ne = fastx_twin::fastx_twin_bz_entries(nullptr, 0);
            std::vector<uint64_t> blk(8 * nb + 8), ent(6 * ne + 6);
            fastx_twin::fastx_twin_bz_blocks(blk.data(), nb);
            fastx_twin::fastx_twin_bz_entries(ent.data(), ne);
            if (!nb || !ne || blk[0] != 32 || blk[2] || ent[0] || ent[6 * (ne - 1) + 1] != nb) { fail("block 0 is not the start of the file, or the entries do not hold the blocks", round, spacing); continue; }
            for (uint64_t i = 0; i < nb; ++i) {
                const uint64_t off = blk[8 * i + 2], len = blk[8 * i + 3];
                if (off + len > n || (i + 1 < nb && (blk[8 * i + 10] != off + len || blk[8 * i + 8] != blk[8 * i + 1])) || (i + 1 == nb && off + len != n)) { fail("the blocks do not tile the text", round, spacing); break; }
                std::vector<uint8_t> out((size_t)len + 1);
                uint64_t got = 0, sum = 0;
                bool good = true;
                for (uint32_t j = 0; j < FX_BZ_MARKS && good; ++j) {       // every lane alone: the segments tile the block's text
                    good = !fastx_twin::fastx_twin_bz_segment(d.data(), d.size(), i, j, j & 3, out.data(), &got) && !memcmp(out.data(), text.data() + off + sum, (size_t)got);
                    sum += got;
                }
                for (uint32_t skew = 0; skew < 4 && good; ++skew)
                    good = !fastx_twin::fastx_twin_bz_segment(d.data(), d.size(), i, FX_BZ_MARKS, skew, out.data(), &got) && got == len && !memcmp(out.data(), text.data() + off, (size_t)len);
                if (!good || sum != len) { fail("a block entered at its marks is not its text", round, spacing); break; }
            }
            if (rc) continue;                      // (a text that is no FASTA / FASTQ: blocks and marks are the bzip2 side's alone)
            std::vector<uint32_t> sel;
            for (uint64_t i = 0; i < cs[0]; i += 3) sel.push_back((uint32_t)i);
            if (cs[0] && sel.back() != cs[0] - 1) sel.push_back((uint32_t)(cs[0] - 1));
            uint64_t ps[4], ms[4];
            uint32_t status = 0;
            if (fastx_twin::fastx_twin_seek_plan(nullptr, nullptr, 0, 0, sel.data(), sel.size(), ps) || ps[1] > n || ps[2] > d.size() || ps[3] > ne) fail("the plan", round, spacing);
            if (fastx_twin::fastx_twin_bz_mapped(d.data(), d.size(), 64, 3001, 4096, sel.data(), sel.size(), &status)) { fail("the mapped pass is not proven", round, spacing); continue; }
            fastx_twin::fastx_twin_plan_stats(ms);
            if (memcmp(ps, ms, sizeof ps)) fail("the mapped pass brought something else than the plan", round, spacing);
            const uint64_t k = fastx_twin::fastx_twin_windowed_count();
            std::vector<FxRec> tab(k);
            fastx_twin::fastx_twin_windowed_table(tab.data());
            std::vector<std::vector<uint8_t>> seqs(k);
            for (uint64_t j = 0; j < k; ++j) { seqs[j].resize(tab[j].seq_len + 1); fastx_twin::fastx_twin_windowed_seq(j, seqs[j].data()); }
            if (fastx_twin::fastx_twin_selected(text.data(), n, 64, 3001, 4096, sel.data(), sel.size()) || fastx_twin::fastx_twin_windowed_count() != k) { fail("the selected pass differs", round, spacing); continue; }
            std::vector<FxRec> want(k);
            fastx_twin::fastx_twin_windowed_table(want.data());
            for (uint64_t j = 0; j < k; ++j) {
                std::vector<uint8_t> out(want[j].seq_len + 1);
                fastx_twin::fastx_twin_windowed_seq(j, out.data());
                if (want[j].name_off != tab[j].name_off || want[j].seq_len != tab[j].seq_len || memcmp(out.data(), seqs[j].data(), want[j].seq_len)) { fail("a record of the mapped pass differs", round, spacing); break; }
            }
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
        if (path.size() > 3 && path.compare(path.size() - 3, 3, ".gz") == 0) { bad += gzip_seek(argv[a], t); ++runs; continue; }
        if (ends(".bz2")) { bad += bzip2_seek(argv[a], t); ++runs; continue; }
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
                    if (!is_bam && !is_sam) bad += fastx_seek(argv[a], t, S, window, piece, rc, tab);
                    if (is_bam) bad += bam_sampled(argv[a], t, S, window, piece, rc, tab);
                    if (is_sam) bad += sam_sampled(argv[a], t, window, piece, rc, tab);
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
