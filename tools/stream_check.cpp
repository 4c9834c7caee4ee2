// stream_check.cpp -- a stand-alone driver of the byte source (csrc/fx_input.h) and the incremental BGZF walk (csrc/bgzf_scan.h
// BgzfWalk) of the streamed first pass, to be built with the sanitizers and run as a program of its own:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lrge_amd/csrc tools/stream_check.cpp -o stream_check
//   ./stream_check file1 file2 ...
// Every file is read whole through one FxInput::read and then again by range at several piece sizes (a descriptor and a buffer):
// the pieces must give the whole file's bytes, head, tail and last word, and reads that reach past the end must fail.  The walk
// fed with those pieces must give the table of bgzf_scan_blocks on the whole buffer -- or refuse where it refuses, at one
// file offset whatever the piece.  Prints "stream_check: ok" and exits 0, or says what differs and exits 1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "bgzf_scan.h"
#include "fx_input.h"

static int fail(const char *path, const char *what, unsigned long long a = 0, unsigned long long b = 0) {
    fprintf(stderr, "stream_check: %s: %s (%llu, %llu)\n", path, what, a, b);
    return 1;
}

static bool same(const BgzfBlock &a, const BgzfBlock &b) {
    return a.c_off == b.c_off && a.o_off == b.o_off && a.d_off == b.d_off && a.d_len == b.d_len && a.c_len == b.c_len && a.isize == b.isize && a.crc == b.crc;
}

static int check(const char *path) {
    FxInput in;
    if (!in.open_path(path)) return fail(path, "cannot be opened");
    std::vector<uint8_t> whole((size_t)in.len + 1);
    if (!in.read(0, in.len, whole.data())) return fail(path, "whole read failed");
    if (in.n_bytes != in.len) return fail(path, "bytes counted", in.n_bytes, in.len);
    uint8_t past[2];
    if (in.read(in.len, 1, past) || in.read(in.len + 1, 0, past) || (in.len && in.read(in.len - 1, 2, past))) return fail(path, "a read past the end did not fail");
    // head, tail and the last word
    uint8_t h[6], t[12];
    uint64_t nh = 0, nt = 0;
    uint32_t isize = 0;
    if (!in.head(h, sizeof h, &nh) || !in.tail(t, sizeof t, &nt) || !in.gzip_isize(&isize)) return fail(path, "head / tail read failed");
    if (nh != (in.len < 6 ? in.len : 6) || memcmp(h, whole.data(), (size_t)nh)) return fail(path, "head differs");
    if (nt != (in.len < 12 ? in.len : 12) || memcmp(t, whole.data() + in.len - nt, (size_t)nt)) return fail(path, "tail differs");
    if (in.len >= 18 && isize != bgzf_u32(whole.data() + in.len - 4)) return fail(path, "last word differs");
    // the table of the whole buffer
    std::vector<BgzfBlock> ref;
    uint64_t ref_len = 0;
    const bool ref_ok = bgzf_scan_blocks(whole.data(), in.len, &ref, &ref_len);
    FxInput mem;                                 // the same bytes as a buffer
    mem.d = whole.data(); mem.len = in.len;
    uint64_t bad_first = 0;
    bool have_bad = false;
    const uint64_t sizes[] = {1, 2, 7, 17, 18, 19, 26, 29, 64, 509, 4096, 65535, 65536, 65537, in.len ? in.len : 1, in.len + 5};
    for (const FxInput *src : {(const FxInput *)&in, (const FxInput *)&mem})
        for (uint64_t piece : sizes) {
            std::vector<uint8_t> buf((size_t)piece);
            std::vector<uint8_t> got;
            std::vector<BgzfBlock> tab;
            BgzfWalk w;
            bool ok = true;
            for (uint64_t at = 0; at < src->len; at += piece) {
                const uint64_t m = piece < src->len - at ? piece : src->len - at;
                if (!src->read(at, m, buf.data())) return fail(path, "a piece could not be read", at, m);
                got.insert(got.end(), buf.begin(), buf.begin() + (std::ptrdiff_t)m);
                if (ok) ok = w.feed(buf.data(), m, &tab);
            }
            if (got.size() != src->len || (!got.empty() && memcmp(got.data(), whole.data(), got.size()))) return fail(path, "the pieces differ from the whole file", piece);
            if (ok) ok = w.end();
            if (ok != ref_ok) return fail(path, "the walks disagree on the file", piece, ok);
            if (ok) {
                if (tab.size() != ref.size() || w.o != ref_len) return fail(path, "another table size", piece, tab.size());
                for (size_t i = 0; i < tab.size(); ++i) if (!same(tab[i], ref[i])) return fail(path, "another block record", piece, i);
            } else {
                if (have_bad && w.bad_off != bad_first) return fail(path, "another refusal offset", piece, w.bad_off);
                bad_first = w.bad_off; have_bad = true;
                if (w.feed(buf.data(), 0, &tab) || w.end()) return fail(path, "a refused walk went on", piece);
            }
        }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: stream_check FILE...\n"); return 2; }
    FxInput none;
    if (none.open_path("/nonexistent/stream_check") || none.open_path(".")) { fprintf(stderr, "stream_check: a missing path or a directory opened\n"); return 1; }
    for (int i = 1; i < argc; ++i) if (check(argv[i])) return 1;
    printf("stream_check: ok (%d files)\n", argc - 1);
    return 0;
}
