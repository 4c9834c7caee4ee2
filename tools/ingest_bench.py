"""FASTQ file -> read set consumable on the device: the device ingest (lrge_hip_reads_open + lrge_hip_seqset_from_reads) against
the route without it (lrge_hip_read_records_gpu_ex into per-record strings, concatenation into the upload arrays,
lrge_hip_seqset_upload), on one synthetic FASTQ (the seeded parts of tools/gzip_bench.py) raw, in BGZF and as plain gzip, and on
the same reads as a BGZF unaligned BAM (written here from the SAM/BAM specification) at several BAM_SEGMENT_BYTES and as plain
unaligned SAM text (the "sam" kind: its record scan beside the FASTQ kind's, and the host reader's time on the same file).  Only
the files of the kinds asked for are written.  Usage:
  python tools/ingest_bench.py [--gbases 1.08] [--dir /tmp] [--reps 5] [--kinds fq,bgzf.fq.gz,fq.gz,bam,sam]
                               [--bam-segments 262144,1048576,4194304] [--out profiles/ingest_bench.json]
                               [--windowed [--window-mb 64[,1024]]] [--sampled K [--window-mb 64]] [--sampled K1,K2,.. --seek]
                               [--kinds fq.zst --zstd-windowed K [--window-mb 64] [--out profiles/ingest_zstd_windowed_bench.json]]
--zstd-windowed K (kind fq.zst: the FASTQ text compressed by libzstd at level 3 with content checksums, once as one frame and once
as 64 frames): in every repeat the resident open (LRGE_GPU_INFLATE_ZSTD), the windowed open (| LRGE_GPU_INGEST_WINDOWED |
LRGE_GPU_INGEST_WINDOWED_ZSTD), the census, the selected open of K seeded ordinals and the host way (libzstd on
one thread, then the open of the plain text) run one after the other, so all five alternate in one process; under the key
"zstd_windowed" of --out.  With LRGE_HIP_LIB_AB naming a build from before the flag only the resident open is timed, under the
key "zstd_windowed_parent".
--stream [--sampled K --seek] (kinds fq, bgzf.fq.gz, fq.gz, bam; DESIGN section 30, BASELINE section 20): in every repeat the single windowed
open, the census and the selected open of K seeded ordinals from a path, each without and with LRGE_GPU_INGEST_STREAM, and with --seek
the two-pass totals (census with a map, then the mapped open), all alternating in one process; the calls without the flag are
unchanged code and stand for the parent commit.  lrge_hip_last_stream_stats of every streamed call is kept, and the peak resident
set of one open per route is taken in a fresh child process each (VmHWM of /proc/self/status before and behind the open: ru_maxrss is
inherited from the parent across exec).  One warm-up and --reps timed repeats, every repeat
written; the default --out becomes profiles/ingest_stream_bench.json.
--sampled K1,K2,.. --seek: on the plain and the BGZF FASTQ file and on the uBAM (kind bam: LRGE_GPU_INGEST_SELECT_ALN), for every K, the census without and with a seek map
(--kinds fq.gz --sampled K1,K2 --seek [--gzip-chunk-kb N]: the same on the plain gzip FASTQ, entered at the entries of its map; the selected open
beside it is the route the parent commit took for the mapped open, "blocks_decoded" counts entries, and with --gzip-chunk-kb the result goes under "<K>@chunk<N>k")
(--kinds sam,sam.gz,cram --sampled K1,K2 --seek: the same on unaligned SAM text, plain and bgzipped, under LRGE_GPU_INGEST_SELECT_SAM, and on an
unaligned CRAM of --cram-slices slices under LRGE_GPU_INGEST_SELECT_CRAM; the single open beside them is the parent
commit's route for the same command -- the full windowed SAM open, the full CRAM open.  The kinds sam.gz and cram are written only when named)
(--kinds fq.bz2 --sampled K1,K2 --seek: the same on the FASTQ as one bzip2 stream of level 9, entered at whole blocks and a block at its 64 marks; the
selected open beside it is the route the parent commit took for the mapped open, "blocks_decoded" counts entries, and one run more under BZIP2_TIMING gives the stage times
of the census that records marks and of the mapped open under "bzip2_stages")
(lrge_hip_reads_census, lrge_hip_reads_census_map), the selected open and the mapped open of the same K seeded ordinals
(lrge_hip_reads_open_selected, lrge_hip_reads_open_mapped) and the existing windowed open, all alternating in one run; with the
bytes the mapped open brought and read, under the key "sampled_seek" / "<K>" of --out.
--sampled K: on each FASTQ file the two passes of the sampled ingest (lrge_hip_reads_census, then lrge_hip_reads_open_selected of K
seeded ordinals and a read set of those K) beside the existing windowed open of the same file (and its read set of ALL reads),
alternating in the same run; the result goes under the key "sampled" of --out.  With LRGE_HIP_LIB_AB naming a build from before
the sampled ingest only the existing open is timed, under the key "sampled_parent": the number to put beside the two passes.
--windowed: on each file the windowed device route (LRGE_GPU_INGEST_WINDOWED | LRGE_GPU_INGEST_WINDOWED_ALN with option
INGEST_WINDOW_BYTES = --window-mb, one run per size of the list on the same files) beside the resident device route, alternating in the same run; the result of the FASTQ kinds
goes under the key "windowed" of --out, that of the kinds bam and sam under "windowed_aln" / "<window-mb>"; the other entries are
kept.  (To compare with another build of the library, run the same command there: the resident route is timed in every run.)

Both routes are driven by a small C++ helper (compiled here with g++ against liblrge_hip.so), so that no Python callback sits
in either clock.  Both start from the file's path with the file in the page cache and end when lrge_hip_seqset_wait has
returned for a set of ALL reads.  One warm-up run per route and file, then --reps timed runs; every run is reported."""
import argparse
import ctypes as C
import json
import multiprocessing as mp
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HELPER = r"""
#include <chrono>
#include <cstdint>
#include <string>
#include <vector>
#include "lrge_hip.h"
static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct Recs { std::vector<std::string> names, seqs; };
static void cb(void *u, const char *n, uint64_t nl, const char *b, uint64_t bl) { Recs *r = (Recs *)u; r->names.emplace_back(n, nl); r->seqs.emplace_back(b, bl); }
// ms: records, arrays, upload + wait
extern "C" int route_host(lrge_hip_ctx *ctx, const char *path, int flags, double ms[3], uint64_t *n_reads, uint64_t *n_bases) {
    Recs r;
    const double t0 = now();
    int used = 0;
    int rc = lrge_hip_read_records_gpu_ex(ctx, path, flags, cb, &r, &used);
    if (rc) return rc;
    const double t1 = now();
    std::vector<uint64_t> off(r.seqs.size() + 1, 0);
    for (size_t i = 0; i < r.seqs.size(); ++i) off[i + 1] = off[i] + r.seqs[i].size();
    std::string cat; cat.reserve(off.back());
    for (auto &s : r.seqs) cat += s;
    const double t2 = now();
    lrge_hip_seqset *s = nullptr;
    rc = lrge_hip_seqset_upload(ctx, cat.data(), off.data(), (uint32_t)r.seqs.size(), nullptr, &s);
    if (!rc) rc = lrge_hip_seqset_wait(s);
    const double t3 = now();
    lrge_hip_seqset_free(s);
    ms[0] = t1 - t0; ms[1] = t2 - t1; ms[2] = t3 - t2;
    *n_reads = r.seqs.size(); *n_bases = off.back();
    return rc;
}
// ms: open (stages[0..2]: text to HBM, record scan, identifiers and lengths), seqset of all reads + wait
extern "C" int route_device(lrge_hip_ctx *ctx, const char *path, int flags, double ms[2], float stages[4], uint64_t *n_reads, uint64_t *n_bases, uint64_t *text_bytes,
                            lrge_hip_bam_stats *bam, uint64_t win[4]) {
    const double t0 = now();
    lrge_hip_reads *r = nullptr;
    int rc = lrge_hip_reads_open(ctx, path, flags, &r);
    if (rc) return rc;
    const double t1 = now();
    const uint64_t n = lrge_hip_reads_count(r);
    std::vector<uint32_t> idx(n), len(n);
    for (uint64_t i = 0; i < n; ++i) idx[i] = (uint32_t)i;
    lrge_hip_seqset *s = nullptr;
    rc = lrge_hip_seqset_from_reads(ctx, r, idx.data(), (uint32_t)n, nullptr, &s);
    if (!rc) rc = lrge_hip_seqset_wait(s);
    const double t2 = now();
    lrge_hip_reads_table(r, len.data(), nullptr, nullptr);
    uint64_t b = 0; for (uint32_t l : len) b += l;
    lrge_hip_reads_timings(r, stages);
    if (lrge_hip_reads_bam_stats(r, bam)) *bam = lrge_hip_bam_stats{0, 0, 0, 0, 0, 0};
    lrge_hip_reads_window_stats(r, win);
    *n_reads = n; *n_bases = b; *text_bytes = lrge_hip_reads_text_bytes(r);
    lrge_hip_seqset_free(s); lrge_hip_reads_free(r);
    ms[0] = t1 - t0; ms[1] = t2 - t1;
    return rc;
}
"""

# ms: census, selected open (stages: its timings), read set of the k kept reads + wait
HELPER_SAMPLED = r"""
#include <chrono>
#include <cstdint>
#include <vector>
#include "lrge_hip.h"
static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
extern "C" int route_sampled(lrge_hip_ctx *ctx, const char *path, int flags, const uint32_t *sel, uint32_t k, double ms[3], float stages[4], uint64_t census[4],
                             uint64_t stats[4], uint64_t win[4]) {
    const double t0 = now();
    int rc = lrge_hip_reads_census(ctx, path, flags, census);
    if (rc) return rc;
    const double t1 = now();
    lrge_hip_reads *r = nullptr;
    rc = lrge_hip_reads_open_selected(ctx, path, flags, sel, k, &r);
    if (rc) return rc;
    const double t2 = now();
    std::vector<uint32_t> idx(k);
    for (uint32_t i = 0; i < k; ++i) idx[i] = i;
    lrge_hip_seqset *s = nullptr;
    rc = lrge_hip_seqset_from_reads(ctx, r, idx.data(), k, nullptr, &s);
    if (!rc) rc = lrge_hip_seqset_wait(s);
    const double t3 = now();
    lrge_hip_reads_timings(r, stages);
    lrge_hip_reads_select_stats(r, stats);
    lrge_hip_reads_window_stats(r, win);
    lrge_hip_seqset_free(s); lrge_hip_reads_free(r);
    ms[0] = t1 - t0; ms[1] = t2 - t1; ms[2] = t3 - t2;
    return rc;
}
"""

# ms: census, census with a map, selected open, mapped open, read set of the k reads of the mapped handle + wait
HELPER_SEEK = r"""
#include <chrono>
#include <cstdint>
#include <vector>
#include "lrge_hip.h"
static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static uint64_t g_kept[2];      // identifier bytes on the host and bytes in the store of the last mapped handle
extern "C" void kept_bytes(uint64_t out[2]) { out[0] = g_kept[0]; out[1] = g_kept[1]; }
// identifier bytes on the host and bytes in the store of the single full open
extern "C" int full_bytes(lrge_hip_ctx *ctx, const char *path, int flags, uint64_t out[2]) {
    lrge_hip_reads *r = nullptr;
    const int rc = lrge_hip_reads_open(ctx, path, flags, &r);
    if (rc) return rc;
    uint64_t w[4] = {0, 0, 0, 0};
    lrge_hip_reads_window_stats(r, w);
    out[0] = lrge_hip_reads_name_bytes(r); out[1] = w[0] ? w[1] : lrge_hip_reads_text_bytes(r);      // (a resident text stays whole)
    lrge_hip_reads_free(r);
    return 0;
}
extern "C" int route_seek(lrge_hip_ctx *ctx, const char *path, int flags, const uint32_t *sel, uint32_t k, double ms[5], uint64_t census[4], uint64_t map_stats[4],
                          uint64_t sel_stats[4], uint64_t seek[4]) {
    uint64_t c2[4], s2[4];
    const double t0 = now();
    int rc = lrge_hip_reads_census(ctx, path, flags, census);
    if (rc) return rc;
    const double t1 = now();
    lrge_hip_read_map *m = nullptr;
    if ((rc = lrge_hip_reads_census_map(ctx, path, flags, c2, &m))) return rc;
    const double t2 = now();
    lrge_hip_reads *a = nullptr, *b = nullptr;
    if ((rc = lrge_hip_reads_open_selected(ctx, path, flags, sel, k, &a))) return rc;
    const double t3 = now();
    if ((rc = lrge_hip_reads_open_mapped(ctx, path, flags, m, sel, k, &b))) return rc;
    const double t4 = now();
    std::vector<uint32_t> idx(k);
    for (uint32_t i = 0; i < k; ++i) idx[i] = i;
    lrge_hip_seqset *s = nullptr;
    rc = lrge_hip_seqset_from_reads(ctx, b, idx.data(), k, nullptr, &s);
    if (!rc) rc = lrge_hip_seqset_wait(s);
    const double t5 = now();
    lrge_hip_read_map_stats(m, map_stats);
    g_kept[0] = lrge_hip_reads_name_bytes(b);
    { uint64_t w[4] = {0, 0, 0, 0}; lrge_hip_reads_window_stats(b, w); g_kept[1] = w[1]; }
    lrge_hip_reads_select_stats(a, s2);
    lrge_hip_reads_select_stats(b, sel_stats);
    lrge_hip_reads_seek_stats(b, seek);
    for (int i = 0; i < 4; ++i) if (c2[i] != census[i] || s2[i] != sel_stats[i]) rc = rc ? rc : -100;      // the two routes must agree
    lrge_hip_seqset_free(s); lrge_hip_reads_free(a); lrge_hip_reads_free(b); lrge_hip_read_map_free(m);
    ms[0] = t1 - t0; ms[1] = t2 - t1; ms[2] = t3 - t2; ms[3] = t4 - t3; ms[4] = t5 - t4;
    return rc;
}
"""


BAM_HEADER = b"BAM\x01" + struct.pack("<i", 22) + b"@HD\tVN:1.6\tSO:unknown\n" + struct.pack("<i", 0)
BAM_STATS = ["segments", "empty_segments", "speculative_starts", "rejected_starts", "repair_rounds", "rewalked_segments"]


def _ubam(fq):
    """the reads of a FASTQ part as unaligned BAM records (SAM/BAM specification 4.2): flag 4, no reference, qualities kept"""
    import numpy as np
    code = np.full(256, 15, np.uint8)
    code[np.frombuffer(b"=ACMGRSVTWYHKDBN", np.uint8)] = np.arange(16, dtype=np.uint8)
    lines = fq.split(b"\n")
    out = []
    for i in range(0, len(lines) - 1, 4):
        name, seq = lines[i][1:].split()[0] + b"\0", lines[i + 1]
        c = code[np.frombuffer(seq, np.uint8)]
        if c.size & 1:
            c = np.append(c, np.uint8(0))
        body = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 0, 4680, 0, 4, len(seq), -1, -1, 0) + name + ((c[0::2] << 4) | c[1::2]).tobytes() + \
            (np.frombuffer(lines[i + 3], np.uint8) - 33).tobytes()
        out.append(struct.pack("<i", len(body)) + body)
    return b"".join(out)


SAM_HEADER = b"@HD\tVN:1.6\tSO:unknown\n"


def _usam(fq):
    """the reads of a FASTQ part as unaligned SAM lines (SAM specification 1.4): flag 4, no reference, qualities kept"""
    lines = fq.split(b"\n")
    return b"".join(b"%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\n" % (lines[i][1:].split()[0], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4))


def _bgzf(data, block=65280, level=1):
    """`data` as BGZF members (SAM/BAM specification 4.1), without the end-of-file block"""
    out = []
    for i in range(0, len(data), block):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        comp = c.compress(data[i:i + block]) + c.flush()
        out.append(bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0]) + b"BC" + struct.pack("<HH", 2, len(comp) + 25) + comp +
                   struct.pack("<II", zlib.crc32(data[i:i + block]), len(data[i:i + block])))
    return b"".join(out)


KINDS = ("fq", "bgzf.fq.gz", "fq.gz", "bam", "sam")
EXTRA_KINDS = ("sam.gz", "cram", "fq.bz2")      # written only when --kinds names them: bgzipped SAM, an unaligned CRAM (cram_file), the FASTQ as one bzip2 stream of level 9
# the flags of the single open and of the sampled calls, by kind (fq, bgzf.fq.gz, bam: as before)
OPEN_FLAGS = {"cram": 3 | 512, "fq.bz2": 15 | 16 | 32 | 64}
SEEK_FLAGS = {"bam": 15 | 1024, "sam": 15 | 4096, "sam.gz": 15 | 4096, "cram": 3 | 512 | 8192, "fq.bz2": 15 | 16}


def cram_file(path, slices, slice_kb):
    """an unaligned CRAM 3.0 of `slices` slices of slice_kb of bases each (BA in rANS 4x8 order 1, what CRAM 3.0 writers use for
    bases), made as tools/cram_bench.py makes its files: one container of four distinct slices is encoded once by tests/cram_writer.py
    and repeated -- containers are independent, so the file is a legal CRAM whose reads repeat.  Returns the bases"""
    import numpy as np
    import cram_writer as CW
    rng = np.random.Generator(np.random.PCG64(7))
    read_len, per_slice = 8192, max(1, slice_kb * 1024 // 8192)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    reads = [(b"bench/%d" % i, bytes(rng.choice(acgt, read_len))) for i in range(4 * per_slice)]
    hdr = b"@HD\tVN:1.6\tSO:unsorted\n"
    head = 26 + len(CW.container(0, 0, 0, 0, 0, 0, [CW.block("raw", 0, 0, struct.pack("<i", len(hdr)) + hdr)], [0]))
    eof = CW.container(-1, 4542278, 0, 0, 0, 0, [CW.block("raw", 1, 0, b"\x01\x00\x01\x00\x01\x00")], [])
    one = CW.write_cram(reads, method="gzip", slices_per_container=4, records_per_slice=per_slice, with_quality=False, with_tags=False, method_for={"BA": "rans1"})
    k = max(1, slices // 4)
    with open(path, "wb") as fh:
        fh.write(one[:head] + one[head:len(one) - len(eof)] * k + eof)
    return len(reads) * read_len * k


def _part(args):
    """(kind -> (text bytes, file bytes)) of part idx, for the kinds asked for"""
    import bgzf_writer as W
    import gzip_bench as GB
    idx, kinds = args
    d = GB._fastq(idx)
    out = {}
    if "fq" in kinds:
        out["fq"] = (len(d), d)
    if "bgzf.fq.gz" in kinds:
        out["bgzf.fq.gz"] = (len(d), W.bgzf_compress(d, eof=False, level=1))
    if "fq.gz" in kinds:
        c = zlib.compressobj(1, zlib.DEFLATED, 31)
        out["fq.gz"] = (len(d), c.compress(d) + c.flush())                  # (the plain gzip file: one member per part)
    if "bam" in kinds:
        bam = (BAM_HEADER if idx == 0 else b"") + _ubam(d)
        out["bam"] = (len(bam), _bgzf(bam))
    if "sam" in kinds:
        sam = (SAM_HEADER if idx == 0 else b"") + _usam(d)
        out["sam"] = (len(sam), sam)
    if "sam.gz" in kinds:
        sam = (SAM_HEADER if idx == 0 else b"") + _usam(d)
        out["sam.gz"] = (len(sam), _bgzf(sam))
    return out


def write_files(d, parts, kinds):
    import bgzf_writer as W
    paths = {k: os.path.join(d, "ingest." + k) for k in kinds}
    size = {k: 0 for k in paths}
    files = {k: open(p, "wb") for k, p in paths.items()}
    bz = None
    if "fq.bz2" in kinds:                       # (one stream: the parts go through one compressor, in order, in this process)
        import bz2
        import gzip_bench as GB
        bz = bz2.BZ2Compressor(9)
        for i in range(parts):
            d = GB._fastq(i)
            files["fq.bz2"].write(bz.compress(d))
            size["fq.bz2"] += len(d)
        files["fq.bz2"].write(bz.flush())
    with mp.get_context("spawn").Pool(16) as pool:
        for part in pool.imap(_part, [(i, tuple(k for k in kinds if k != "fq.bz2")) for i in range(parts)] if len(kinds) > (bz is not None) else []):
            for k, (n, data) in part.items():
                files[k].write(data)
                size[k] += n
    for k, fh in files.items():
        if k in ("bgzf.fq.gz", "bam", "sam.gz"):
            fh.write(W.EOF_BLOCK)
        fh.close()
    return paths, size


def windowed_runs(a, ctx, H, kinds, paths, text_bytes, aln):
    """the resident and the windowed device route on every file, alternating; into the key "windowed" of a.out, or (aln: the kinds
    bam and sam) into "windowed_aln" / "<window-mb>" of it"""
    out = {"window_bytes": a.window_mb << 20, "reps": a.reps, "text_bytes": {k: text_bytes[k] for k in kinds}, "files": {}}
    ctx.set_option("INGEST_WINDOW_BYTES", str(a.window_mb << 20))
    for kind in kinds:
        p = paths[kind]
        with open(p, "rb") as fh:
            while fh.read(64 << 20):
                pass                                                  # page cache
        runs = {"resident": [], "windowed": []}
        seen = {}
        for rep in range(a.reps + 1):
            for route, flags in (("resident", 15), ("windowed", 15 | 32 | 64)):
                ms2, st, nr, nb, tb, bs, win = (C.c_double * 2)(), (C.c_float * 4)(), C.c_uint64(), C.c_uint64(), C.c_uint64(), (C.c_uint64 * 6)(), (C.c_uint64 * 4)()
                rc = H.route_device(ctx.h, p.encode(), flags, C.byref(ms2), C.byref(st), C.byref(nr), C.byref(nb), C.byref(tb), C.byref(bs), C.byref(win))
                assert rc == 0, (kind, route, rc, ctx._lib.lrge_hip_last_error(ctx.h))
                assert tb.value == text_bytes[kind] and seen.setdefault("reads", (nr.value, nb.value)) == (nr.value, nb.value)
                store = (nb.value + 1) // 2 if kind == "bam" else nb.value                # (bam: packed, a pad nibble per odd read)
                assert (win[0] >= 1 and store <= win[1] <= store + nr.value) if route == "windowed" else win[0] == 0, (kind, route, list(win))   # (a gzip round may deliver all of the text: one window)
                seen[route] = list(win)
                if rep:                                                # (run 0 is the warm-up)
                    runs[route].append(dict(open_ms=ms2[0], seqset_ms=ms2[1], total_ms=sum(ms2), text_ms=st[0], scan_ms=st[1], names_ms=st[2]))
        med = lambda r, k: statistics.median(x[k] for x in runs[r])   # noqa: E731
        rng = lambda r, k: (min(x[k] for x in runs[r]), max(x[k] for x in runs[r]))   # noqa: E731
        f = dict(file_bytes=os.path.getsize(p), reads=seen["reads"][0], text_bytes=text_bytes[kind], store_bytes=seen["windowed"][1], windows=seen["windowed"][0],
                 largest_window_bytes=seen["windowed"][2], carried_bytes=seen["windowed"][3], resident_route=runs["resident"], windowed_route=runs["windowed"])
        for r in ("resident", "windowed"):
            for k in ("open_ms", "text_ms", "scan_ms", "seqset_ms", "total_ms"):
                f["%s_%s_median" % (r, k)] = med(r, k)
                f["%s_%s_range" % (r, k)] = rng(r, k)
        out["files"][kind] = f
        print(kind, json.dumps({k: v for k, v in f.items() if not k.endswith("_route")}), flush=True)
    ctx.set_option("INGEST_WINDOW_BYTES", None)
    result = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if aln:
        result.setdefault("windowed_aln", {})[str(a.window_mb)] = out
    else:
        result["windowed"] = out
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)


def sampled_runs(a, ctx, H, HS, kinds, paths, text_bytes):
    """the existing windowed open and -- HS: the library has them -- the two passes of the sampled ingest on every file, alternating;
    into the key "sampled" (HS None: "sampled_parent") of a.out"""
    import numpy as np
    out = {"window_bytes": a.window_mb << 20, "reps": a.reps, "k": a.sampled, "files": {}}
    ctx.set_option("INGEST_WINDOW_BYTES", str(a.window_mb << 20))
    for kind in kinds:
        p = paths[kind]
        with open(p, "rb") as fh:
            while fh.read(64 << 20):
                pass                                                  # page cache
        runs = {"open": [], "sampled": []}
        sel, seen = None, {}
        for rep in range(a.reps + 1):
            ms2, st, nr, nb, tb, bs, win = (C.c_double * 2)(), (C.c_float * 4)(), C.c_uint64(), C.c_uint64(), C.c_uint64(), (C.c_uint64 * 6)(), (C.c_uint64 * 4)()
            rc = H.route_device(ctx.h, p.encode(), 15 | 32 | 64, C.byref(ms2), C.byref(st), C.byref(nr), C.byref(nb), C.byref(tb), C.byref(bs), C.byref(win))
            assert rc == 0, (kind, rc, ctx._lib.lrge_hip_last_error(ctx.h))
            seen["reads"], seen["bases"], seen["windows"] = nr.value, nb.value, win[0]
            if rep:                                                    # (run 0 is the warm-up)
                runs["open"].append(dict(open_ms=ms2[0], seqset_all_ms=ms2[1], text_ms=st[0], scan_ms=st[1], names_ms=st[2]))
            if HS is None:
                continue
            if sel is None:
                sel = np.sort(np.random.default_rng(1).choice(nr.value, min(a.sampled, nr.value), replace=False)).astype(np.uint32)
            ms3, st, cen, sst, win = (C.c_double * 3)(), (C.c_float * 4)(), (C.c_uint64 * 4)(), (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
            rc = HS.route_sampled(ctx.h, p.encode(), 15, sel.ctypes.data, sel.size, C.byref(ms3), C.byref(st), C.byref(cen), C.byref(sst), C.byref(win))
            assert rc == 0, (kind, rc, ctx._lib.lrge_hip_last_error(ctx.h))
            assert (cen[0], cen[1], cen[2]) == (nr.value, nb.value, text_bytes[kind]) and (sst[0], sst[1], sst[2]) == (nr.value, sel.size, nb.value), (list(cen), list(sst))
            seen["kept_bases"], seen["sampled_windows"] = sst[3], win[0]
            if rep:
                runs["sampled"].append(dict(census_ms=ms3[0], selected_open_ms=ms3[1], both_ms=ms3[0] + ms3[1], seqset_k_ms=ms3[2], text_ms=st[0], scan_ms=st[1], names_ms=st[2]))
        f = dict(file_bytes=os.path.getsize(p), text_bytes=text_bytes[kind], **seen)
        for route, rr in runs.items():
            for key in (rr[0] if rr else {}):
                f["%s_%s_median" % (route, key)] = statistics.median(x[key] for x in rr)
                f["%s_%s_range" % (route, key)] = (min(x[key] for x in rr), max(x[key] for x in rr))
        out["files"][kind] = f
        print(kind, json.dumps(f), flush=True)
    ctx.set_option("INGEST_WINDOW_BYTES", None)
    result = json.load(open(a.out)) if os.path.exists(a.out) else {}
    result["sampled" if HS is not None else "sampled_parent"] = out
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)


def zstd_files(d, parts):
    """the FASTQ text of the other kinds as ingest.fq.zst (one frame) and ingest.fq64.zst (64 frames): libzstd level 3, content checksums"""
    import gzip_bench as GB
    import zstd_corpus as Z
    with mp.get_context("spawn").Pool(16) as pool:
        text = b"".join(pool.map(GB._fastq, range(parts)))
    paths = {"fq.zst": os.path.join(d, "ingest.fq.zst"), "fq64.zst": os.path.join(d, "ingest.fq64.zst")}
    open(paths["fq.zst"], "wb").write(Z.compress(text, 3))
    cut = -(-len(text) // 64)
    with mp.get_context("spawn").Pool(16) as pool:
        open(paths["fq64.zst"], "wb").write(b"".join(pool.map(Z.compress, [text[i:i + cut] for i in range(0, len(text), cut)])))
    return paths, len(text)


def zstd_runs(a, ctx, H, HS, paths, n_text):
    """the five routes of --zstd-windowed on both files, alternating in every repeat (HS None: the library is from before the flag,
    only the resident open); into the key "zstd_windowed" (HS None: "zstd_windowed_parent") of a.out"""
    import numpy as np
    from lrge_amd import readio
    ZSTD, SLIDE = 128, 32 | 2048
    out = {"window_bytes": a.window_mb << 20, "reps": a.reps, "k": a.zstd_windowed, "text_bytes": n_text, "files": {}}
    ctx.set_option("INGEST_WINDOW_BYTES", str(a.window_mb << 20))
    for kind, p in paths.items():
        raw = open(p, "rb").read()                                    # (page cache; the host way starts from these bytes' file too)
        runs, sel, seen = [], None, {}
        for rep in range(a.reps + 1):
            r = {}
            for route, flags in (("resident", 15 | ZSTD), ("windowed", 15 | ZSTD | SLIDE)):
                if route == "windowed" and HS is None:
                    continue
                ms2, st, nr, nb, tb, bs, win = (C.c_double * 2)(), (C.c_float * 4)(), C.c_uint64(), C.c_uint64(), C.c_uint64(), (C.c_uint64 * 6)(), (C.c_uint64 * 4)()
                rc = H.route_device(ctx.h, p.encode(), flags, C.byref(ms2), C.byref(st), C.byref(nr), C.byref(nb), C.byref(tb), C.byref(bs), C.byref(win))
                assert rc == 0, (kind, route, rc, ctx._lib.lrge_hip_last_error(ctx.h))
                assert tb.value == n_text and seen.setdefault("reads", (nr.value, nb.value)) == (nr.value, nb.value) and (win[0] > 1) == (route == "windowed"), (kind, route, list(win))
                r.update({route + "_open_ms": ms2[0], route + "_text_ms": st[0], route + "_scan_ms": st[1], route + "_seqset_ms": ms2[1]})
                if route == "windowed":
                    seen.update(windows=win[0], store_bytes=win[1], largest_window_bytes=win[2])
            if HS is not None:
                if sel is None:
                    sel = np.sort(np.random.default_rng(1).choice(seen["reads"][0], min(a.zstd_windowed, seen["reads"][0]), replace=False)).astype(np.uint32)
                ms3, st, cen, sst, win = (C.c_double * 3)(), (C.c_float * 4)(), (C.c_uint64 * 4)(), (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
                rc = HS.route_sampled(ctx.h, p.encode(), 15 | ZSTD | 2048, sel.ctypes.data, sel.size, C.byref(ms3), C.byref(st), C.byref(cen), C.byref(sst), C.byref(win))
                assert rc == 0, (kind, rc, ctx._lib.lrge_hip_last_error(ctx.h))
                assert (cen[0], cen[1], cen[2]) == (seen["reads"][0], seen["reads"][1], n_text) and (sst[0], sst[1]) == (seen["reads"][0], sel.size), (list(cen), list(sst))
                seen["kept_bases"] = sst[3]
                r.update(census_ms=ms3[0], selected_open_ms=ms3[1], two_pass_ms=ms3[0] + ms3[1], seqset_k_ms=ms3[2])
                t0 = time.perf_counter()
                text = readio.zstd_decompress(open(p, "rb").read())
                t1 = time.perf_counter()
                dr = ctx.open_reads(text, 3)
                t2 = time.perf_counter()
                assert dr.n == seen["reads"][0] and len(text) == n_text
                dr.free()
                del text
                r.update(libzstd_ms=(t1 - t0) * 1e3, host_way_ms=(t2 - t0) * 1e3)
            if rep:                                                    # (run 0 is the warm-up)
                runs.append(r)
        f = dict(file_bytes=len(raw), reads=seen["reads"][0], bases=seen["reads"][1], every_run=runs, **{k: v for k, v in seen.items() if k != "reads"})
        if HS is not None:
            dr = ctx.open_reads(raw, 15 | ZSTD | SLIDE)
            f["zstd_stats"] = dict(zip(("rounds", "largest_history", "largest_work_text", "history_bytes_moved"), dr.zstd_stats()))
            dr.free()
        for key in runs[0]:
            f["%s_median" % key] = statistics.median(x[key] for x in runs)
            f["%s_range" % key] = (min(x[key] for x in runs), max(x[key] for x in runs))
        out["files"][kind] = f
        print(kind, json.dumps({k: v for k, v in f.items() if k != "every_run"}), flush=True)
    ctx.set_option("INGEST_WINDOW_BYTES", None)
    result = json.load(open(a.out)) if os.path.exists(a.out) else {}
    result["zstd_windowed" if HS is not None else "zstd_windowed_parent"] = out
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)


def bzip2_stages(ctx, HK, p, flags, sel):
    """one route_seek under BZIP2_TIMING: the stage lines the library prints to stderr -- the census with a map (its walk and
    run-length write record marks), then the mapped open (entropy, scatter and k_bz_marks_text of the touched blocks only)"""
    import re
    ctx.set_option("BZIP2_TIMING", "1")
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            ms5, cen, mst, sst, sk = (C.c_double * 5)(), (C.c_uint64 * 4)(), (C.c_uint64 * 4)(), (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
            rc = HK.route_seek(ctx.h, p.encode(), flags, sel.ctypes.data, sel.size, C.byref(ms5), C.byref(cen), C.byref(mst), C.byref(sst), C.byref(sk))
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            ctx.set_option("BZIP2_TIMING", None)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    keys = ("find_ms", "entropy_ms", "scatter_ms", "walk_ms", "rle_crc_ms", "marks_text_ms")
    lines = [dict(zip(keys, (float(g) for g in m))) for m in re.findall(r"bzip2 stages ms: find ([\d.]+) entropy ([\d.]+) scatter ([\d.]+) walk ([\d.]+) rle_crc ([\d.]+) marks_text ([\d.]+)", text)]
    if rc != 0 or len(lines) != 2:
        return {"error": "rc %d, %d stage lines" % (rc, len(lines))}
    return {"census_map": lines[0], "mapped_open": lines[1], "timed_census_map_ms": ms5[1], "timed_mapped_open_ms": ms5[3]}


def seek_runs(a, ctx, H, HK, kinds, paths, text_bytes, ks):
    """for every K: the windowed open, the census without and with a map, the selected and the mapped open on every file, all
    alternating in every repeat; into the key "sampled_seek" / "<K>" of a.out"""
    import numpy as np
    ctx.set_option("INGEST_WINDOW_BYTES", str(a.window_mb << 20))
    if a.gzip_chunk_kb:                                                # (kind fq.gz, DESIGN section 28: a smaller chunk gives more entries)
        ctx.set_option("GZIP_CHUNK_BYTES", str(a.gzip_chunk_kb << 10))
    result = json.load(open(a.out)) if os.path.exists(a.out) else {}
    for K in ks:
        out = {"window_bytes": a.window_mb << 20, "reps": a.reps, "k": K, "gzip_chunk_bytes": a.gzip_chunk_kb << 10, "files": {}}
        for kind in kinds:
            p = paths[kind]
            with open(p, "rb") as fh:
                while fh.read(64 << 20):
                    pass                                              # page cache
            runs, sel, seen = [], None, {}
            for rep in range(a.reps + 1):
                ms2, st, nr, nb, tb, bs, win = (C.c_double * 2)(), (C.c_float * 4)(), C.c_uint64(), C.c_uint64(), C.c_uint64(), (C.c_uint64 * 6)(), (C.c_uint64 * 4)()
                rc = H.route_device(ctx.h, p.encode(), OPEN_FLAGS.get(kind, 15 | 32 | 64), C.byref(ms2), C.byref(st), C.byref(nr), C.byref(nb), C.byref(tb), C.byref(bs), C.byref(win))
                assert rc == 0, (kind, rc, ctx._lib.lrge_hip_last_error(ctx.h))
                if sel is None:
                    full = (C.c_uint64 * 2)()
                    assert HK.full_bytes(ctx.h, p.encode(), OPEN_FLAGS.get(kind, 15 | 32 | 64), C.byref(full)) == 0
                if sel is None:
                    sel = np.sort(np.random.default_rng(1).choice(nr.value, min(K, nr.value), replace=False)).astype(np.uint32)
                ms5, cen, mst, sst, sk = (C.c_double * 5)(), (C.c_uint64 * 4)(), (C.c_uint64 * 4)(), (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
                rc = HK.route_seek(ctx.h, p.encode(), SEEK_FLAGS.get(kind, 15), sel.ctypes.data, sel.size, C.byref(ms5), C.byref(cen), C.byref(mst), C.byref(sst), C.byref(sk))
                assert rc == 0, (kind, rc, ctx._lib.lrge_hip_last_error(ctx.h))
                assert (cen[0], cen[1], cen[2]) == (nr.value, nb.value, text_bytes[kind]) and (sst[0], sst[1], sst[2]) == (nr.value, sel.size, nb.value), (list(cen), list(sst))
                kb = (C.c_uint64 * 2)()
                HK.kept_bytes(C.byref(kb))
                seen = dict(reads=nr.value, bases=nb.value, kept_bases=sst[3], points=mst[1], stride=mst[2], runs=sk[0], text_bytes_brought=sk[1], file_bytes_read=sk[2], blocks_decoded=sk[3],
                            open_store_bytes=full[1], open_name_bytes=full[0], mapped_store_bytes=kb[1], mapped_name_bytes=kb[0])
                if rep:                                                # (run 0 is the warm-up)
                    runs.append(dict(open_ms=ms2[0], census_ms=ms5[0], census_map_ms=ms5[1], selected_open_ms=ms5[2], mapped_open_ms=ms5[3], seqset_k_ms=ms5[4],
                                     map_cost_ms=ms5[1] - ms5[0], two_pass_ms=ms5[1] + ms5[3], two_pass_parent_ms=ms5[0] + ms5[2]))
            f = dict(file_bytes=os.path.getsize(p), text_bytes=text_bytes[kind], every_run=runs, **seen)
            if kind == "fq.bz2":                                      # (the stages of the census that records marks and of the mapped open, one run more)
                f["bzip2_stages"] = bzip2_stages(ctx, HK, p, SEEK_FLAGS[kind], sel)
            for key in runs[0]:
                f["%s_median" % key] = statistics.median(x[key] for x in runs)
                f["%s_range" % key] = (min(x[key] for x in runs), max(x[key] for x in runs))
            out["files"][kind] = f
            print(K, kind, json.dumps({k: v for k, v in f.items() if k != "every_run"}), flush=True)
        key = str(K) + ("@chunk%dk" % a.gzip_chunk_kb if a.gzip_chunk_kb else "")
        prev = result.setdefault("sampled_seek", {}).get(key)
        if prev and (prev.get("window_bytes"), prev.get("reps")) == (out["window_bytes"], out["reps"]):      # (a second run with other kinds into the same --out adds its files)
            out["files"] = {**prev["files"], **out["files"]}
        result["sampled_seek"][key] = out
    ctx.set_option("INGEST_WINDOW_BYTES", None)
    ctx.set_option("GZIP_CHUNK_BYTES", None)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)


STREAM = 16384
STREAM_KINDS = ("fq", "bgzf.fq.gz", "fq.gz", "bam")


def _vm_kib(field):
    """a field of /proc/self/status in KiB (VmHWM: the peak resident set of this process image -- it starts anew at exec, where the
    ru_maxrss of getrusage is inherited from the parent's high-water mark and says nothing about a child of a large parent)"""
    for line in open("/proc/self/status"):
        if line.startswith(field + ":"):
            return int(line.split()[1])
    return -1


def _rss_child(path, flags):
    """one open of `path` in this (fresh) process: its code, the stream statistics, and the process's own peak resident set (VmHWM)
    with the context made, before the open, and behind the open -- the difference is what the open added"""
    from lrge_amd import engine
    ctx = engine.Context(0)
    h, st = C.c_void_p(), (C.c_uint64 * 4)()
    before = _vm_kib("VmHWM")
    rc = ctx._lib.lrge_hip_reads_open(ctx.h, path.encode(), flags, C.byref(h))
    after = _vm_kib("VmHWM")
    ctx._lib.lrge_hip_last_stream_stats(ctx.h, C.byref(st))
    ctx._lib.lrge_hip_reads_free(h)
    print(json.dumps(dict(rc=rc, stream_stats=[int(x) for x in st], vm_hwm_before_open_kib=before, vm_hwm_after_open_kib=after, open_added_kib=after - before)), flush=True)
    ctx.close()


def stream_runs(a, ctx, kinds, paths, text_bytes, k_sel, seek):
    """every path call without and with LRGE_GPU_INGEST_STREAM on every file, alternating; into a.out"""
    import numpy as np
    L = ctx._lib
    ctx.set_option("INGEST_WINDOW_BYTES", str(a.window_mb << 20))
    out = {"window_bytes": a.window_mb << 20, "stream_bytes": int(os.environ.get("LRGE_HIP_INGEST_STREAM_BYTES") or (64 << 20)), "reps": a.reps, "k": k_sel, "seek": bool(seek), "files": {}}
    for kind in kinds:
        p = paths[kind].encode()
        with open(paths[kind], "rb") as fh:
            while fh.read(64 << 20):
                pass                                                  # page cache
        open_fl, sel_fl = 15 | 32 | 64, 15 | (1024 if kind == "bam" else 0)
        runs = {"whole": [], "stream": []}
        stats, sel, seen = {}, None, {}

        def last():
            st = (C.c_uint64 * 4)()
            L.lrge_hip_last_stream_stats(ctx.h, C.byref(st))
            return [int(x) for x in st]

        def timed(call):
            t0 = time.perf_counter()
            rc = call()
            assert rc == 0, (kind, rc, L.lrge_hip_last_error(ctx.h))
            return (time.perf_counter() - t0) * 1e3

        for rep_i in range(a.reps + 1):
            for route, fl in (("whole", 0), ("stream", STREAM)):
                r, h, cen, m = {}, C.c_void_p(), (C.c_uint64 * 4)(), C.c_void_p()
                r["open_ms"] = timed(lambda: L.lrge_hip_reads_open(ctx.h, p, open_fl | fl, C.byref(h)))
                stats[route + "_open"] = last()
                assert L.lrge_hip_reads_text_bytes(h) == text_bytes[kind] and seen.setdefault("reads", int(L.lrge_hip_reads_count(h))) == L.lrge_hip_reads_count(h)
                L.lrge_hip_reads_free(h)
                r["census_ms"] = timed(lambda: L.lrge_hip_reads_census(ctx.h, p, sel_fl | fl, C.byref(cen)))
                stats[route + "_census"] = last()
                assert (cen[0], cen[2]) == (seen["reads"], text_bytes[kind]) and seen.setdefault("bases", int(cen[1])) == cen[1], list(cen)
                if sel is None:
                    sel = np.sort(np.random.default_rng(1).choice(seen["reads"], min(k_sel, seen["reads"]), replace=False)).astype(np.uint32)
                r["selected_open_ms"] = timed(lambda: L.lrge_hip_reads_open_selected(ctx.h, p, sel_fl | fl, sel.ctypes.data, sel.size, C.byref(h)))
                stats[route + "_selected"] = last()
                assert L.lrge_hip_reads_count(h) == sel.size
                L.lrge_hip_reads_free(h)
                r["two_pass_ms"] = r["census_ms"] + r["selected_open_ms"]
                if seek:
                    r["census_map_ms"] = timed(lambda: L.lrge_hip_reads_census_map(ctx.h, p, sel_fl | fl, C.byref(cen), C.byref(m)))
                    r["mapped_open_ms"] = timed(lambda: L.lrge_hip_reads_open_mapped(ctx.h, p, sel_fl | fl, m, sel.ctypes.data, sel.size, C.byref(h)))
                    assert L.lrge_hip_reads_count(h) == sel.size
                    L.lrge_hip_reads_free(h)
                    L.lrge_hip_read_map_free(m)
                    r["two_pass_seek_ms"] = r["census_map_ms"] + r["mapped_open_ms"]
                if rep_i:                                              # (run 0 is the warm-up)
                    runs[route].append(r)
        f = dict(file_bytes=os.path.getsize(paths[kind]), text_bytes=text_bytes[kind], stream_stats=stats, whole_route=runs["whole"], stream_route=runs["stream"], **seen)
        for route in ("whole", "stream"):
            for key in runs[route][0]:
                f["%s_%s_median" % (route, key)] = statistics.median(x[key] for x in runs[route])
                f["%s_%s_range" % (route, key)] = (min(x[key] for x in runs[route]), max(x[key] for x in runs[route]))
        for route, fl in (("whole", 0), ("stream", STREAM)):        # the peak resident set of one open, a fresh child process a route
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rss-child", paths[kind], str(open_fl | fl), "--window-mb", str(a.window_mb)], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            f[route + "_open_child"] = json.loads(r.stdout.strip().splitlines()[-1])
        out["files"][kind] = f
        print(kind, json.dumps({k: v for k, v in f.items() if not k.endswith("_route")}), flush=True)
    ctx.set_option("INGEST_WINDOW_BYTES", None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbases", type=float, default=1.08)
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--bam-segments", default="262144,1048576,4194304")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_bench.json"))
    ap.add_argument("--windowed", action="store_true")
    ap.add_argument("--window-mb", default="64")
    ap.add_argument("--sampled", default="0")
    ap.add_argument("--seek", action="store_true")
    ap.add_argument("--gzip-chunk-kb", type=int, default=0)
    ap.add_argument("--zstd-windowed", type=int, default=0)
    ap.add_argument("--cram-slices", type=int, default=512)
    ap.add_argument("--cram-slice-kb", type=int, default=256)
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--rss-child", nargs=2, metavar=("PATH", "FLAGS"))
    a = ap.parse_args()
    if a.rss_child:
        os.environ["LRGE_HIP_INGEST_WINDOW_BYTES"] = str(int(a.window_mb.split(",")[0]) << 20)
        return _rss_child(a.rss_child[0], int(a.rss_child[1]))
    seek_ks = [int(k) for k in a.sampled.split(",") if int(k)] if a.seek else []
    a.sampled = 0 if a.seek else int(a.sampled)
    if a.seek and not seek_ks:
        ap.error("--seek needs --sampled K[,K..]")
    from lrge_amd import build as B, engine
    work = tempfile.mkdtemp(dir=a.dir, prefix="ingest_bench_")
    src = os.path.join(work, "helper.cpp")
    open(src, "w").write(HELPER)
    so = os.path.join(work, "libhelper.so")
    lib_dir = os.path.dirname(os.environ.get("LRGE_HIP_LIB_AB") or "") or B.LIB_DIR          # (the helper calls the library the context comes from)
    build = lambda out, cpp: subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-o", out, cpp,   # noqa: E731
                                                    "-L" + lib_dir, "-llrge_hip", "-Wl,-rpath," + lib_dir])
    build(so, src)
    parts = max(1, round(a.gbases * 1e9 * 2.02 / (256 << 20)))       # a record is 2 bytes per base and a header
    t0 = time.perf_counter()
    if a.zstd_windowed:
        paths, n_text = zstd_files(work, parts)
        print("files written in %.0f s: %d text bytes" % (time.perf_counter() - t0, n_text), flush=True)
        ctx = engine.Context(0)
        H = C.CDLL(so)
        H.route_device.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_double * 2), C.POINTER(C.c_float * 4), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64 * 6), C.POINTER(C.c_uint64 * 4)]
        HS, extra = None, []
        if hasattr(ctx._lib, "lrge_hip_reads_zstd_stats"):
            extra = [os.path.join(work, "sampled.cpp"), os.path.join(work, "libsampled.so")]
            open(extra[0], "w").write(HELPER_SAMPLED)
            build(extra[1], extra[0])
            HS = C.CDLL(extra[1])
            HS.route_sampled.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_double * 3), C.POINTER(C.c_float * 4)] + [C.POINTER(C.c_uint64 * 4)] * 3
        a.window_mb = int(a.window_mb.split(",")[0])
        zstd_runs(a, ctx, H, HS, paths, n_text)
        ctx.close()
        for p in list(paths.values()) + [src, so] + extra:
            os.remove(p)
        os.rmdir(work)
        return
    kinds = [k for k in KINDS + EXTRA_KINDS if k in a.kinds.split(",") and (not a.stream or k in STREAM_KINDS)]
    paths, text_bytes = write_files(work, parts, [k for k in kinds if k != "cram"])
    if "cram" in kinds:
        paths["cram"] = os.path.join(work, "ingest.cram")
        text_bytes["cram"] = cram_file(paths["cram"], a.cram_slices, a.cram_slice_kb)      # (what lrge_hip_reads_text_bytes reports: the bases)
    print("files written in %.0f s: %s text bytes" % (time.perf_counter() - t0, text_bytes), flush=True)
    ctx = engine.Context(0)
    if a.stream:
        if a.out == os.path.join(ROOT, "profiles", "ingest_bench.json"):
            a.out = os.path.join(ROOT, "profiles", "ingest_stream_bench.json")
        a.window_mb = int(a.window_mb.split(",")[0])
        stream_runs(a, ctx, [k for k in kinds if k in STREAM_KINDS], paths, text_bytes, seek_ks[0] if seek_ks else (a.sampled or 1000), bool(seek_ks))
        ctx.close()
        for p in list(paths.values()) + [src, so]:
            os.remove(p)
        os.rmdir(work)
        return
    H = C.CDLL(so)
    H.route_host.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_double * 3), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    H.route_device.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_double * 2), C.POINTER(C.c_float * 4), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64 * 6), C.POINTER(C.c_uint64 * 4)]
    if seek_ks:
        extra = [os.path.join(work, "seek.cpp"), os.path.join(work, "libseek.so")]
        open(extra[0], "w").write(HELPER_SEEK)
        build(extra[1], extra[0])
        HK = C.CDLL(extra[1])
        HK.route_seek.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_double * 5)] + [C.POINTER(C.c_uint64 * 4)] * 4
        HK.full_bytes.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_uint64 * 2)]
        HK.kept_bytes.argtypes = [C.POINTER(C.c_uint64 * 2)]
        a.window_mb = int(a.window_mb.split(",")[0])
        seek_runs(a, ctx, H, HK, [k for k in kinds if k in ("fq", "bgzf.fq.gz", "fq.gz", "bam", "sam", "sam.gz", "cram", "fq.bz2")], paths, text_bytes, seek_ks)
        ctx.close()
        for p in list(paths.values()) + [src, so] + extra:
            os.remove(p)
        os.rmdir(work)
        return
    if a.sampled:
        HS, extra = None, []
        if hasattr(ctx._lib, "lrge_hip_reads_census"):
            extra = [os.path.join(work, "sampled.cpp"), os.path.join(work, "libsampled.so")]
            open(extra[0], "w").write(HELPER_SAMPLED)
            build(extra[1], extra[0])
            HS = C.CDLL(extra[1])
            HS.route_sampled.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_double * 3), C.POINTER(C.c_float * 4)] + [C.POINTER(C.c_uint64 * 4)] * 3
        a.window_mb = int(a.window_mb.split(",")[0])
        sampled_runs(a, ctx, H, HS, [k for k in kinds if k not in ("bam", "sam")], paths, text_bytes)
        ctx.close()
        for p in list(paths.values()) + [src, so] + extra:
            os.remove(p)
        os.rmdir(work)
        return
    if a.windowed:
        for mb in a.window_mb.split(","):
            a.window_mb = int(mb)
            for aln in (False, True):
                part = [k for k in kinds if (k in ("bam", "sam")) == aln]
                if part:
                    windowed_runs(a, ctx, H, part, paths, text_bytes, aln)
        kinds = []
    result = {"text_bytes": text_bytes, "reps": a.reps, "files": {}}
    # (a BAM run per segment size: the host route it is compared with does not depend on the option, and is timed beside each)
    work_list = [(k, k, None) for k in kinds if k != "bam"] + [("bam", "bam@%d" % int(S), int(S)) for S in a.bam_segments.split(",") if "bam" in kinds]
    for kind, label, seg in work_list:
        p = paths[kind]
        ctx.set_option("BAM_SEGMENT_BYTES", None if seg is None else str(seg))
        with open(p, "rb") as fh:
            while fh.read(64 << 20):
                pass                                                  # page cache
        runs_h, runs_d = [], []
        for rep in range(a.reps + 1):
            ms3, nr, nb = (C.c_double * 3)(), C.c_uint64(), C.c_uint64()
            rc = H.route_host(ctx.h, p.encode(), 3, C.byref(ms3), C.byref(nr), C.byref(nb))
            assert rc == 0, (kind, rc)
            ms2, st, nr2, nb2, tb, bs = (C.c_double * 2)(), (C.c_float * 4)(), C.c_uint64(), C.c_uint64(), C.c_uint64(), (C.c_uint64 * 6)()
            rc = H.route_device(ctx.h, p.encode(), 15, C.byref(ms2), C.byref(st), C.byref(nr2), C.byref(nb2), C.byref(tb), C.byref(bs), C.byref((C.c_uint64 * 4)()))
            assert rc == 0, (kind, rc, ctx._lib.lrge_hip_last_error(ctx.h))
            assert (nr.value, nb.value) == (nr2.value, nb2.value) and tb.value == text_bytes[kind]
            if rep:                                                    # (run 0 is the warm-up)
                runs_h.append(dict(records_ms=ms3[0], arrays_ms=ms3[1], upload_ms=ms3[2], total_ms=sum(ms3)))
                runs_d.append(dict(open_ms=ms2[0], seqset_ms=ms2[1], total_ms=sum(ms2), text_ms=st[0], scan_ms=st[1], names_ms=st[2]))
        med = lambda runs, k: statistics.median(r[k] for r in runs)   # noqa: E731
        rng = lambda runs, k: (min(r[k] for r in runs), max(r[k] for r in runs))   # noqa: E731
        f = dict(file_bytes=os.path.getsize(p), reads=nr.value, bases=nb.value, host_route=runs_h, device_route=runs_d,
                 host_total_ms_median=med(runs_h, "total_ms"), host_total_ms_range=rng(runs_h, "total_ms"),
                 host_records_ms_median=med(runs_h, "records_ms"), host_records_ms_range=rng(runs_h, "records_ms"),
                 device_total_ms_median=med(runs_d, "total_ms"), device_total_ms_range=rng(runs_d, "total_ms"),
                 scan_ms_median=med(runs_d, "scan_ms"), scan_ms_range=rng(runs_d, "scan_ms"), scan_text_gb_per_s=text_bytes[kind] / med(runs_d, "scan_ms") / 1e6)
        if seg is not None:
            f.update(bam_segment_bytes=seg, bam_stats=dict(zip(BAM_STATS, [int(x) for x in bs])))
        result["files"][label] = f
        print(label, json.dumps({k: v for k, v in f.items() if not k.endswith("_route")}), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if not a.windowed:
        for key in ("windowed", "windowed_aln"):
            if os.path.exists(a.out) and key in json.load(open(a.out)):
                result[key] = json.load(open(a.out))[key]
        json.dump(result, open(a.out, "w"), indent=1)
    for p in list(paths.values()) + [src, so]:
        os.remove(p)
    os.rmdir(work)


if __name__ == "__main__":
    main()
