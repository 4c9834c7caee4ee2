"""FASTQ file -> read set consumable on the device: the device ingest (lrge_hip_reads_open + lrge_hip_seqset_from_reads) against
the route without it (lrge_hip_read_records_gpu_ex into per-record strings, concatenation into the upload arrays,
lrge_hip_seqset_upload), on one synthetic FASTQ (the seeded parts of tools/gzip_bench.py) raw, in BGZF and as plain gzip.  Usage:
  python tools/ingest_bench.py [--gbases 1.08] [--dir /tmp] [--reps 5] [--out profiles/ingest_bench.json]

Both routes are driven by a small C++ helper (compiled here with g++ against liblrge_hip.so), so that no Python callback sits
in either clock.  Both start from the file's path with the file in the page cache and end when lrge_hip_seqset_wait has
returned for a set of ALL reads.  One warm-up run per route and file, then --reps timed runs; every run is reported."""
import argparse
import ctypes as C
import json
import multiprocessing as mp
import os
import statistics
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
extern "C" int route_device(lrge_hip_ctx *ctx, const char *path, int flags, double ms[2], float stages[4], uint64_t *n_reads, uint64_t *n_bases, uint64_t *text_bytes) {
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
    *n_reads = n; *n_bases = b; *text_bytes = lrge_hip_reads_text_bytes(r);
    lrge_hip_seqset_free(s); lrge_hip_reads_free(r);
    ms[0] = t1 - t0; ms[1] = t2 - t1;
    return rc;
}
"""


def _bgzf_part(idx):
    import bgzf_writer as W
    import gzip_bench as GB
    d = GB._fastq(idx)
    c = zlib.compressobj(1, zlib.DEFLATED, 31)
    return len(d), d, W.bgzf_compress(d, eof=False, level=1), c.compress(d) + c.flush()


def write_files(d, parts):
    import bgzf_writer as W
    paths = {k: os.path.join(d, "ingest." + k) for k in ("fq", "bgzf.fq.gz", "fq.gz")}
    size = 0
    with mp.get_context("spawn").Pool(16) as pool, open(paths["fq"], "wb") as fr, open(paths["bgzf.fq.gz"], "wb") as fb, open(paths["fq.gz"], "wb") as fg:
        for n, raw, bg, gz in pool.imap(_bgzf_part, range(parts)):
            fr.write(raw); fb.write(bg); fg.write(gz)        # (the plain gzip file: one member per part)
            size += n
        fb.write(W.EOF_BLOCK)
    return paths, size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbases", type=float, default=1.08)
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_bench.json"))
    a = ap.parse_args()
    from lrge_amd import build as B, engine
    work = tempfile.mkdtemp(dir=a.dir, prefix="ingest_bench_")
    src = os.path.join(work, "helper.cpp")
    open(src, "w").write(HELPER)
    so = os.path.join(work, "libhelper.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-o", so, src,
                           "-L" + B.LIB_DIR, "-llrge_hip", "-Wl,-rpath," + B.LIB_DIR])
    parts = max(1, round(a.gbases * 1e9 * 2.02 / (256 << 20)))       # a record is 2 bytes per base and a header
    t0 = time.perf_counter()
    paths, text_bytes = write_files(work, parts)
    print("files written in %.0f s: %d text bytes" % (time.perf_counter() - t0, text_bytes), flush=True)
    ctx = engine.Context(0)
    H = C.CDLL(so)
    H.route_host.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_double * 3), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    H.route_device.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_double * 2), C.POINTER(C.c_float * 4), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                               C.POINTER(C.c_uint64)]
    result = {"text_bytes": text_bytes, "reps": a.reps, "files": {}}
    for kind, p in paths.items():
        with open(p, "rb") as fh:
            while fh.read(64 << 20):
                pass                                                  # page cache
        runs_h, runs_d = [], []
        for rep in range(a.reps + 1):
            ms3, nr, nb = (C.c_double * 3)(), C.c_uint64(), C.c_uint64()
            rc = H.route_host(ctx.h, p.encode(), 3, C.byref(ms3), C.byref(nr), C.byref(nb))
            assert rc == 0, (kind, rc)
            ms2, st, nr2, nb2, tb = (C.c_double * 2)(), (C.c_float * 4)(), C.c_uint64(), C.c_uint64(), C.c_uint64()
            rc = H.route_device(ctx.h, p.encode(), 3, C.byref(ms2), C.byref(st), C.byref(nr2), C.byref(nb2), C.byref(tb))
            assert rc == 0, (kind, rc, ctx._lib.lrge_hip_last_error(ctx.h))
            assert (nr.value, nb.value) == (nr2.value, nb2.value) and tb.value == text_bytes
            if rep:                                                    # (run 0 is the warm-up)
                runs_h.append(dict(records_ms=ms3[0], arrays_ms=ms3[1], upload_ms=ms3[2], total_ms=sum(ms3)))
                runs_d.append(dict(open_ms=ms2[0], seqset_ms=ms2[1], total_ms=sum(ms2), text_ms=st[0], scan_ms=st[1], names_ms=st[2]))
        med = lambda runs, k: statistics.median(r[k] for r in runs)   # noqa: E731
        rng = lambda runs, k: (min(r[k] for r in runs), max(r[k] for r in runs))   # noqa: E731
        f = dict(file_bytes=os.path.getsize(p), reads=nr.value, bases=nb.value, host_route=runs_h, device_route=runs_d,
                 host_total_ms_median=med(runs_h, "total_ms"), host_total_ms_range=rng(runs_h, "total_ms"),
                 device_total_ms_median=med(runs_d, "total_ms"), device_total_ms_range=rng(runs_d, "total_ms"),
                 scan_ms_median=med(runs_d, "scan_ms"), scan_text_gb_per_s=text_bytes / med(runs_d, "scan_ms") / 1e6)
        result["files"][kind] = f
        print(kind, json.dumps({k: v for k, v in f.items() if not k.endswith("_route")}), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)
    for p in list(paths.values()) + [src, so]:
        os.remove(p)
    os.rmdir(work)


if __name__ == "__main__":
    main()
