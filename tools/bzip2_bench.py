"""bzip2 input: libbz2 on one thread (what include/lrge_io.hpp bunzip2_all runs) against the device path (lrge_hip_bzip2_inflate),
on a seeded FASTQ compressed as ONE level-9 stream.  Usage:
  python tools/bzip2_bench.py [--mb 512] [--repeats 5] [--out profiles/bzip2_bench.json]

Clock: from the compressed bytes in memory to the last decompressed byte delivered; both sides write the whole text into a
preallocated buffer.  One warm-up of each, then `repeats` rounds that alternate host and device on the same buffer in the same
process.  Reported: medians with ranges, the ratio of the medians, the call's stats, and the per-stage times of one more device run
with option BZIP2_TIMING (find, entropy decode, scatter, walk, run-length layer with CRC; that run drains the stream between the
stages, so its total is not the end-to-end time)."""
import argparse
import bz2
import ctypes as C
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fastq(n_bytes):
    import numpy as np
    rng = np.random.default_rng(2024)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    out, n, k = [], 0, 0
    while n < n_bytes:
        ln = int(rng.integers(500, 3000))
        seq = acgt[rng.integers(0, 4, ln)].tobytes()
        qual = (rng.integers(0, 3, ln, dtype=np.uint8) * 5 + 35).tobytes()
        rec = b"@r%d len=%d\n%s\n+\n%s\n" % (k, ln, seq, qual)
        out.append(rec); n += len(rec); k += 1
    return b"".join(out)


def host(data, size):
    """bunzip2_all's loop: one BZ2_bzDecompress stream, the output taken 1 MiB at a time"""
    out = bytearray(size)
    t0 = time.perf_counter()
    d = bz2.BZ2Decompressor()
    o = 0
    x = d.decompress(data, 1 << 20)
    while True:
        out[o:o + len(x)] = x
        o += len(x)
        if d.eof:
            break
        x = d.decompress(b"", 1 << 20)
    return time.perf_counter() - t0, o, out


def device(ctx, data, size):
    from lrge_amd import _ffi
    out = bytearray(size)
    base = C.addressof((C.c_char * max(1, size)).from_buffer(out))
    total = [0]

    def sink(_u, p, n):
        if total[0] + n > size:
            return 1
        C.memmove(base + total[0], p, n)
        total[0] += n
        return 0
    cb = _ffi.GZIP_SINK(sink)
    st = (C.c_uint64 * len(_ffi.BZIP2_STAT_NAMES))()
    t0 = time.perf_counter()
    rc = ctx._lib.lrge_hip_bzip2_inflate(ctx.h, data, len(data), cb, None, C.cast(st, C.c_void_p))
    t = time.perf_counter() - t0
    return rc, t, total[0], dict(zip(_ffi.BZIP2_STAT_NAMES, list(st))), out


def stage_times(ctx, data, size):
    """one device run with BZIP2_TIMING: the line the library prints to stderr"""
    ctx.set_option("BZIP2_TIMING", 1)
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            rc = device(ctx, data, size)[0]
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            ctx.set_option("BZIP2_TIMING", None)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    m = re.search(r"bzip2 stages ms: find ([\d.]+) entropy ([\d.]+) scatter ([\d.]+) walk ([\d.]+) rle_crc ([\d.]+)", text)
    if rc != 0 or not m:
        return {"error": "rc %d, no stage line" % rc}
    return dict(zip(("find_ms", "entropy_ms", "scatter_ms", "walk_ms", "rle_crc_ms"), (float(g) for g in m.groups())))


def spread(v):
    return {"median_s": round(statistics.median(v), 3), "min_s": round(min(v), 3), "max_s": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=512.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bzip2_bench.json"))
    a = ap.parse_args()
    from lrge_amd import engine
    t0 = time.perf_counter()
    text = fastq(int(a.mb * (1 << 20)))
    data = bz2.compress(text, 9)
    size = len(text)
    print("text %d bytes, bzip2 -9 %d bytes, made in %.1f s" % (size, len(data), time.perf_counter() - t0), flush=True)
    ctx = engine.Context(0)
    th, nh, oh = host(data, size)                                   # warm-up of each side, and the comparison of the bytes
    rc, td, nd, st, od = device(ctx, data, size)
    assert rc == 0 and nh == nd == size and oh == od == text, (rc, nh, nd, size)
    del oh, od, text
    print("warm-up: host %.3f s, device %.3f s, %s" % (th, td, st), flush=True)
    hs, ds = [], []
    for r in range(a.repeats):
        hs.append(host(data, size)[0])
        rc, td, nd, st, _ = device(ctx, data, size)
        assert rc == 0 and nd == size
        ds.append(td)
        print("repeat %d: host %.3f s, device %.3f s" % (r + 1, hs[-1], ds[-1]), flush=True)
    rec = {"uncompressed_bytes": size, "compressed_bytes": len(data), "level": 9, "repeats": a.repeats,
           "host_libbz2_1thread": spread(hs), "device_end_to_end": spread(ds),
           "device_speedup_vs_host": round(statistics.median(hs) / statistics.median(ds), 2),
           "device_out_GBps": round(size / statistics.median(ds) / 1e9, 3), "stats": st,
           "stages": stage_times(ctx, data, size)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
