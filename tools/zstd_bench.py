"""Zstandard input: the device path (lrge_hip_reads_open* | LRGE_GPU_INFLATE_ZSTD: decode to HBM and record scan) against libzstd
on one thread (readio.zstd_decompress) and against the way to the same resident read set without the flag (host decode, then
open_reads of the plain text), on a FASTQ of the counter-based generator's reads (lrge_amd/synth_cb.py) compressed at levels 3
and 19, as one frame and as 64 frames.  Usage:
  python tools/zstd_bench.py [--mb 48] [--repeats 3] [--out profiles/zstd_bench.json]

Clock: from the compressed bytes in memory to the read set open on the device (or, for libzstd alone, to the last decompressed
byte).  One warm-up of each, then `repeats` rounds that alternate the sides in the same process.  Reported per file: medians
with ranges, the device with ZSTD_CHECKSUM 1 and 0, the checksum's own milliseconds and its share of the decode (lrge_hip_zstd_stats:
checksum_us of a lrge_hip_zstd_inflate run), and the per-kernel times of one more such run with option ZSTD_TIMING (that run
drains the stream between the stages, so its total is not the end-to-end time)."""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def fastq(n_bytes):
    """reads 0, 1, 2, ... of the counter-based generator (ONT-like lengths and errors) with seeded qualities of twelve values"""
    import numpy as np
    from lrge_amd import synth_cb
    spec = synth_cb.Spec(20_000_000, 4242, "ont")
    rng = np.random.default_rng(2026)
    out, size, first = [], 0, 0
    while size < n_bytes:
        b = spec.host_reads(first=first, n=64)
        for i in range(64):
            seq = b.bases[int(b.offsets[i]):int(b.offsets[i + 1])].tobytes()
            qual = (rng.integers(0, 12, len(seq), dtype=np.uint8) * 3 + 40).tobytes()
            out.append(b"@%s\n%s\n+\n%s\n" % (b.names[i], seq, qual))
            size += len(out[-1])
        first += 64
    return out


def stage_times(ctx, data):
    ctx.set_option("ZSTD_TIMING", 1)
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            _, st = ctx.zstd_inflate(data)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            ctx.set_option("ZSTD_TIMING", None)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    m = re.search(r"zstd stages ms: heads ([\d.]+) literals ([\d.]+) sequences ([\d.]+) execute ([\d.]+) resolve ([\d.]+) checksum ([\d.]+)", text)
    if not m:
        return {"error": "no stage line"}, st
    return dict(zip(("heads_ms", "literals_ms", "sequences_ms", "execute_ms", "resolve_ms", "checksum_ms"), (float(g) for g in m.groups()))), st


def spread(v):
    return {"median_s": round(statistics.median(v), 4), "min_s": round(min(v), 4), "max_s": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=48.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--levels", default="3,19")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zstd_bench.json"))
    a = ap.parse_args()
    import zstd_corpus as Z
    from lrge_amd import _ffi, engine, readio
    t0 = time.perf_counter()
    recs = fastq(int(a.mb * (1 << 20)))
    text = b"".join(recs)
    print("text %d bytes in %d records, made in %.1f s" % (len(text), len(recs), time.perf_counter() - t0), flush=True)
    files = {}
    for level in (int(x) for x in a.levels.split(",")):
        t0 = time.perf_counter()
        files["l%d_one_frame" % level] = Z.compress(text, level)
        per = -(-len(recs) // 64)
        files["l%d_64_frames" % level] = b"".join(Z.compress(b"".join(recs[i:i + per]), level) for i in range(0, len(recs), per))
        print("level %d compressed in %.1f s: %d and %d bytes" % (level, time.perf_counter() - t0, len(files["l%d_one_frame" % level]), len(files["l%d_64_frames" % level])), flush=True)
    ctx = engine.Context(0)
    flags = _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP
    out = {"uncompressed_bytes": len(text), "records": len(recs), "repeats": a.repeats, "files": {}}

    def dev_open(data, checksum):
        ctx.set_option("ZSTD_CHECKSUM", checksum)
        t = time.perf_counter()
        dr = ctx.open_reads(data, flags | _ffi.GPU_INFLATE_ZSTD)
        t = time.perf_counter() - t
        n = dr.n
        dr.free()
        return t, n

    def host_open(data):
        t = time.perf_counter()
        plain = readio.zstd_decompress(data)
        t1 = time.perf_counter() - t
        dr = ctx.open_reads(plain, flags)
        t2 = time.perf_counter() - t
        n = dr.n
        dr.free()
        return t1, t2, n
    for name, data in files.items():
        assert readio.zstd_decompress(data) == text
        got, st0 = ctx.zstd_inflate(data)
        assert got == text, name
        del got
        n_ref = host_open(data)[2]
        assert dev_open(data, 1)[1] == n_ref == len(recs) and dev_open(data, 0)[1] == n_ref
        lib, parent, d1, d0 = [], [], [], []
        for r in range(a.repeats):
            t1, t2, _ = host_open(data)
            lib.append(t1); parent.append(t2)
            d1.append(dev_open(data, 1)[0]); d0.append(dev_open(data, 0)[0])
            print("%s repeat %d: libzstd %.3f s, host decode + open_reads %.3f s, device %.3f s (checksum on), %.3f s (off)" % (name, r + 1, t1, t2, d1[-1], d0[-1]), flush=True)
        ctx.set_option("ZSTD_CHECKSUM", 1)
        stages, st = stage_times(ctx, data)
        decode_ms = sum(v for k, v in stages.items() if k.endswith("_ms")) if "error" not in stages else None
        out["files"][name] = {
            "compressed_bytes": len(data), "stats": st,
            "libzstd_1thread": spread(lib), "host_decode_plus_open_reads": spread(parent),
            "device_open_reads_checksum_1": spread(d1), "device_open_reads_checksum_0": spread(d0),
            "device_vs_parent_way": round(statistics.median(parent) / statistics.median(d1), 2),
            "stages": stages, "checksum_ms": round(st["checksum_us"] / 1000.0, 3),
            "checksum_share_of_stage_sum": round(stages["checksum_ms"] / decode_ms, 3) if decode_ms else None,
        }
    ctx.set_option("ZSTD_CHECKSUM", None)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
