"""xz input: the device decode (lrge_hip_xz_inflate; lrge_hip_reads_open* | LRGE_GPU_INFLATE_XZ: decode to HBM and record scan)
against liblzma on one thread (the library behind the host reader's unxz_all, here through Python's binding) and against the way to
the same resident read set without the flag (host decode, then open_reads of the plain text), on a FASTQ of the counter-based
generator's reads (lrge_amd/synth_cb.py) compressed at preset 6.  Usage:
  python tools/xz_bench.py [--mb 48] [--repeats 5] [--block-mb 24] [--out profiles/xz_bench.json]

Files: the text in blocks of --block-mb (24 MiB is what `xz -6 -T` writes: three times the 8 MiB dictionary), and the same text cut
into 64 equal blocks, of which the first 1, 8 and all 64 are taken: the parallelism of the decode is the number of blocks, so these
say from which block count on the device wins.  Clock: from the compressed bytes in memory to the last decompressed byte on the
host (lrge_hip_xz_inflate, liblzma) or to the read set open on the device.  One warm-up of each, then `repeats` rounds that
alternate the sides in the same process; medians with ranges, and the stage times of lrge_hip_xz_stats (walk, decode, check)."""
import argparse
import concurrent.futures
import json
import lzma
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def payload(part):
    return lzma.compress(part, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "preset": 6}])


def spread(v):
    return {"median_s": round(statistics.median(v), 4), "min_s": round(min(v), 4), "max_s": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=48.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--block-mb", type=float, default=24.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xz_bench.json"))
    a = ap.parse_args()
    import xz_corpus as X
    import xz_writer as XW
    from zstd_bench import fastq
    t0 = time.perf_counter()
    recs = fastq(int(a.mb * (1 << 20)))
    text = b"".join(recs)
    print("text %d bytes in %d records, made in %.1f s" % (len(text), len(recs), time.perf_counter() - t0), flush=True)
    # blocks cut between records, compressed side by side (the workers never open the device)
    def cut(n_bytes):
        parts, cur, size = [], [], 0
        for r in recs:
            cur.append(r); size += len(r)
            if size >= n_bytes:
                parts.append(b"".join(cur)); cur, size = [], 0
        if cur:
            parts.append(b"".join(cur))
        return parts
    big, small = cut(int(a.block_mb * (1 << 20))), cut(-(-len(text) // 64))
    t0 = time.perf_counter()
    with concurrent.futures.ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        big_p, small_p = list(pool.map(payload, big)), list(pool.map(payload, small))
    d8m = XW.dict_byte(8 << 20)
    files = {"blocks_of_%g_mib_all_%d" % (a.block_mb, len(big)): (XW.stream(list(zip(big_p, big)), XW.CHECK_CRC64, dict_b=d8m), text)}
    for k in (1, 8, len(small)):
        files["blocks_64th_first_%d" % k] = (XW.stream(list(zip(small_p[:k], small[:k])), XW.CHECK_CRC64, dict_b=d8m), b"".join(small[:k]))
    print("compressed in %.1f s: %s" % (time.perf_counter() - t0, {k: len(v[0]) for k, v in files.items()}), flush=True)
    from lrge_amd import _ffi, engine
    ctx = engine.Context(0)
    flags = _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP
    out = {"uncompressed_bytes": len(text), "records": len(recs), "repeats": a.repeats, "preset": 6, "files": {}}

    def timed(f):
        t = time.perf_counter()
        r = f()
        return time.perf_counter() - t, r

    def dev_open(data, fl):
        t = time.perf_counter()
        dr = ctx.open_reads(data, fl)
        t = time.perf_counter() - t
        n = dr.n
        dr.free()
        return t, n
    for name, (data, plain) in files.items():
        w = X.walk(data)
        got, st = ctx.xz_inflate(data)                                   # (the warm-up of the device, and the proof of the bytes)
        assert got == plain and X.decompress(data) == plain, name
        del got
        n_ref = dev_open(plain, flags)[1]
        assert dev_open(data, flags | _ffi.GPU_INFLATE_XZ)[1] == n_ref
        lib, parent, inflate, opened, stages = [], [], [], [], []
        for r in range(a.repeats):
            t1, p = timed(lambda: X.decompress(data))
            t2 = t1 + dev_open(p, flags)[0]
            del p
            lib.append(t1); parent.append(t2)
            t3, (_, st) = timed(lambda: ctx.xz_inflate(data))
            inflate.append(t3); stages.append(st)
            opened.append(dev_open(data, flags | _ffi.GPU_INFLATE_XZ)[0])
            print("%s repeat %d: liblzma %.3f s, host decode + open_reads %.3f s, device inflate %.3f s, device open_reads %.3f s" % (name, r + 1, t1, t2, t3, opened[-1]),
                  flush=True)
        med = lambda k: round(statistics.median(s[k] for s in stages) / 1000.0, 3)
        out["files"][name] = {
            "compressed_bytes": len(data), "uncompressed_bytes": len(plain), "blocks": w["blocks"], "chunks": w["chunks"], "stats": stages[-1],
            "liblzma_1thread": spread(lib), "host_decode_plus_open_reads": spread(parent), "device_xz_inflate": spread(inflate),
            "device_open_reads": spread(opened), "device_vs_parent_way": round(statistics.median(parent) / statistics.median(opened), 3),
            "liblzma_mb_per_s": round(len(plain) / statistics.median(lib) / 1e6, 1), "device_inflate_mb_per_s": round(len(plain) / statistics.median(inflate) / 1e6, 1),
            "stages_ms": {"walk": med("walk_us"), "decode": med("decode_us"), "check": med("check_us")},
            "decode_mb_per_s_per_block": round(len(plain) / w["blocks"] / (statistics.median(s["decode_us"] for s in stages) / 1e6) / 1e6, 2),
        }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
