"""BGZF input decompression: the host path against the device path, on one seeded BGZF FASTQ (>= 4 GB uncompressed,
written by 16 processes).  Usage:  python tools/bgzf_bench.py [--gb 4] [--dir /tmp] [--out profiles/bgzf_inflate.json]

Four measurements of the same file:
  (a) today's host path: one zlib stream over the whole file on one thread (include/lrge_io.hpp gunzip_all does the same)
  (b) 16-thread host zlib over the BGZF blocks: the obvious alternative
  (c) the device path end to end: lrge_hip_bgzf_inflate (scan, pinned staging, upload / decode / download, copy out)
  (d) k_inflate alone, from `rocprofv3 --kernel-trace --stats` in a run of its own (--kernel-only, a child process)
plus the file read, and the records end to end through lrge_hip_read_records / lrge_hip_read_records_gpu (parse included;
the per-record Python callback is the same in both).  The record goes to --out as JSON."""
import argparse
import ctypes as C
import glob
import json
import multiprocessing as mp
import os
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PART = 256 << 20          # uncompressed bytes per writer task


def _part(args):
    """One task: ~256 MiB of FASTQ (seeded by the task index) as BGZF blocks, level 6 like bgzip."""
    import numpy as np
    import bgzf_writer as W
    idx, nbytes = args
    rng = np.random.default_rng(1000 + idx)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    out, n, k = [], 0, 0
    while n < nbytes:
        ln = int(rng.integers(500, 3000))
        seq = acgt[rng.integers(0, 4, ln)].tobytes()
        qual = (rng.integers(0, 3, ln, dtype=np.uint8) * 5 + 35).tobytes()
        rec = b"@p%d_r%d len=%d\n%s\n+\n%s\n" % (idx, k, ln, seq, qual)
        out.append(rec); n += len(rec); k += 1
    return W.bgzf_compress(b"".join(out), eof=False)


def write_file(path, gb):
    import bgzf_writer as W
    tasks = [(i, PART) for i in range((int(gb * (1 << 30)) + PART - 1) // PART)]
    t0 = time.perf_counter()
    with mp.get_context("spawn").Pool(16) as pool, open(path, "wb") as fh:
        for blob in pool.imap(_part, tasks):
            fh.write(blob)
        fh.write(W.EOF_BLOCK)
    return time.perf_counter() - t0


def block_table(data):
    """(offset, size, isize) of every member, from the BC subfield (bgzf_writer puts it first)."""
    out, off = [], 0
    while off < len(data):
        bsize = int.from_bytes(data[off + 16:off + 18], "little") + 1
        out.append((off, bsize, int.from_bytes(data[off + bsize - 4:off + bsize], "little")))
        off += bsize
    return out


def host_single(data, table):
    """(a): the members one after the other on one thread, like gunzip_all's one zlib stream (zlib's own cost per byte)."""
    mv = memoryview(data)
    return b"".join(zlib.decompress(mv[off:off + size], 31) for off, size, _ in table)


def host_threads(data, table, total, threads=16):
    """(b): blocks over 16 threads (zlib releases the GIL), each written to its output offset."""
    out = bytearray(total)
    mv = memoryview(data)
    starts, o = [], 0
    for _, _, isz in table:
        starts.append(o); o += isz
    step = (len(table) + threads - 1) // threads

    def work(t):
        for i in range(t * step, min(len(table), (t + 1) * step)):
            off, size, isz = table[i]
            out[starts[i]:starts[i] + isz] = zlib.decompress(mv[off:off + size], 31)
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(work, range(threads)))
    return out


def device(ctx, data, total):
    import numpy as np
    out = np.empty(max(1, total), np.uint8)
    t0 = time.perf_counter()
    ctx._check(ctx._lib.lrge_hip_bgzf_inflate(ctx.h, data, len(data), out.ctypes.data, total))
    return time.perf_counter() - t0, out


def records(fn, *args):
    CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_char), C.c_uint64, C.POINTER(C.c_char), C.c_uint64)
    n = [0]

    def cb(u, name, nl, b, bl):
        n[0] += 1
    f = CB(cb)
    t0 = time.perf_counter()
    rc = fn(*args, f)
    return rc, n[0], time.perf_counter() - t0


def kernel_only(path):
    from lrge_amd import engine
    with open(path, "rb") as fh:
        data = fh.read()
    ctx = engine.Context(0)
    total = C.c_uint64()
    assert ctx._lib.lrge_hip_bgzf_scan(data, len(data), None, C.byref(total)) == 0
    device(ctx, data, total.value)
    ctx.close()


def rocprof_kernel(path, tmp):
    d = os.path.join(tmp, "prof")
    cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run",
           "--", sys.executable, os.path.abspath(__file__), "--kernel-only", path]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return {"error": "rocprofv3 exit %d: %s" % (r.returncode, r.stderr[-400:])}
    import csv
    files = glob.glob(os.path.join(d, "**", "*.csv"), recursive=True)
    for f in files:
        if not f.endswith("kernel_stats.csv"):
            continue
        for row in csv.DictReader(open(f)):
            if "k_inflate" in row.get("Name", ""):
                return {"calls": int(row["Calls"]), "total_ns": int(float(row["TotalDurationNs"])),
                        "max_ns": int(float(row["MaxNs"])), "min_ns": int(float(row["MinNs"]))}
    return {"error": "no k_inflate row in the kernel statistics", "files": [os.path.relpath(f, d) for f in files]}


def log(rec, key):
    """one line per stage as it finishes (a long run stays visibly alive)"""
    print("[bgzf_bench] %s = %s" % (key, rec[key]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=4.0)
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_inflate.json"))
    ap.add_argument("--kernel-only")
    a = ap.parse_args()
    if a.kernel_only:
        return kernel_only(a.kernel_only)
    import numpy as np
    from lrge_amd import engine
    tmp = tempfile.mkdtemp(dir=a.dir)
    path = os.path.join(tmp, "reads.fq.gz")
    rec = {"gen_s": write_file(path, a.gb)}
    log(rec, "gen_s")
    t0 = time.perf_counter()
    with open(path, "rb") as fh:
        data = fh.read()
    rec["read_s"] = time.perf_counter() - t0
    rec["compressed_bytes"] = len(data)
    table = block_table(data)
    total = sum(t[2] for t in table)
    rec["blocks"], rec["uncompressed_bytes"] = len(table), total
    log(rec, "read_s"); log(rec, "uncompressed_bytes")

    t0 = time.perf_counter(); ref = host_single(data, table); rec["a_host_1thread_inflate_s"] = time.perf_counter() - t0
    assert len(ref) == total
    log(rec, "a_host_1thread_inflate_s")
    t0 = time.perf_counter(); alt = host_threads(data, table, total); rec["b_host_16thread_inflate_s"] = time.perf_counter() - t0
    assert alt == ref
    del alt
    log(rec, "b_host_16thread_inflate_s")
    ctx = engine.Context(0)
    s, out = device(ctx, data, total)                      # first call: code object load, pool growth
    rec["c_device_first_call_s"] = s
    s, out = device(ctx, data, total)
    rec["c_device_inflate_s"] = s
    log(rec, "c_device_first_call_s"); log(rec, "c_device_inflate_s")
    assert np.array_equal(out[:total], np.frombuffer(ref, np.uint8)), "device output differs from zlib"
    del out, ref
    L = ctx._lib
    CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_char), C.c_uint64, C.POINTER(C.c_char), C.c_uint64)
    L.lrge_hip_read_records.argtypes = [C.c_char_p, CB, C.c_void_p, C.c_char_p, C.c_uint64]
    L.lrge_hip_read_records_gpu.argtypes = [C.c_void_p, C.c_char_p, CB, C.c_void_p, C.POINTER(C.c_int)]
    used = C.c_int()
    rc, n_h, s_h = records(lambda f: L.lrge_hip_read_records(os.fsencode(path), f, None, None, 0))
    rc2, n_g, s_g = records(lambda f: L.lrge_hip_read_records_gpu(ctx.h, os.fsencode(path), f, None, C.byref(used)))
    assert rc == 0 and rc2 == 0 and n_h == n_g and used.value == 1
    rec.update(records=n_h, records_host_path_s=s_h, records_device_path_s=s_g)
    log(rec, "records_host_path_s"); log(rec, "records_device_path_s")
    ctx.close()
    rec["d_kernel"] = rocprof_kernel(path, tmp)
    os.remove(path)
    gbs = lambda sec: round(total / sec / 1e9, 2)
    rec["inflate_GBps"] = {"a_host_1thread": gbs(rec["a_host_1thread_inflate_s"]), "b_host_16thread": gbs(rec["b_host_16thread_inflate_s"]),
                           "c_device_end_to_end": gbs(rec["c_device_inflate_s"])}
    if "total_ns" in rec["d_kernel"]:
        rec["inflate_GBps"]["d_kernel"] = gbs(rec["d_kernel"]["total_ns"] / 1e9)
    rec["speedup_c_over_a"] = round(rec["a_host_1thread_inflate_s"] / rec["c_device_inflate_s"], 2)
    rec["speedup_c_over_b"] = round(rec["b_host_16thread_inflate_s"] / rec["c_device_inflate_s"], 2)
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
