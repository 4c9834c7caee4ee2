"""Identifier ranks: the host sorts the callers run today against the device call (lrge_hip_name_ranks).  Usage:
  python tools/names_bench.py [--sizes 15000,200000,2100000] [--out profiles/names_bench.json]

For n identifiers of two kinds -- UUID-like (36 bytes) and PacBio-like (m64011_190830_220126/<zmw>/ccs), the shapes of
tests/test_names_twin.py, formatted from one seeded generator -- it times
  python   engine.name_ranks (a Python `sorted` over a list of bytes), best of 3, one run at a million names and above;
  cpp      names_lsd_host_sort_ranks of the twin library, the std::sort form of detail::name_ranks, best of 3;
  device   lrge_hip_name_ranks on the table of all names (idx NULL), one warm-up, then best of 5: the call's own stats[3]
           (gather, transfer, sorts, read-back) and the wall clock around the ctypes call.
The three rank vectors must be equal.  Every clock starts with the names as one blob plus offsets in host memory (python: as a
list of bytes) and ends with the ranks in host memory.  Writes one JSON file and prints a table."""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def uuid_names(rng, n):
    out = []
    for _ in range(n):
        h = b"%032x" % rng.getrandbits(128)
        out.append(h[:8] + b"-" + h[8:12] + b"-" + h[12:16] + b"-" + h[16:20] + b"-" + h[20:])
    return out


def pacbio_names(rng, n):
    return [b"m64011_190830_220126/%d/ccs" % z for z in rng.sample(range(1, 180_000_000), n)]


def best(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        t.append(time.perf_counter() - t0)
    return min(t), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="15000,200000,2100000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "names_bench.json"))
    a = ap.parse_args()
    from lrge_amd import build as Bd, engine
    T = C.CDLL(Bd.build_names_lsd_twin())
    T.names_lsd_host_sort_ranks.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    ctx = engine.Context(0)
    rows = []
    for n in [int(x) for x in a.sizes.split(",")]:
        for kind, gen in (("uuid", uuid_names), ("pacbio", pacbio_names)):
            names = gen(random.Random(n), n)
            blob = b"".join(names)
            off = np.zeros(n + 1, dtype=np.uint64)
            np.cumsum(np.fromiter(map(len, names), dtype=np.uint64, count=n), out=off[1:])
            t_py, (r_py,) = best(lambda: engine.name_ranks(names), 1 if n >= 1_000_000 else 3)
            r_cpp = np.zeros(n, dtype=np.uint32)
            t_cpp, rc = best(lambda: T.names_lsd_host_sort_ranks(blob, off.ctypes.data, n, None, n, r_cpp.ctypes.data), 3)
            assert rc == 0
            r_dev = np.zeros(n, dtype=np.uint32)
            st = np.zeros(4, dtype=np.uint64)
            call = lambda: ctx._lib.lrge_hip_name_ranks(ctx.h, blob, off.ctypes.data, n, None, n, r_dev.ctypes.data, st.ctypes.data)   # noqa: E731
            assert call() == 0, ctx._lib.lrge_hip_last_error(ctx.h)
            walls, calls = [], []
            for _ in range(5):
                t0 = time.perf_counter()
                assert call() == 0
                walls.append(time.perf_counter() - t0)
                calls.append(int(st[3]) * 1e-6)
            assert np.array_equal(r_py, r_cpp) and np.array_equal(r_py, r_dev), (n, kind)
            row = dict(n=n, kind=kind, name_bytes=len(blob), words=int(st[1]), sorts=int(st[0]), distinct=int(st[2]),
                       python_ms=round(t_py * 1e3, 3), cpp_ms=round(t_cpp * 1e3, 3), device_call_ms=round(min(calls) * 1e3, 3),
                       device_wall_ms=round(min(walls) * 1e3, 3))
            rows.append(row)
            print(row, flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(dict(tool="tools/names_bench.py", rows=rows), fh, indent=1)
        fh.write("\n")
    print("| n | kind | W | engine.name_ranks ms | C++ host sort ms | device call ms (stats[3]) | device wall ms |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %d | %s | %d | %.1f | %.1f | %.2f | %.2f |" % (r["n"], r["kind"], r["words"], r["python_ms"], r["cpp_ms"], r["device_call_ms"], r["device_wall_ms"]))


if __name__ == "__main__":
    main()
