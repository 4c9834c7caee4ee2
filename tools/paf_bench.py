"""overlaps.paf: the host path (-C) against the device path (-C --gpu-paf; lrge_hip_paf_text) on one MI355X.  Usage:
  python tools/paf_bench.py [--configs c2_bact_twoset,c5_human_tenth] [--presets ont,pb] [--reps 5] [--dir DIR] [--out profiles/paf_bench.json]

For every configuration (synth.make_config) and preset: the sets are uploaded, the index is built and the count pass
(overlap_twoset) runs, as in a -C run; then, one warm-up and the median of --reps calls each,
  host     tools/paf_host_bench.cpp: lrge_hip_chains (count), lrge_hip_chains (fill), lrge_hip_paf_stats, lrge::paf_format_lines and
           the file write, a clock around each;
  device   lrge_hip_paf_text with a sink that writes the file, the hint the strategies pass (lrge::paf_chain_hint of the counts): its
           wall clock as it runs (copies beside writes), and with option PAF_SERIAL the phases of lrge_hip_last_paf_phases --
           statistics, chains, measure, setup (the device text blocks and the two pinned pieces taken), write (scan + kernel), copy
           down, file write (the sink).  With --sliced-bytes the device calls are repeated with PAF_PIECE_BYTES that small: many slices.
Both files must hold the same multiset of lines.  Every clock is a host clock around work that ends in a device synchronise or in
host memory.  Writes one JSON file and prints both tables, with the line and byte counts and the chains per query."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOST_PHASES = ["chains_count_ms", "chains_fill_ms", "paf_stats_ms", "format_ms", "file_write_ms"]
DEV_PHASES = ["stats_us", "chains_us", "measure_us", "setup_us", "write_us", "copy_wait_us", "sink_us"]


def table(names):
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum(np.fromiter(map(len, names), dtype=np.uint64, count=len(names)), out=off[1:])
    return b"".join(names), off


def med(rows, key):
    return round(statistics.median(r[key] for r in rows), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2_bact_twoset,c5_human_tenth")
    ap.add_argument("--presets", default="ont,pb")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sliced-bytes", type=int, default=2 << 20, help="a second device measurement with PAF_PIECE_BYTES at this value (0: none)")
    ap.add_argument("--dir", default=None, help="where the two overlaps.paf go (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paf_bench.json"))
    a = ap.parse_args()
    import tempfile
    from lrge_amd import build as Bd, engine, synth
    H = C.CDLL(Bd.build_paf_host_bench())
    vp = C.c_void_p
    H.paf_host_bench.argtypes = [vp, vp, vp, C.c_int, C.c_char_p, vp, C.c_uint32, vp, C.c_char_p, vp, C.c_uint32, vp, C.c_char_p, vp, vp]
    work = a.dir or tempfile.mkdtemp(prefix="paf_bench_")
    os.makedirs(work, exist_ok=True)
    ctx = engine.Context(0)
    rows = []
    for cfg in a.configs.split(","):
        t0 = time.perf_counter()
        _, q, t = synth.make_config(cfg)
        print("%s: %d queries, %d targets drawn in %.0f s" % (cfg, q.n, t.n, time.perf_counter() - t0), flush=True)
        qr, tr = engine.name_ranks(q.names, t.names)
        Qd, Td = ctx.upload(q.bases, q.offsets, qr), ctx.upload(t.bases, t.offsets, tr)
        qb, qo = table(q.names)
        tb, to = table(t.names)
        qlen, tlen = q.lens().astype(np.uint32), t.lens().astype(np.uint32)
        for preset in a.presets.split(","):
            ix = engine.Index(ctx, Td, {"ont": 0, "pb": 1}[preset])
            counts, _ = ix.overlap_twoset(Qd)
            s = int(counts.sum())
            hint = s + s // 4 + 1024                      # lrge::paf_chain_hint
            host_path, dev_path = os.path.join(work, "host.paf"), os.path.join(work, "device.paf")

            def host_once():
                us, out = np.zeros(5, dtype=np.float64), np.zeros(2, dtype=np.uint64)
                t0 = time.perf_counter()
                rc = H.paf_host_bench(ctx.h, ix.h, Qd.h, 1, qb, qo.ctypes.data, q.n, qlen.ctypes.data, tb, to.ctypes.data, t.n, tlen.ctypes.data,
                                      host_path.encode(), us.ctypes.data, out.ctypes.data)
                assert rc == 0, (rc, ctx._lib.lrge_hip_last_error(ctx.h))
                r = dict(zip(HOST_PHASES, (us / 1e3).tolist()))
                r["total_ms"] = (time.perf_counter() - t0) * 1e3
                r["lines"], r["bytes"] = int(out[0]), int(out[1])
                return r

            def device_once(serial):
                ctx.set_option("PAF_SERIAL", "1" if serial else None)
                with open(dev_path, "wb") as fh:
                    t0 = time.perf_counter()
                    ix.paf_text_to(fh.write, Qd, q.names, t.names, dual=True, chain_hint=hint)
                    fh.flush()
                    ms = (time.perf_counter() - t0) * 1e3
                r = ctx.last_paf_stats()
                r["wall_ms"] = ms                         # (with the two name tables built in Python: not the library's time)
                return r
            host = [host_once() for _ in range(a.reps + 1)][1:]
            dev = [device_once(False) for _ in range(a.reps + 1)][1:]
            ser = [device_once(True) for _ in range(a.reps + 1)][1:]
            ctx.set_option("PAF_SERIAL", None)
            sliced = None
            if a.sliced_bytes:      # many slices: what the two pieces buy (copy down and file write of one slice beside the write of the next)
                ctx.set_option("PAF_PIECE_BYTES", str(a.sliced_bytes))
                d2 = [device_once(False) for _ in range(a.reps + 1)][1:]
                s2 = [device_once(True) for _ in range(a.reps + 1)][1:]
                ctx.set_option("PAF_SERIAL", None); ctx.set_option("PAF_PIECE_BYTES", None)
                sliced = dict(piece_bytes=a.sliced_bytes, slices=d2[0]["slices"], format_ms=round(statistics.median(r["format_us"] for r in d2) / 1e3, 3),
                              format_serial_ms=round(statistics.median(r["format_us"] for r in s2) / 1e3, 3),
                              total_ms=round(statistics.median(r["total_us"] for r in d2) / 1e3, 3),
                              total_serial_ms=round(statistics.median(r["total_us"] for r in s2) / 1e3, 3))
            same = sorted(open(host_path, "rb").read().split(b"\n")) == sorted(open(dev_path, "rb").read().split(b"\n"))
            row = dict(config=cfg, preset=preset, queries=q.n, targets=t.n, lines=host[0]["lines"], bytes=host[0]["bytes"],
                       chains_per_query=round(host[0]["lines"] / max(q.n, 1), 2), counted_overlaps=s, hint=hint, same_lines=same,
                       chain_runs=dev[0]["chain_runs"], slices=dev[0]["slices"], record_bytes_held=48 * dev[0]["records"], reps=a.reps,
                       host={k: med(host, k) for k in HOST_PHASES + ["total_ms"]},
                       device=dict(total_ms=round(statistics.median(r["total_us"] for r in dev) / 1e3, 3), wall_ms=med(dev, "wall_ms"),
                                   format_ms=round(statistics.median(r["format_us"] for r in dev) / 1e3, 3)),
                       device_sliced=sliced,
                       device_serial=dict({k.replace("_us", "_ms"): round(statistics.median(r[k] for r in ser) / 1e3, 3) for k in DEV_PHASES + ["total_us"]}))
            rows.append(row)
            print(json.dumps(row), flush=True)
            assert same, "the two files differ"
            assert dev[0]["lines"] == host[0]["lines"] and dev[0]["bytes"] == host[0]["bytes"]
            ix.free()
        Qd.free(); Td.free()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rows, fh, indent=1)
    print("\nhost path (ms, median of %d)" % a.reps)
    print("| config | preset | lines | MB | chains/query | chains (count) | chains (fill) | paf_stats | format | file write | total |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        h = r["host"]
        print("| %s | %s | %d | %.1f | %.1f | %s | %s |" % (r["config"], r["preset"], r["lines"], r["bytes"] / 1e6, r["chains_per_query"],
                                                             " | ".join("%.1f" % h[k] for k in HOST_PHASES), "%.1f" % h["total_ms"]))
    print("\ndevice path (ms, median of %d; phases with PAF_SERIAL, total as it runs)" % a.reps)
    print("| config | preset | chain runs | slices | record MB held | statistics | chains | measure | setup | write | copy down | file write | total (serial) | total |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        d = r["device_serial"]
        print("| %s | %s | %d | %d | %.1f | %s | %.1f | %.1f |" % (r["config"], r["preset"], r["chain_runs"], r["slices"], r["record_bytes_held"] / 1e6,
                                                           " | ".join("%.1f" % d[k.replace("_us", "_ms")] for k in DEV_PHASES), d["total_ms"], r["device"]["total_ms"]))
    if a.sliced_bytes:
        print("\ndevice path with PAF_PIECE_BYTES=%d (ms): measure + write + deliver, and the whole call, as it runs and serial" % a.sliced_bytes)
        print("| config | preset | slices | format | format (serial) | total | total (serial) |")
        print("|---|---|---|---|---|---|---|")
        for r in rows:
            d = r["device_sliced"]
            print("| %s | %s | %d | %.1f | %.1f | %.1f | %.1f |" % (r["config"], r["preset"], d["slices"], d["format_ms"], d["format_serial_ms"], d["total_ms"], d["total_serial_ms"]))


if __name__ == "__main__":
    main()
