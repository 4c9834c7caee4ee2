#!/usr/bin/env python
"""What target names shared across target SHARDS cost (lrge_hip_overlap_twoset_tsharded): a world of N ranks emulated on
ONE GPU -- the ranks are threads that take turns (lrge_hip_comm_local_group_serialize), a rank's busy_ms is the time its share takes
on a GPU of its own, the step is the slowest rank's.  The target set is a config's targets followed by a copy of their first third
(a concatenated file), the copy under the SAME names (--names repeated) or under names of its own (--names renamed).

  --route collective   lrge_hip_index_build_tsharded + lrge_hip_overlap_twoset_tsharded (every rank maps all queries against its shard)
  --route qshard       the query-sharded forward form (lrge_hip_index_build_sharded + lrge_hip_overlap_twoset on the rank's queries,
                       one all-gather of the estimates): the only multi-GPU route for such a set before the collective call existed

A step is index build + overlap + estimates with the reads resident in HBM.  Prints one JSON line.  NOT a bench result.

  python tools/tshard_names_cost.py --config c5_human_tenth --preset pb --world 8 --route collective --names repeated
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c5_human_tenth")
    ap.add_argument("--preset", default="pb")
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--route", choices=["collective", "qshard"], default="collective")
    ap.add_argument("--names", choices=["repeated", "renamed"], default="repeated")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--join-s", type=float, default=240.0)
    a = ap.parse_args()
    from lrge_amd import engine, parallel, synth
    preset = 1 if a.preset == "pb" else 0
    t0 = time.perf_counter()
    _, q, t = synth.make_config(a.config)
    n3 = t.n // 3
    off = np.asarray(t.offsets, dtype=np.uint64)
    bases = np.concatenate([t.bases, t.bases[:int(off[n3])]])
    offs = np.concatenate([off, off[-1] + off[1:n3 + 1]])
    names = list(t.names) + (list(t.names[:n3]) if a.names == "repeated" else [b"copy%08d" % i for i in range(n3)])
    lens = np.diff(offs).astype(np.uint32)
    qr, tr = engine.name_ranks(q.names, names)
    sys.stderr.write("[tshard_names_cost] %d targets, %.2f Gbases, %d queries; data ready in %.1f s\n" % (len(lens), float(offs[-1]) / 1e9, q.n, time.perf_counter() - t0))
    W = a.world
    tb = parallel.shard_by_bases(lens, W)
    qb = parallel.shard_by_bases(q.lens(), W)
    avg_t = float(np.float32(lens.sum()) / np.float32(len(lens)))
    grp = parallel.LocalGroup(W)
    grp.serialize(True)
    res, errs = [None] * W, []

    def rank_main(r):
        comm = None
        try:
            c = engine.Context(0)
            comm = grp.comm(c, r)
            comm.turn(True)
            t0_, t1_ = tb[r], tb[r + 1]
            Td = c.upload(bases[int(offs[t0_]):int(offs[t1_])], offs[t0_:t1_ + 1] - offs[t0_], tr[t0_:t1_])
            if a.route == "collective":
                Qd, q_lens = c.upload(q.bases, q.offsets, qr), q.lens()
            else:
                sub = q.slice(qb[r], qb[r + 1])
                Qd, q_lens = c.upload(sub.bases, sub.offsets, qr[qb[r]:qb[r + 1]]), sub.lens()
            comm.turn(False)
            best = None
            for it in range(a.warmup + a.steps):
                if it == a.warmup:
                    comm.busy_ms(reset=True)
                before = comm.busy_ms()
                comm.turn(True)
                if a.route == "collective":
                    ix = engine.Index(c, Td, preset, comm=comm, tshard=True)
                    counts, has = ix.overlap_twoset_tsharded(Qd, comm)
                    tm, cn = c.timings(), c.counters()
                    est = c.estimates(counts, q_lens, avg_t, len(lens), 100)
                else:
                    ix = engine.Index(c, Td, preset, streamed=Qd, comm=comm, shard=(lens, tr, t0_))
                    counts, has = ix.overlap_twoset(Qd)
                    tm, cn = c.timings(), c.counters()
                    est = c.estimates(counts, q_lens, avg_t, len(lens), 100)
                    n_of = [qb[i + 1] - qb[i] for i in range(W)]
                    est = comm.all_gather_f32(est, max(n_of), n_of)
                ix.free()
                comm.turn(False)
                step = comm.busy_ms() - before
                if it >= a.warmup and (best is None or step < best[0]):
                    best = (step, tm, cn)
            res[r] = dict(rank=r, busy_ms_per_step=comm.busy_ms() / a.steps, best_step_busy_ms=best[0], overlap_call_ms=round(best[1]["total"], 3),
                          count_stage_ms=round(best[1]["count"], 3), shared_name_pairs=best[2]["shared_name_pairs"], shared_name_distinct=best[2]["shared_name_distinct"],
                          sum_counts=int(np.asarray(counts, dtype=np.int64).sum()), n_counts=len(counts), no_mapping=int((np.asarray(has) == 0).sum()),
                          est_finite=int(np.isfinite(est).sum()))
            Qd.free(); Td.free(); comm.close(); c.close()
        except Exception as e:      # noqa: BLE001 -- reported below; the peers must not wait for this rank
            errs.append((r, repr(e)))
            try:
                comm.abort(); comm.turn(False)
            except Exception:       # noqa: BLE001
                pass

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(W)]
    for t_ in th:
        t_.start()
    deadline = time.perf_counter() + a.join_s
    for t_ in th:
        t_.join(timeout=max(0.1, deadline - time.perf_counter()))
    if errs or any(t_.is_alive() for t_ in th):
        print(json.dumps({"errors": errs, "ranks_still_running": sum(t_.is_alive() for t_ in th)}))
        sys.stdout.flush()
        os._exit(1)
    grp.close()
    total = res[0]["sum_counts"] if a.route == "collective" else sum(x["sum_counts"] for x in res)
    print(json.dumps({"NOT_A_BENCH_RESULT": "all ranks on one GPU, taking turns", "config": a.config, "preset": "ava-pb" if preset else "ava-ont", "world": W,
                      "route": a.route, "names": a.names, "n_targets": int(len(lens)), "target_gbases": round(float(offs[-1]) / 1e9, 3), "n_queries": int(q.n),
                      "steps": a.steps, "warmup": a.warmup,
                      "slowest_rank_busy_ms_per_step": max(x["busy_ms_per_step"] for x in res), "slowest_rank_best_step_ms": max(x["best_step_busy_ms"] for x in res),
                      "slowest_rank_overlap_call_ms": max(x["overlap_call_ms"] for x in res),
                      "sum_counts_whole_job": total, "shared_name_pairs": sum(x["shared_name_pairs"] for x in res),
                      "shared_name_distinct": sum(x["shared_name_distinct"] for x in res), "ranks": res}))


if __name__ == "__main__":
    main()
