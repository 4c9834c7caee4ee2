"""GPU: lrge_hip_overlap_twoset_tsharded -- forward two-set with the TARGETS sharded over the ranks of a world, a target name counted
once per query whichever shards bear it.  The reference inserts target_name into a HashSet per query (twoset.rs:286-317); a shard
sees only its own reads, so a kept mapping onto a bearer of a name that also lives in another shard leaves a (query, name) pair, the
distinct pairs travel to the rank that owns the query and are counted there once (k_count_shared, k_pair_cuts, k_name_pairs_count).
Every rank must hold exactly what ONE index over all targets gives, and what the oracle gives.

The ranks are threads of this process on one GPU (as in tests/test_gpu_multi.py), each with a context of its own; every thread is
joined with a time limit, so a rank stuck in a collective fails the test instead of hanging it.  Target sets, helpers and the read
batches are those of tests/test_gpu_shared_names.py; no seed had to be changed (the non-vacuity checks below hold for the
committed sample as it is)."""
import threading

import numpy as np
import pytest

from test_gpu_shared_names import PRESETS, _case, make_set, part_bases_for, part_of, to_arrays  # noqa: F401 -- make_set via _case

pytestmark = pytest.mark.gpu

JOIN_S = 120
COUNTERS_OFF_PATH = ("lookup_launches", "batches", "rs_scatter_launches")


@pytest.fixture(scope="module")
def rank_ctxs():
    """one context per rank of the largest world, made once for the module"""
    from lrge_amd import engine
    cs = [engine.Context(0) for _ in range(8)]
    yield cs
    for c in cs:
        c.close()


def case(ctx, oracle, tiny_ont, tiny_hifi, kind, preset):
    """the set, the single index's and the oracle's answers (computed once per (kind, preset) by test_gpu_shared_names._case); the
    uploads it makes on the session context are not used here and go back at once"""
    c, Qd, Td = _case(ctx, oracle, tiny_ont, tiny_hifi, kind, preset)
    Qd.free(); Td.free()
    return c


def run_world(rank_ctxs, world, c, preset, bounds=None, nq=None, F=False, opts=None, plain_index_on=None):
    """Every rank r in a thread: uploads targets [bounds[r], bounds[r + 1]) of case `c` and the first nq queries, builds its
    target-sharded index, runs the OLD route (plain overlap_twoset; the caller sums) and the collective call.
    -> per rank dict(old=(counts, has), old_cn, new=(counts, has), new_cn) or dict(code=error code of the collective call)"""
    from lrge_amd import _ffi, engine, parallel
    ds, seqs, names = c["ds"], c["seqs"], c["names"]
    qr, tr = engine.name_ranks(ds.q.names, names)
    bounds = bounds or parallel.shard_by_bases(c["lens"], world)
    q = ds.q if nq is None else ds.q.slice(0, nq)
    grp = parallel.LocalGroup(world)
    out, errs = [None] * world, []

    def rank_main(r):
        cx = rank_ctxs[r]
        try:
            for k, v in (opts or {}).items():
                cx.set_option(k, v)
            comm = grp.comm(cx, r)
            t0, t1 = bounds[r], bounds[r + 1]
            b, o = to_arrays(seqs[t0:t1])
            Td = cx.upload(b, o, tr[t0:t1])
            Qd = cx.upload(q.bases, q.offsets, qr[:q.n])
            ix = engine.Index(cx, Td, PRESETS[preset], comm=comm, tshard=True)
            res = {}
            res["old"] = tuple(x.copy() for x in ix.overlap_twoset(Qd, remove_internal=F))
            res["old_cn"] = cx.counters()
            use = ix
            if plain_index_on == r:
                use = engine.Index(cx, Td, PRESETS[preset])
            try:
                res["new"] = tuple(x.copy() for x in use.overlap_twoset_tsharded(Qd, comm, remove_internal=F))
                res["new_cn"] = cx.counters()
            except _ffi.LrgeHipError as e:
                res["code"] = e.code
            if use is not ix:
                use.free()
            ix.free(); Qd.free(); Td.free()
            comm.close()
            out[r] = res
        except Exception as e:      # noqa: BLE001 -- reported by the main thread
            errs.append((r, repr(e)))
        finally:
            for k in (opts or {}):
                cx.set_option(k, None)

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=JOIN_S)
    assert not any(t.is_alive() for t in th), "a rank outlived its join limit (stuck in a collective?)"
    grp.close()
    assert not errs, errs
    assert all(o is not None for o in out), "a rank did not finish"
    return out, bounds


def check_exact(out, c, F=False, nq=None):
    """every rank holds the counts and has_mapping of the single index and of the oracle"""
    for r, res in enumerate(out):
        assert "new" in res, (r, res.get("code"))
        for ref in (c["single"][F], c["oracle"][F]):
            assert np.array_equal(res["new"][0], ref[0][:nq]), (r, F, np.nonzero(res["new"][0] != ref[0][:nq])[0][:10])
            assert np.array_equal(res["new"][1], ref[1][:nq]), (r, F)


def old_way(out):
    return sum(res["old"][0].astype(np.int64) for res in out)


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("preset", ["ont", "pb"])
@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_shards_count_a_shared_name_once(ctx, oracle, rank_ctxs, tiny_ont, tiny_hifi, kind, preset, world):
    c = case(ctx, oracle, tiny_ont, tiny_hifi, kind, preset)
    out, _ = run_world(rank_ctxs, world, c, preset)
    check_exact(out, c)
    pairs = sum(res["new_cn"]["shared_name_pairs"] for res in out)
    distinct = sum(res["new_cn"]["shared_name_distinct"] for res in out)
    print(kind, preset, world, "pairs", pairs, "distinct", distinct, "queries the old way gets wrong", int(np.sum(old_way(out) != c["single"][False][0])))
    # non-vacuity: plain overlap_twoset per rank, summed, counts some name once per shard
    assert np.any(old_way(out) != c["single"][False][0]), "the old way is right on this set: the comparison shows nothing"
    assert np.all(old_way(out) >= c["single"][False][0])
    assert pairs > 0
    assert 0 < distinct <= pairs


@pytest.mark.parametrize("nq", [1, 2])
def test_fewer_queries_than_ranks(ctx, oracle, rank_ctxs, tiny_ont, tiny_hifi, nq):
    """world 3, one or two queries: some owners' ranges are empty (pair_owner.h: [0, 0), [0, 0), [0, 1) at nq = 1)"""
    from lrge_amd import parallel
    c = case(ctx, oracle, tiny_ont, tiny_hifi, "a", "ont")
    out, _ = run_world(rank_ctxs, 3, c, "ont", nq=nq)
    check_exact(out, c, nq=nq)
    # non-vacuity: pairs were emitted, on more than one rank (so some crossed), and the old way is wrong on these very queries
    assert sum(res["new_cn"]["shared_name_pairs"] for res in out) > 0
    assert [res["new_cn"]["shared_name_pairs"] > 0 for res in out].count(True) >= 2
    assert np.any(old_way(out) != c["single"][False][0][:nq])
    owners = [r for r, res in enumerate(out) if res["new_cn"]["shared_name_distinct"] > 0]
    b = parallel.pair_owner_bounds(nq, 3)
    assert owners and all(b[r] < b[r + 1] for r in owners) and len(owners) <= nq        # only ranks that own a query counted anything


def test_repeats_on_one_rank_only(ctx, oracle, rank_ctxs, tiny_ont, tiny_hifi):
    """set "one-part", cut where its first part ends: only rank 0 bears repeats, no name is in two shards, no pair exists"""
    from lrge_amd import engine, parallel
    c = case(ctx, oracle, tiny_ont, tiny_hifi, "one-part", "ont")
    p2 = part_of(c["lens"], part_bases_for(c["lens"], 2))
    bounds = [0, int(np.sum(p2 == 0)), len(c["lens"])]
    _, tr = engine.name_ranks(c["ds"].q.names, c["names"])
    assert not parallel.cross_shard_duplicates(tr, bounds) and len(set(tr[:bounds[1]])) < bounds[1] and len(set(tr[bounds[1]:])) == bounds[2] - bounds[1]
    out, _ = run_world(rank_ctxs, 2, c, "ont", bounds=bounds)
    check_exact(out, c)
    assert np.array_equal(old_way(out), c["single"][False][0])
    for res in out:
        assert res["new_cn"]["shared_name_pairs"] == 0 and res["new_cn"]["shared_name_distinct"] == 0


def test_a_small_pair_buffer_is_flushed_and_grown_before_the_exchange(ctx, oracle, rank_ctxs, tiny_ont, tiny_hifi):
    c = case(ctx, oracle, tiny_ont, tiny_hifi, "a", "ont")
    ref, _ = run_world(rank_ctxs, 2, c, "ont")
    out, _ = run_world(rank_ctxs, 2, c, "ont", opts={"DEBUG_NAME_PAIRS_CAP": "4"})
    check_exact(out, c)
    for a, b in zip(out, ref):      # what was emitted and what is distinct do not depend on how the buffer was managed
        assert a["new_cn"]["shared_name_pairs"] == b["new_cn"]["shared_name_pairs"] > 4
        assert a["new_cn"]["shared_name_distinct"] == b["new_cn"]["shared_name_distinct"]


@pytest.mark.parametrize("preset", ["ont", "pb"])
def test_names_shared_across_parts_and_across_shards(ctx, oracle, rank_ctxs, tiny_ont, tiny_hifi, preset):
    """set c at world 2, every shard's index in (at least) 2 parts: one call settles names shared by the parts of a shard and by the shards"""
    from lrge_amd import engine, parallel
    c = case(ctx, oracle, tiny_ont, tiny_hifi, "c", preset)
    bounds = parallel.shard_by_bases(c["lens"], 2)
    pb = max(part_bases_for(c["lens"][bounds[r]:bounds[r + 1]], 2) for r in range(2))
    _, tr = engine.name_ranks(c["ds"].q.names, c["names"])
    across_parts = False
    for r in range(2):
        sub = tr[bounds[r]:bounds[r + 1]]
        parts = part_of(c["lens"][bounds[r]:bounds[r + 1]], pb)
        across_parts |= any(len(set(parts[sub == x])) > 1 for x in set(sub))
    assert across_parts and parallel.cross_shard_duplicates(tr, bounds)
    out, _ = run_world(rank_ctxs, 2, c, preset, opts={"PART_BASES": str(pb)})
    check_exact(out, c)
    assert all(res["new_cn"]["index_parts"] >= 2 for res in out)
    assert sum(res["new_cn"]["shared_name_pairs"] for res in out) > 0


def test_queries_in_views(ctx, oracle, rank_ctxs, tiny_ont, tiny_hifi):
    c = case(ctx, oracle, tiny_ont, tiny_hifi, "b", "ont")
    qb = int(c["ds"].q.lens().sum())
    out, _ = run_world(rank_ctxs, 3, c, "ont", opts={"STREAM_BASES": str(qb // 3 + 1)})
    check_exact(out, c)
    assert all(res["new_cn"]["lookup_launches"] >= 3 for res in out)
    assert sum(res["new_cn"]["shared_name_pairs"] for res in out) > 0


@pytest.mark.parametrize("kind", ["a", "c"])
def test_remove_internal(ctx, oracle, rank_ctxs, tiny_ont, tiny_hifi, kind):
    """-F: against the oracle run with remove_internal"""
    c = case(ctx, oracle, tiny_ont, tiny_hifi, kind, "ont")
    out, _ = run_world(rank_ctxs, 3, c, "ont", F=True)
    check_exact(out, c, F=True)


def test_world_of_one(ctx, oracle, rank_ctxs, tiny_ont, tiny_hifi):
    c = case(ctx, oracle, tiny_ont, tiny_hifi, "b", "ont")
    out, _ = run_world(rank_ctxs, 1, c, "ont")
    check_exact(out, c)
    assert np.array_equal(out[0]["new"][0], out[0]["old"][0]) and np.array_equal(out[0]["new"][1], out[0]["old"][1])
    assert out[0]["new_cn"]["shared_name_pairs"] == 0


@pytest.mark.parametrize("world", [2, 8])
def test_the_path_is_not_taken(ctx, oracle, rank_ctxs, tiny_ont, tiny_hifi, world):
    """all names distinct: the plain target-sharded route (overlap_twoset, the caller's all-reduce) and the collective call agree, and
    each rank launches what overlap_twoset launches on the same context and index"""
    c = case(ctx, oracle, tiny_ont, tiny_hifi, "distinct", "ont")
    out, _ = run_world(rank_ctxs, world, c, "ont")
    check_exact(out, c)
    plain_c = old_way(out)
    plain_h = (sum(res["old"][1].astype(np.int64) for res in out) > 0).astype(np.uint32)
    for res in out:
        assert np.array_equal(res["new"][0], plain_c) and np.array_equal(res["new"][1], plain_h)
        for k in COUNTERS_OFF_PATH:
            assert res["new_cn"][k] == res["old_cn"][k], k
        assert res["new_cn"]["shared_name_pairs"] == 0 and res["new_cn"]["shared_name_distinct"] == 0


def test_a_refusal_on_one_rank_is_the_refusal_of_every_rank(ctx, oracle, rank_ctxs, tiny_ont, tiny_hifi):
    """rank 1 of 3 passes an index that lrge_hip_index_build_tsharded did not build: LRGE_ERR_INVALID on every rank, nobody waits"""
    from lrge_amd import _ffi
    c = case(ctx, oracle, tiny_ont, tiny_hifi, "a", "ont")
    out, _ = run_world(rank_ctxs, 3, c, "ont", plain_index_on=1)
    assert [res.get("code") for res in out] == [_ffi.ERR_INVALID] * 3, out
