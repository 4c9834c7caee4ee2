"""CPU: the host side of lrge_hip_overlap_twoset_tsharded -- the forward strategy with the targets sharded, a target name counted
once per query whichever shards bear it (twoset.rs:286-317).  The ownership rule of the (query, name) pairs, the new symbol through
every layer of the ABI, and the `count_shared` form of parallel.twoset_forward_target_sharded."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from lrge_amd import parallel
from test_abi import _c_decls, _rs_decls

SYM = "lrge_hip_overlap_twoset_tsharded"
T_RANKS = np.array([0, 1, 2, 3, 4, 2, 6, 7])      # name 2 in both shards of the two-rank world below


class World2(parallel.SoloComm):
    """the two-rank stub world of tests/test_host_mirror.py: rank 0 of 2, collectives that return their input"""
    rank, world = 0, 2


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_pair_owner_bounds_tile_the_queries(world):
    for nq in (0, 1, world - 1, world, world + 1, 2 ** 32 - 1):
        b = parallel.pair_owner_bounds(nq, world)
        assert len(b) == world + 1 and b[0] == 0 and b[-1] == nq, (nq, world, b)
        assert all(b[r] <= b[r + 1] for r in range(world)), (nq, world, b)              # rank order, no overlap, no gap
        assert all(b[r] == r * nq // world for r in range(world + 1))                    # the rule of csrc/pair_owner.h
        sizes = [b[r + 1] - b[r] for r in range(world)]
        assert sum(sizes) == nq and max(sizes) - min(sizes) <= 1, (nq, world, sizes)
        # every query has exactly one owner
        for q in {0, nq // 2, nq - 1} if nq else ():
            assert sum(b[r] <= q < b[r + 1] for r in range(world)) == 1


def test_pair_owner_header_computes_the_same_bounds(tmp_path):
    """csrc/pair_owner.h compiled as host code (the __host__ __device__ markers defined away) against parallel.pair_owner_bounds"""
    import subprocess
    src = tmp_path / "po.cpp"
    src.write_text('#define __host__\n#define __device__\n#include "pair_owner.h"\n#include <cstdio>\n#include <cstdlib>\n'
                   'int main(int c, char **v) { for (int i = 1; i + 1 < c; i += 2) { unsigned long long nq = strtoull(v[i], 0, 10), w = strtoull(v[i + 1], 0, 10);\n'
                   '  for (unsigned long long r = 0; r <= w; ++r) printf("%llu ", pair_owner_first(r, nq, w)); printf("\\n"); } return 0; }\n')
    exe = tmp_path / "po"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "lrge_amd", "csrc"), "-o", str(exe), str(src)])
    cases = [(nq, w) for w in (1, 2, 3, 8, 16) for nq in (0, 1, w - 1, w, w + 1, 12345, 2 ** 32 - 1)]
    out = subprocess.check_output([str(exe)] + [str(x) for c in cases for x in c], text=True).strip().split("\n")
    assert len(out) == len(cases)
    for (nq, w), line in zip(cases, out):
        assert [int(x) for x in line.split()] == parallel.pair_owner_bounds(nq, w), (nq, w)
    assert '#include "pair_owner.h"' in open(os.path.join(ROOT, "lrge_amd", "csrc", "k_chain.h")).read()      # the kernel uses this rule


def test_the_symbol_through_every_layer():
    from lrge_amd import _ffi
    c = _c_decls()
    assert SYM in c, "include/lrge_hip.h does not declare " + SYM
    assert c[SYM] == ("i32", ["ptr"] * 7)
    hdr = open(os.path.join(ROOT, "include", "lrge_hip.h")).read()
    comment = hdr[:hdr.index("int  " + SYM)].rsplit("/*", 1)[1]
    assert "twoset.rs:286-317" in comment                                                 # cites the reference like its neighbours
    L = _ffi.lib()
    assert hasattr(L, SYM), "liblrge_hip.so does not export " + SYM
    assert SYM in _ffi.EXPORTS and len(getattr(L, SYM).argtypes) == 7
    rs, txt = _rs_decls()
    assert SYM in rs, "the Rust shim does not declare " + SYM
    assert rs[SYM] == c[SYM]
    assert re.search(r"check!\([^;]*%s\(" % SYM, txt), "the shim declares the call but never makes it"


def test_count_shared_does_not_refuse_and_returns_the_collective_result():
    lens = np.full(8, 100)
    assert parallel.cross_shard_duplicates(T_RANKS, parallel.shard_by_bases(lens, 2))
    counts, has = np.array([3, 0, 7], np.uint32), np.array([2, 0, 1], np.uint32)
    seen = []

    def collective(lo, hi):
        seen.append((lo, hi))
        return counts, has
    got_c, got_h, rng = parallel.twoset_forward_target_sharded(collective, lens, World2(), t_ranks=T_RANKS, count_shared=True)
    assert seen == [(0, 4)] and rng == (0, 4)
    assert np.array_equal(got_c, counts) and got_c.dtype == np.uint32
    assert np.array_equal(got_h, [1, 0, 1])                                               # 0 / 1
    # with build_fn: overlap_fn gets the index
    got_c, _, _ = parallel.twoset_forward_target_sharded(lambda ix: (counts + ix, has), lens, World2(), n_queries=3, build_fn=lambda lo, hi: 10,
                                                         t_ranks=T_RANKS, count_shared=True)
    assert np.array_equal(got_c, counts + 10)


def test_count_shared_does_not_reduce_the_counts_again():
    """the collective call has summed the counts already: only the one-word status agreement is left"""
    class Doubling(World2):
        calls = []

        def all_reduce_u32(self, a):
            self.calls.append(len(a))
            return np.asarray(a, np.uint32) * 2       # (a world whose two ranks contribute the same)
    counts = np.array([5, 1], np.uint32)
    # status 0 doubled is still 0; counts must come back untouched
    got_c, _, _ = parallel.twoset_forward_target_sharded(lambda lo, hi: (counts, counts), np.full(8, 100), Doubling(), t_ranks=T_RANKS, count_shared=True)
    assert np.array_equal(got_c, counts) and Doubling.calls == [1]


def test_count_shared_status_agreement_after_the_collective_call():
    """a rank that has LEFT the collective call and then fails alone (here: the shape of what it returned) says so in the status
    word; a peer's word makes this rank raise RankFailed"""
    class Peer(World2):
        def all_reduce_u32(self, a):
            return np.asarray(a, np.uint32) + 1       # (the other rank failed)
    with pytest.raises(parallel.RankFailed):
        parallel.twoset_forward_target_sharded(lambda lo, hi: (np.zeros(2, np.uint32),) * 2, np.full(8, 100), Peer(), t_ranks=T_RANKS, count_shared=True)

    class Log(World2):
        words, aborted = [], 0

        def all_reduce_u32(self, a):
            self.words.append(list(a)); return np.asarray(a, np.uint32)

        def abort(self):
            Log.aborted += 1
    with pytest.raises(ValueError):
        parallel.twoset_forward_target_sharded(lambda lo, hi: (np.zeros(2, np.uint32), np.zeros(3, np.uint32)), np.full(8, 100), Log(), t_ranks=T_RANKS, count_shared=True)
    assert Log.words == [[1]] and Log.aborted == 0


def test_count_shared_a_failure_inside_the_collective_aborts_and_enters_nothing():
    """overlap_fn and build_fn are collective: a rank that fails in either has peers inside that collective, so it aborts the
    communicator (which wakes them) and raises -- it must NOT enter the status all-reduce, which its peers are not at"""
    class Log(World2):
        def __init__(self):
            self.reduces, self.aborts = 0, 0

        def all_reduce_u32(self, a):
            self.reduces += 1; return np.asarray(a, np.uint32)

        def abort(self):
            self.aborts += 1

    def boom(*_):
        raise MemoryError("x")
    for kw in (dict(), dict(build_fn=boom, n_queries=3), dict(build_fn=lambda lo, hi: 1, n_queries=3)):
        c = Log()
        with pytest.raises(MemoryError):
            parallel.twoset_forward_target_sharded(boom, np.full(8, 100), c, t_ranks=T_RANKS, count_shared=True, **kw)
        assert c.reduces == 0 and c.aborts == 1, kw


def test_the_default_still_refuses():
    with pytest.raises(ValueError, match="Duplicate read identifier"):
        parallel.twoset_forward_target_sharded(lambda lo, hi: (np.zeros(3, np.uint32),) * 2, np.full(8, 100), World2(), t_ranks=T_RANKS)
    with pytest.raises(ValueError, match="Duplicate read identifier"):
        parallel.twoset_forward_target_sharded(lambda lo, hi: (np.zeros(3, np.uint32),) * 2, np.full(8, 100), World2(), t_ranks=T_RANKS, count_shared=False)
