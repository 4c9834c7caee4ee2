"""GPU: the chaining and counting kernels on inputs that sit ON their limits (tests/chain_cases.py; tests/test_chain_cases.py
proves on the CPU that they do), in every kernel form, against the CPU oracle bit for bit.

The sampled reads of the other GPU tests put the anchors of an overlap on a near-constant diagonal: dd == bw, an empty stretch of
exactly max_gap, a chain of exactly min_chain_score, overhang / maplen == ratio and a pair kept on both strands then occur by
accident, if ever, and a kernel whose penalty table is one entry short, or that compares with < for <=, passes them."""
import numpy as np
import pytest

import chain_cases as CC
from conftest import to_arrays

pytestmark = pytest.mark.gpu

FIELDS = ["query", "target", "rev", "score", "cnt", "qs", "qe", "rs", "re", "mlen", "blen"]
MODES = [(False, 0.2), (True, 0.2), (True, 0.05)]         # (remove_internal, max_overhang_ratio)
FORMS = {                                                  # options of the context (lrge_hip_ctx_set_option), per kernel form
    "default": {},
    "hw": {"CHAIN": "hw"},
    "lpg": {"CHAIN": "lpg"},
    "lpg_notab": {"CHAIN": "lpg", "LPG_NOTAB": "1"},       # the f32 penalty per candidate instead of the table in LDS
    "lpg_no_prune": {"CHAIN": "lpg", "LPG_NO_PRUNE": "1"},
    "auto64": {"LPG_MAX": "64"},                           # groups above 64 anchors -> k_chain_hw, the rest -> k_chain_lpg
}


def _rows(rows):
    a = np.asarray(rows, dtype=np.int64).reshape(-1, len(FIELDS))
    return a[np.lexsort(a.T[::-1])]


class _Edges:
    """one preset: the case sets on the device with their three indexes, and what the oracle says of them (computed once)"""

    def __init__(self, ctx, O, preset):
        from lrge_amd import engine
        self.cases, qseqs, qnames, tseqs, tnames = CC.build(preset)
        n = self.n = len(self.cases)
        pid = 1 if preset == "pb" else 0
        opreset = O.PRESET_AVA_PB if preset == "pb" else O.PRESET_AVA_ONT
        # two sets
        qr, tr = engine.name_ranks(qnames, tnames)
        self.Qd, self.Td = ctx.upload(*to_arrays(qseqs), qr), ctx.upload(*to_arrays(tseqs), tr)
        self.ixT, self.ixQ = engine.Index(ctx, self.Td, pid), engine.Index(ctx, self.Qd, pid)
        opt = O.make_opt(opreset, dual=True)
        Qo, To = O.ReadSet(qseqs, qnames), O.ReadSet(tseqs, tnames)
        ixT, ixQ = O.Index(To, opt), O.Index(Qo, opt)
        self.chains = _rows([(q, r["rid"], r["rev"], r["score"], r["cnt"], r["qs"], r["qe"], r["rs"], r["re"], r["mlen"], r["blen"])
                             for q in range(n) for r in ixT.map(qseqs[q], qnames[q])])
        self.twoset, self.inv_q, self.inv_t = {}, {}, {}
        for mode in MODES:
            rc, c, h = ixT.twoset_counts(Qo, remove_internal=mode[0], ratio=mode[1])
            assert rc == 0
            self.twoset[mode] = (c, h)
            rc, self.inv_q[mode] = ixQ.inverse_counts(To, remove_internal=mode[0], ratio=mode[1])    # twoset.rs:596-599: the QUERY set indexed
            assert rc == 0
            rc, self.inv_t[mode] = ixT.inverse_counts(Qo, remove_internal=mode[0], ratio=mode[1])    # and the roles the other way round
            assert rc == 0
        # all-vs-all over the union, under fresh names in an order that is not the order of the reads (NO_DUAL works on names)
        perm = np.random.Generator(np.random.PCG64(5)).permutation(2 * n)
        useqs, unames = qseqs + tseqs, [b"u%05d" % v for v in perm]
        (ur,) = engine.name_ranks(unames)
        self.Ud = ctx.upload(*to_arrays(useqs), ur)
        self.ixU = engine.Index(ctx, self.Ud, pid)
        ixU = O.Index(O.ReadSet(useqs, unames), O.make_opt(opreset, dual=False))
        self.ava = {}
        for mode in MODES:
            rc, self.ava[mode] = ixU.ava_counts(remove_internal=mode[0], ratio=mode[1])
            assert rc == 0

    def label(self, read):
        """the case a read of the query set, of the target set or of their union belongs to"""
        return self.cases[int(read) % self.n].label

    def same(self, what, got, exp):
        bad = np.nonzero(np.asarray(got) != np.asarray(exp))[0]
        assert bad.size == 0, "%s differs in %d reads, first: %s" % (
            what, bad.size, ["%s (got %d, oracle %d)" % (self.label(b), got[b], exp[b]) for b in bad[:8]])

    def free(self):
        for o in (self.ixT, self.ixQ, self.ixU, self.Qd, self.Td, self.Ud):
            o.free()


@pytest.fixture(scope="module", params=["ont", "pb"])
def edges(ctx, oracle, request):
    e = _Edges(ctx, oracle, request.param)
    yield e
    e.free()


@pytest.mark.parametrize("form", list(FORMS))
def test_chain_edges(ctx, edges, knobs, form):
    for name, value in FORMS[form].items():
        knobs.set(name, value)
    e = edges
    # all eleven fields of every chain
    got = e.ixT.chains(e.Qd, dual=True)
    got = _rows(np.stack([got[f].astype(np.int64) for f in FIELDS], axis=1))
    exp = e.chains
    if got.shape != exp.shape or (got != exp).any():
        gs, es = {tuple(r) for r in got.tolist()}, {tuple(r) for r in exp.tolist()}
        only = sorted((r[0], "device only", r) for r in gs - es) + sorted((r[0], "oracle only", r) for r in es - gs)
        pytest.fail("%d chains against the oracle's %d; %s" % (len(got), len(exp), ["%s: %s %s" % (e.label(q), w, r) for q, w, r in sorted(only)[:8]]))
    for mode in MODES:
        tag = "remove_internal=%s ratio=%g" % mode
        c, h = e.ixT.overlap_twoset(e.Qd, remove_internal=mode[0], max_overhang_ratio=mode[1])
        e.same("two-set counts, " + tag, c, e.twoset[mode][0])
        e.same("two-set has_mapping, " + tag, h, e.twoset[mode][1])
        e.same("inverse counts (query set indexed), " + tag,
               e.ixQ.overlap_inverse(e.Td, remove_internal=mode[0], max_overhang_ratio=mode[1]), e.inv_q[mode])
        e.same("inverse counts (target set indexed), " + tag,
               e.ixT.overlap_inverse(e.Qd, remove_internal=mode[0], max_overhang_ratio=mode[1]), e.inv_t[mode])
        e.same("all-vs-all counts, " + tag, e.ixU.overlap_ava(remove_internal=mode[0], max_overhang_ratio=mode[1]), e.ava[mode])
    assert len(exp) > 1000 and e.twoset[MODES[0]][0].sum() > 1000
