"""The proof of tests/chain_cases.py: with the CPU oracle alone, every generated case sits on the edge it is named for.  These
are conditions, not measurements -- a case that misses its edge fails here, so that tests/test_gpu_chain_edges.py never
compares the kernels on inputs that decide nothing."""
import numpy as np
import pytest

import chain_cases as CC

PRESETS = ["ont", "pb"]


class _Proof:
    """one preset: the cases, the oracle index of the target set, and per case the anchors and chains on its own target"""

    def __init__(self, O, preset):
        self.O, self.preset, self.p = O, preset, CC.PRESETS[preset]
        self.cases, self.qseqs, self.qnames, self.tseqs, self.tnames = CC.build(preset)
        self.opt = O.make_opt(O.PRESET_AVA_PB if preset == "pb" else O.PRESET_AVA_ONT, dual=True)
        self.ix = O.Index(O.ReadSet(self.tseqs, self.tnames), self.opt)
        self._chains = {}

    def anchors(self, i):
        """(target last base, query last base, span) of case i's anchors on its own target and its own strand, by target
        position.  A reversed anchor carries its query position on the reverse strand: for an "/rc" twin that is the position
        in the read the twin was made from."""
        a = self.ix.anchors(self.qseqs[i], self.qnames[i])
        x, y = a["x"], a["y"]
        own = ((x >> np.uint64(32)) & np.uint64(0x7fffffff)) == np.uint64(i)
        own &= (x >> np.uint64(63)) == np.uint64(1 if self.cases[i].meta["rc"] else 0)
        x, y = x[own], y[own]
        return [(int(xx & np.uint64(0xffffffff)), int(yy & np.uint64(0xffffffff)), int(yy >> np.uint64(32)) & 0xff) for xx, yy in zip(x, y)]

    def chains(self, i, own=True, **loose):
        """case i's accepted chains (on its own target); loose: acceptance limits to apply instead of the preset's"""
        key = (i, own, tuple(sorted(loose.items())))
        if key not in self._chains:
            keep = {f: getattr(self.opt, f) for f in loose}
            for f, v in loose.items():
                setattr(self.opt, f, v)
            try:
                r = self.ix.map(self.qseqs[i], self.qnames[i])
            finally:
                for f, v in keep.items():
                    setattr(self.opt, f, v)
            self._chains[key] = r[r["rid"] == i] if own else r
        return self._chains[key]

    def orig_q(self, i, r):
        """(qs, qe) of chain r in the coordinates of the read an "/rc" twin was made from"""
        qlen = len(self.qseqs[i])
        return (qlen - int(r["qe"]), qlen - int(r["qs"])) if self.cases[i].meta["rc"] else (int(r["qs"]), int(r["qe"]))

    def of(self, family):
        return [(i, c) for i, c in enumerate(self.cases) if c.family == family]


@pytest.fixture(scope="module", params=PRESETS)
def proof(oracle, request):
    return _Proof(oracle, request.param)


def test_sets_are_well_formed(proof):
    n = len(proof.cases)
    assert proof.qnames == [b"q%04d" % i for i in range(n)] and proof.tnames == [b"t%04d" % i for i in range(n)]
    assert len(set(proof.qnames) | set(proof.tnames)) == 2 * n            # distinct names, hence distinct ranks
    assert len({c.label for c in proof.cases}) == n
    assert {c.family for c in proof.cases} == {"band", "gap", "threshold", "overhang", "both"}
    for fam in ("band", "gap", "threshold", "overhang", "both"):
        assert any(c.meta["rc"] for _, c in proof.of(fam)) and any(not c.meta["rc"] for _, c in proof.of(fam))
    assert all(set(s) <= set(b"ACGT") for s in proof.qseqs + proof.tseqs)
    # a pair is 20 kb at most.  The overhang sweeps (6 kb + 2.4 kb for each of 2 ratios x 2 sides x 81 offsets, and mirrored) are
    # 5.4 Mbases of a set as listed, 6.3 with their twins; the other families together are about 1.5 Mbases
    sizes = {fam: sum(len(c.q) + len(c.t) for _, c in proof.of(fam)) for fam in ("band", "gap", "threshold", "overhang", "both")}
    print("%s: %d cases, bases %s" % (proof.preset, n, sizes))
    assert max(len(c.q) + len(c.t) for c in proof.cases) < 22000
    assert sum(sizes.values()) - sizes["overhang"] < 1_600_000 and sizes["overhang"] < 6_500_000


def test_band_cases_sit_on_the_band_limit(proof):
    """The two flanks differ in diagonal by exactly D, and the oracle chains them into one iff D <= bw.  In the "short" variants, and in
    "mid" for ava-ont, the flank behind the junction scores less than the gap costs at dd = bw (0.12 * 2000 + 5 = 245 for ava-ont,
    0.152 * 500 + 4 = 80 for ava-pb), so the backtrack cuts the chain at the junction whether the DP linked it or not: they reach the
    limit inside the DP only, and what is asserted of their chains is that none spans the junction above bw.  The "decoys" variants are the ones whose first anchor behind the junction finds its predecessor far back in the window."""
    bw = proof.p["bw"]
    seen = set()
    for i, c in proof.of("band"):
        m = c.meta
        D, J = m["D"], m["junction"]
        an = proof.anchors(i)
        assert an, c.label
        shift = D if m["form"] == "ins" else 0                        # query bases between A and B
        sign = 1 if m["form"] == "del" else -1                        # dr - dq across the junction
        decoys = [(x, y) for x, y, _ in an if m["variant"] == "decoys" and J <= x < J + D]
        rest = [(x, y) for x, y, _ in an if (x, y) not in decoys]
        before = [(x, y) for x, y in rest if y < J]
        behind = [(x, y) for x, y in rest if y >= J + shift]
        assert len(before) + len(behind) == len(rest), "%s: an anchor inside the inserted block" % c.label
        assert {x - y for x, y in before} == {0}, c.label
        assert {x - y for x, y in behind} == {sign * D}, c.label       # the diagonals differ by exactly D
        assert len(before) > 64 or m["variant"] == "weak", c.label
        if m["variant"] == "weak":
            assert 3 <= len(before) <= 32 and 3 <= len(behind) <= 32, c.label
        elif m["variant"] == "short":
            assert 3 <= len(behind) < 8, (c.label, len(behind))
        elif m["variant"] == "mid":
            assert 8 <= len(behind) <= 32, (c.label, len(behind))
        else:
            assert len(behind) > 64, c.label
        # in target order the decoys stand between the flanks, and none of them can precede an anchor of B in the query
        assert m["decoys"][0] <= len(decoys) + (m["variant"] != "decoys") <= m["decoys"][1] + 1, (c.label, len(decoys))
        assert all(y > behind[0][1] for _, y in decoys) and len({x - y for x, y in decoys}) <= 1
        ch = [r for r in proof.chains(i) if not (decoys and J <= r["rs"] and r["re"] <= J + D)]
        spans = [r for r in ch if proof.orig_q(i, r)[0] < J and proof.orig_q(i, r)[1] > J + shift]
        if m["variant"] == "weak":                                    # ONE chain, or NONE: the limit decides a count
            assert len(proof.chains(i, own=False)) == len(ch) == (1 if D <= bw else 0), "%s: %d chains" % (c.label, len(ch))
            both = proof.chains(i, min_chain_score=50)                 # the flanks the preset rejects at bw + 1: 92 .. 99 each
            assert D <= bw or (len(both) == 2 and all(92 <= r["score"] <= 99 for r in both)), c.label
        elif m["variant"] in ("short", "mid"):
            assert len(ch) >= 1 and ch[0]["cnt"] >= len(before) and (D <= bw or not spans), c.label
        elif D <= bw:
            assert len(ch) == 1 and len(spans) == 1, "%s: %d chains" % (c.label, len(ch))
            qs, qe = proof.orig_q(i, ch[0])                           # both flanks from end to end, across the junction
            assert qs <= before[0][1] and qe == behind[-1][1] + 1 and ch[0]["cnt"] > len(rest) - 8, c.label
        else:
            assert len(ch) == 2 and not spans, "%s: %d chains" % (c.label, len(ch))
        seen.add((m["form"], D, m["variant"], m["decoys"], m["rc"]))
    assert len(seen) == ((6 + 4) * 2 + 2 * 3 + (4 if proof.p["hpc"] else 0)) * 2
    assert {D for _, D, _, _, _ in seen} == {1, 2, bw - 1, bw, bw + 1, bw + 2}


def test_gap_cases_sit_on_the_reach_limit(proof):
    seen = set()
    for i, c in proof.of("gap"):
        m = c.meta
        an = proof.anchors(i)
        left = max(k for k, (x, y, _) in enumerate(an) if y < m["junction"])
        (x0, y0, _), (x1, y1, _) = an[left], an[left + 1]              # adjacent in target order: nothing between them
        assert (y1 - y0, x1 - x0) == (m["dq"], m["dr"]), (c.label, y1 - y0, x1 - x0)
        assert max(m["dq"], m["dr"]) == m["gap"] and abs(m["dq"] - m["dr"]) in (0, 2)
        assert all(b[1] > a[1] for a, b in zip(an, an[1:])), c.label   # and in query order
        ch = proof.chains(i)
        if m["weak"]:                                                  # ONE chain, or NONE: the limit decides a count
            assert len(proof.chains(i, own=False)) == len(ch) == (1 if m["gap"] <= CC.MAX_GAP else 0), "%s: %d chains" % (c.label, len(ch))
            both = proof.chains(i, min_chain_score=50)                 # the flanks the preset rejects at 5001: 60 .. 99 each
            assert m["gap"] <= CC.MAX_GAP or (len(both) == 2 and all(60 <= r["score"] <= 99 for r in both)), c.label
            seen.add((c.label.split("/")[0], m["gap"], m["rc"], True))
            continue
        assert len(ch) == (1 if m["gap"] <= CC.MAX_GAP else 2), "%s: %d chains" % (c.label, len(ch))
        if m["gap"] <= CC.MAX_GAP:
            qs, qe = proof.orig_q(i, ch[0])                            # both flanks from end to end
            assert qs <= an[0][1] and qe == an[-1][1] + 1 and ch[0]["cnt"] > len(an) - 8, c.label
        seen.add((c.label.split("/")[0], m["gap"], m["rc"], False))
    assert seen == {(k, g, rc, weak) for k in ("gap", "gapq", "gapr") for g in (4999, 5000, 5001) for rc in (False, True)
                    for weak in (False, True) if not (weak and g == 4999)}


def test_threshold_cases_cross_the_acceptance_limits(proof):
    th = proof.of("threshold")
    assert sorted({c.meta["L"] for _, c in th if c.meta["rep"] == ""}) == list(range(60, 261))
    for rc in (False, True):
        plain = [(i, c) for i, c in th if c.meta["rc"] == rc and c.meta["rep"] != "runs"]
        acc = {c.meta["L"]: len(proof.chains(i)) for i, c in plain}
        assert set(acc.values()) == {0, 1}
        rejected, accepted = [L for L, n in acc.items() if not n], [L for L, n in acc.items() if n]
        assert min(rejected) == 60 and max(accepted) == 260
        assert max(rejected) > min(accepted) - 40                      # one crossing region, both outcomes on either side of it
        assert any(acc[L] == 0 and acc[L + 1] == 1 for L in range(60, 260))
        # scores next to min_chain_score = 100: what the DP gave a chain the preset then rejected
        near_miss = [i for i, c in plain if not len(proof.chains(i)) and
                     any(90 <= r["score"] <= 99 for r in proof.chains(i, min_chain_score=90))]
        near_hit = [i for i, c in plain if any(100 <= r["score"] <= 110 for r in proof.chains(i))]
        assert near_miss and near_hit
        assert any(r["score"] == 100 for i in near_hit for r in proof.chains(i)), "no chain accepted at exactly min_chain_score"
        assert any(r["score"] == 99 for i in near_miss for r in proof.chains(i, min_chain_score=90)), "no chain rejected one below"
    cnts = [int(r["cnt"]) for i, c in th for r in proof.chains(i)]
    if proof.preset == "pb":
        # min_cnt = 3 decides only where two anchors reach score 100: HPC k-mers over long runs (thrun)
        assert 3 in cnts, "no accepted chain of exactly min_cnt anchors"
        two = [i for i, c in th if not len(proof.chains(i)) and
               any(r["cnt"] == 2 and r["score"] >= 100 for r in proof.chains(i, min_cnt=1))]
        assert two, "no chain of two anchors with an accepted score"
    else:
        # k = 15 without HPC: an anchor adds at most its span, 15, so score 100 needs 7 anchors and min_cnt never decides
        assert min(cnts) >= 7


def _overhang_maplen(qlen, qs, qe, rev, tlen, ts, te):     # mapping.rs:59-74
    if not rev:
        ov = min(qs, ts) + min(qlen - qe, tlen - te)
    else:
        ov = min(qs, tlen - te) + min(qlen - qe, ts)
    return ov, max(qe - qs, te - ts)


def test_overhang_cases_sit_on_the_predicates(proof):
    O = proof.O
    hits = {}
    for i, c in proof.of("overhang"):
        m = c.meta
        ch = proof.chains(i)
        assert len(ch) == 1, "%s: %d chains" % (c.label, len(ch))
        r = ch[0]
        args = (len(proof.qseqs[i]), int(r["qs"]), int(r["qe"]), int(r["rev"]), len(proof.tseqs[i]), int(r["rs"]), int(r["re"]))
        ov, maplen = _overhang_maplen(*args)
        assert (ov, maplen) == (m["overhang"], m["maplen"]), (c.label, ov, maplen, m)    # the generator's arithmetic is the oracle's
        per = int(round(1 / m["ratio"]))
        if maplen % per:
            continue
        d = ov - maplen // per
        if abs(d) > 1:
            continue
        # forward predicate: overhang / maplen < ratio in f32, equality is not below; inverse: overhang > (i32)(maplen * ratio)
        assert O.is_internal(*args, m["ratio"]) == (d < 0), c.label
        assert O.inverse_skip(*args, m["ratio"]) == (d > 0), c.label
        assert int(np.float32(maplen) * np.float32(m["ratio"])) == maplen // per
        hits.setdefault((m["mirrored"], m["ratio"], m["rc"], m["side"]), set()).add(d)
    for mirrored in (False, True):
        for ratio in CC.RATIOS:
            for rc in (False, True):
                got = hits.get((mirrored, ratio, rc, 1), set()) | hits.get((mirrored, ratio, rc, 2), set())
                assert got == {-1, 0, 1}, "mirrored=%s ratio=%g rc=%s: only %s" % (mirrored, ratio, rc, sorted(got))
            for side in (1, 2):
                assert 0 in hits.get((mirrored, ratio, False, side), set()) | hits.get((mirrored, ratio, True, side), set())
    sweep = {(c.meta["mirrored"], c.meta["ratio"], c.meta["side"], c.meta["v"]) for _, c in proof.of("overhang") if not c.meta["rc"]}
    assert len(sweep) == 2 * 2 * 2 * (2 * CC.SWEEP + 1)


def test_both_strand_cases_keep_one_pair_on_both_strands(proof):
    O = proof.O
    idx = [i for i, _ in proof.of("both")]
    Qo = O.ReadSet([proof.qseqs[i] for i in idx], [proof.qnames[i] for i in idx])
    counts = {}
    for rem, ratio in ((False, 0.2), (True, 0.2), (True, 0.05)):
        rc, cnt, has = proof.ix.twoset_counts(Qo, remove_internal=rem, ratio=ratio, threads=2)
        assert rc == 0 and has.all()
        counts[(rem, ratio)] = cnt
    for k, i in enumerate(idx):
        c = proof.cases[i]
        ch = proof.chains(i)
        assert sorted(int(r["rev"]) for r in ch) == [0, 1], "%s: strands %s" % (c.label, [int(r["rev"]) for r in ch])
        assert len(proof.chains(i, own=False)) == 2, c.label                      # and no other target
        internal = {}
        for r in ch:
            args = (len(proof.qseqs[i]), int(r["qs"]), int(r["qe"]), int(r["rev"]), len(proof.tseqs[i]), int(r["rs"]), int(r["re"]))
            internal[int(r["rev"])] = (O.is_internal(*args, 0.2), O.is_internal(*args, 0.05))
        part = c.label.split("/")[1] if c.label.count("/") and not c.label.startswith("both/rc") else "none"
        fwd_part_strand = 1 if c.meta["rc"] else 0                                 # the strand the g[a:b] part maps on
        want = {"none": (False, False), "fwd-int": (True, False), "rev-int": (False, True)}[part]
        assert (internal[fwd_part_strand][0], internal[1 - fwd_part_strand][0]) == want, (c.label, internal)
        assert internal[0][1] is False and internal[1][1] is False, c.label
        for key in counts:
            assert counts[key][k] == 1, (c.label, key, counts[key][k])             # two kept groups, one pair
    assert len(idx) == 6
