"""GPU: forward two-set against a PARTITIONED index whose parts share target names.  The reference inserts target_name into a
HashSet per query (twoset.rs:286-317): a name is counted once however many reads bear it.  One index does that (k_count's t_dup
walk); the parts of a partitioned index each see only their own reads, so a group onto a read whose name also occurs in another
part leaves a (query, name) pair instead of a count, and the distinct pairs are counted behind the last part (k_count_shared,
k_name_pairs_count).  The parts must answer exactly as the single index and the oracle do, on three kinds of target sets:
  a  the set followed by a copy of its first third under the same names (a concatenated file: identical reads under one name)
  b  about one read in ten renamed to the name of a read at least half the set away (different reads under one name)
  c  names borne by three reads each that lie in three different parts at 7 parts, two of them in one part at 2 parts
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PRESETS = {"ont": 0, "pb": 1}
KINDS = ("a", "b", "c")
SEED_B = 2            # the renaming of set b (chosen on the CPU with the oracle: see test_the_sets_are_not_vacuous)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shared_names_plain_counters.json")


# ---- the target sets (numpy + the read batches of lrge_amd.synth only: tests/golden/make_shared_names_counters.py loads this file too) ----
def part_of(lens, part_bases):
    """index part of every read: index_build_parts cuts by reads, every part at most part_bases bases"""
    out, acc, p = np.zeros(len(lens), dtype=np.int64), 0, 0
    for r, l in enumerate(lens):
        if acc and acc + int(l) > part_bases:
            p, acc = p + 1, 0
        acc += int(l)
        out[r] = p
    return out


def part_bases_for(lens, n_parts):
    return int(np.sum(lens)) // n_parts + 1


def make_set(kind, q, t):
    """(seqs, names) of the target set of one kind, built from the read batch t (q: the queries, for kind c)"""
    seqs, names, n = t.seqs(), list(t.names), t.n
    if kind == "a":
        return seqs + seqs[:n // 3], names + names[:n // 3]
    if kind == "b":
        rng = np.random.Generator(np.random.PCG64(SEED_B))
        orig = list(names)
        for i in np.nonzero(rng.random(n) < 0.1)[0]:
            j = int(rng.integers(i + n // 2, n)) if i < n - n // 2 else int(rng.integers(0, i - n // 2 + 1))
            assert abs(j - int(i)) >= n // 2
            names[i] = orig[j]
        return seqs, names
    if kind == "c":
        # per query (by the truth of the sample) three targets that overlap it, in three different parts at 7 parts and two of them
        # in one part at 2 parts: one name for the three
        lens = t.lens()
        p7, p2 = part_of(lens, part_bases_for(lens, 7)), part_of(lens, part_bases_for(lens, 2))
        used, n_names = set(), 0
        for qi in range(q.n):
            ov = [i for i in range(n) if i not in used and min(int(q.ends[qi]), int(t.ends[i])) - max(int(q.starts[qi]), int(t.starts[i])) >= 3000]
            trip = next(((x, y, z) for x in ov for y in ov for z in ov
                         if x < y < z and len({p7[x], p7[y], p7[z]}) == 3 and len({p2[x], p2[y], p2[z]}) == 2), None)
            if trip is None:
                continue
            for i in trip[1:]:
                names[i] = names[trip[0]]
            used.update(trip)
            n_names += 1
        assert n_names >= 3, "set c: too few (query, three bearers) constellations in this sample"
        return seqs, names
    if kind == "distinct":
        return seqs, names
    if kind == "one-part":       # duplicates inside the first of 2 parts only
        p2 = part_of(t.lens(), part_bases_for(t.lens(), 2))
        first = np.nonzero(p2 == 0)[0]
        for i in first[3::7]:
            names[i] = names[first[1]]
        return seqs, names
    raise ValueError(kind)


def to_arrays(seqs):
    lens = np.array([len(s) for s in seqs], dtype=np.uint64)
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offs[1:])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), offs


def plain_cases(ctx, q, t, preset):
    """The calls of test_the_path_is_not_taken: {case: (counters, counts, counts of the single index)} -- also what
    tests/golden/make_shared_names_counters.py records on the commit before the feature."""
    from lrge_amd import engine
    out = {}
    for kind, n_parts in (("distinct", 2), ("distinct", 7), ("one-part", 2)):
        seqs, names = make_set(kind, q, t)
        qr, tr = engine.name_ranks(q.names, names)
        b, o = to_arrays(seqs)
        Qd, Td = ctx.upload(q.bases, q.offsets, qr), ctx.upload(b, o, tr)
        ctx.set_option("PART_BASES", None)
        ix = engine.Index(ctx, Td, preset)
        ref, _ = ix.overlap_twoset(Qd)
        ix.free()
        ctx.set_option("PART_BASES", str(part_bases_for(np.diff(o), n_parts)))
        try:
            ixp = engine.Index(ctx, Td, preset)
            counts, _ = ixp.overlap_twoset(Qd)
            out["%s/%d" % (kind, n_parts)] = (ctx.counters(), counts.copy(), ref.copy())
            ixp.free()
        finally:
            ctx.set_option("PART_BASES", None)
    return out


# ---- references: the single index (existing behaviour) and the oracle, once per (kind, preset) ----
_REF = {}


def _case(ctx, oracle, tiny_ont, tiny_hifi, kind, preset):
    from lrge_amd import engine
    key = (kind, preset)
    if key not in _REF:
        ds = tiny_ont if preset == "ont" else tiny_hifi
        seqs, names = make_set(kind, ds.q, ds.t)
        opt = oracle.make_opt(oracle.PRESET_AVA_PB if preset == "pb" else oracle.PRESET_AVA_ONT, dual=True)
        ixo = oracle.Index(oracle.ReadSet(seqs, names), opt)
        Qo = oracle.ReadSet(ds.q.seqs(), ds.q.names)
        exp = {}
        for F in (False, True):
            rc, ec, eh = ixo.twoset_counts(Qo, remove_internal=F, threads=8)
            assert rc == 0
            exp[F] = (ec.copy(), eh.copy())
        rc, dc, _ = oracle.Index(oracle.ReadSet(seqs, [b"uniq%06d" % i for i in range(len(names))]), opt).twoset_counts(Qo, threads=8)
        assert rc == 0
        _REF[key] = dict(ds=ds, seqs=seqs, names=names, oracle=exp, oracle_distinct=dc.copy(), lens=np.array([len(s) for s in seqs]))
    c = _REF[key]
    qr, tr = engine.name_ranks(c["ds"].q.names, c["names"])
    b, o = to_arrays(c["seqs"])
    Qd, Td = ctx.upload(c["ds"].q.bases, c["ds"].q.offsets, qr), ctx.upload(b, o, tr)
    if "single" not in c:
        ix = engine.Index(ctx, Td, PRESETS[preset])
        c["single"], c["anchors"] = {}, {}
        for F in (False, True):
            counts, has = ix.overlap_twoset(Qd, remove_internal=F)
            c["single"][F], c["anchors"][F] = (counts.copy(), has.copy()), ctx.counters()["anchors"]
            assert ctx.counters()["shared_name_pairs"] == 0 and ctx.counters()["shared_name_distinct"] == 0
        ix.free()
        # the two references agree with each other before anything is compared against them
        for F in (False, True):
            assert np.array_equal(c["single"][F][0], c["oracle"][F][0]) and np.array_equal(c["single"][F][1], c["oracle"][F][1]), (kind, preset, F)
    return c, Qd, Td


@pytest.mark.parametrize("preset", ["ont", "pb"])
@pytest.mark.parametrize("kind", KINDS)
def test_parts_count_a_shared_name_once(ctx, oracle, knobs, tiny_ont, tiny_hifi, kind, preset):
    """Exactness: counts and has_mapping of 2, 3, 7 and 25 parts equal the single index's and the oracle's, with and without -F, and
    the parts see the same anchors.  (Before the feature: LrgeHipError(ERR_DUPLICATE_ID) at the first call.)"""
    from lrge_amd import engine
    c, Qd, Td = _case(ctx, oracle, tiny_ont, tiny_hifi, kind, preset)
    for n_parts in (2, 3, 7, 25):
        knobs.set("PART_BASES", str(part_bases_for(c["lens"], n_parts)))
        ixp = engine.Index(ctx, Td, PRESETS[preset])
        for F in (False, True):
            counts, has = ixp.overlap_twoset(Qd, remove_internal=F)
            cn = ctx.counters()
            assert cn["index_parts"] >= n_parts
            assert np.array_equal(counts, c["single"][F][0]), (n_parts, F, np.nonzero(counts != c["single"][F][0])[0][:10])
            assert np.array_equal(has, c["single"][F][1]), (n_parts, F)
            assert cn["anchors"] == c["anchors"][F], (n_parts, F)
        ixp.free()


@pytest.mark.parametrize("preset", ["ont", "pb"])
@pytest.mark.parametrize("kind", KINDS)
def test_the_sets_are_not_vacuous(ctx, oracle, knobs, tiny_ont, tiny_hifi, kind, preset):
    """Every set makes the parts emit the same (query, name) pair more than once, and the shared names change the answer: some query
    counts fewer names than it would if every read had a name of its own."""
    from lrge_amd import engine
    c, Qd, Td = _case(ctx, oracle, tiny_ont, tiny_hifi, kind, preset)
    assert np.all(c["oracle"][False][0] <= c["oracle_distinct"]) and np.any(c["oracle"][False][0] < c["oracle_distinct"])
    for n_parts in (2, 7):
        knobs.set("PART_BASES", str(part_bases_for(c["lens"], n_parts)))
        ixp = engine.Index(ctx, Td, PRESETS[preset])
        counts, _ = ixp.overlap_twoset(Qd)
        cn = ctx.counters()
        ixp.free()
        print(kind, preset, n_parts, "pairs", cn["shared_name_pairs"], "distinct", cn["shared_name_distinct"])
        assert np.array_equal(counts, c["single"][False][0])
        assert cn["shared_name_pairs"] > cn["shared_name_distinct"] > 0, (kind, preset, n_parts, cn["shared_name_pairs"], cn["shared_name_distinct"])


@pytest.mark.parametrize("preset", ["ont", "pb"])
@pytest.mark.parametrize("kind", KINDS)
def test_views_times_parts(ctx, oracle, knobs, tiny_ont, tiny_hifi, kind, preset):
    """The pairs of a call accumulate over the parts AND the views of the queries (global query indices), in a buffer that is
    flushed (sort, unique, compact) and grown on the way: at least 3 views x 3 and 7 parts, with the default buffer and with one
    that starts at a handful of entries."""
    from lrge_amd import engine
    c, Qd, Td = _case(ctx, oracle, tiny_ont, tiny_hifi, kind, preset)
    qb = int(c["ds"].q.lens().sum())
    knobs.set("STREAM_BASES", str(qb // 3 + 1))
    seen = {}
    for n_parts in (3, 7):
        knobs.set("PART_BASES", str(part_bases_for(c["lens"], n_parts)))
        ixp = engine.Index(ctx, Td, PRESETS[preset])
        for cap in (None, 4):
            if cap:
                knobs.set("DEBUG_NAME_PAIRS_CAP", str(cap))
            for F in (False, True):
                counts, has = ixp.overlap_twoset(Qd, remove_internal=F)
                cn = ctx.counters()
                assert cn["lookup_launches"] >= 3 * n_parts                       # (views x parts)
                assert np.array_equal(counts, c["single"][F][0]) and np.array_equal(has, c["single"][F][1]), (n_parts, cap, F)
                # what was emitted and what is distinct do not depend on how the buffer was managed
                assert seen.setdefault((n_parts, F), (cn["shared_name_pairs"], cn["shared_name_distinct"])) == (cn["shared_name_pairs"], cn["shared_name_distinct"])
                assert F or cn["shared_name_pairs"] > cn["shared_name_distinct"] > 0
            knobs.unset("DEBUG_NAME_PAIRS_CAP")
        ixp.free()


@pytest.mark.parametrize("preset", ["ont", "pb"])
def test_the_path_is_not_taken(ctx, knobs, tiny_ont, tiny_hifi, preset):
    """An all-distinct set, and one whose only duplicates sit inside one of 2 parts, launch what they always did: both counters 0,
    the counts of the single index, and every other counter what the commit before the feature gave for the same call
    (tests/golden/shared_names_plain_counters.json, recorded there by tests/golden/make_shared_names_counters.py)."""
    ds = tiny_ont if preset == "ont" else tiny_hifi
    golden = json.load(open(GOLDEN))[preset]
    got = plain_cases(ctx, ds.q, ds.t, PRESETS[preset])
    assert set(got) == set(golden)
    for case, (cn, counts, ref) in got.items():
        assert cn["shared_name_pairs"] == 0 and cn["shared_name_distinct"] == 0, case
        assert np.array_equal(counts, ref), case
        both = [k for k in cn if k in golden[case]]
        assert len(both) >= 20
        assert {k: cn[k] for k in both} == {k: golden[case][k] for k in both}, case


def test_inverse_and_ava_still_refuse_duplicates(ctx, oracle, knobs, tiny_ont, tiny_hifi):
    from lrge_amd import engine, _ffi
    c, Qd, Td = _case(ctx, oracle, tiny_ont, tiny_hifi, "b", "ont")
    knobs.set("PART_BASES", str(part_bases_for(c["lens"], 3)))
    ixp = engine.Index(ctx, Td, PRESETS["ont"])
    for call in (lambda: ixp.overlap_inverse(Qd), lambda: ixp.overlap_ava()):
        with pytest.raises(_ffi.LrgeHipError) as ei:
            call()
        assert ei.value.code == _ffi.ERR_DUPLICATE_ID
    ixp.free()
