"""Read pairs that put the chaining and counting kernels (k_chain_lpg.h, k_chain_hw.h, k_chain_common.h, k_chain.h) on their
compare-against-a-limit edges on purpose: the band limit (dd against bw), the reach limit (dq / dr against max_gap), the
acceptance limits (min_cnt, min_chain_score), the -F predicates at equality, and one (query, target) pair kept on both
strands.  Sampled reads carry per-base noise only and decide an outcome at one of these edges by accident, if ever.

Plain Python + numpy, no GPU and no oracle.  Every case is a (query, target) pair of reads cut from its own random 4-letter
genome, so cases do not interact; build(preset) returns them all as one query set (names q%04d) and one target set (t%04d).
Where a case needs a minimizer position (the anchor gap of the gap family, the chain ends of the overhang family, the score of
a weak flank) the module finds it with its own restatement of the minimizer rule (minimizers() below: mm2:sketch.c without its
tie handling, enough for random sequence); tests/test_chain_cases.py proves with the oracle that every case sits where its
label says.  A set is 7.7 Mbases: 6.3 of them the overhang sweeps (648 pairs of 6 kb + 2.4 kb, and the twins near the centres), about
1.5 all other families together.  On an MI355X every kernel form takes under a second on a set.

Families (each for both presets; each built a second time, from other draws, with the query reverse-complemented: label "/rc"):
  band       query A + B against target A + X + B, |X| = D ("del": dr - dq = D), and mirrored ("ins": dq - dr = D);
             D in 1, 2, bw - 1, bw, bw + 1, bw + 2.  Variants at D = bw and bw + 1:
             "short" / "mid": the flank behind the junction (B) holds fewer than 8 / between 8 and 32 anchors;
             "decoys=8 / 33 / 65": that many anchors and more stand between the flanks in target order without being candidates,
             so the first anchor of B finds A behind the first block of the k_chain_lpg window / outside that window / outside
             the 64 anchors k_chain_hw holds as well (chain_slow_tail);
             "weak" (ava-pb): two flanks that are accepted only as ONE chain -- the band limit decides a count.
  gap        shared flanks A and B around unrelated fillers, so that the last anchor of A and the first of B are exactly 4999,
             5000 and 5001 apart with nothing between them: "gap" on both axes (dd = 0), "gapq" / "gapr" on the query / target
             axis alone (the other axis 2 shorter), which tells (u32)(dq - 1) < dqlim from (u32)(dr - 1) < maxdx.
             "weak": flanks that are accepted only as ONE chain -- the reach limit decides a count.
  threshold  pairs sharing exactly L bases, L = 60 .. 260, inside unrelated reads, and five more draws of L = 95 .. 125: chains
             around min_chain_score 100.  "thrun" (ava-pb): the shared bases are homopolymer runs of 1 .. 8, whose HPC k-mers span
             several times k, so that chains of two and three anchors reach score 100 and min_cnt 3 decides (without HPC three
             anchors of span 15 score 45 at most: min_cnt never decides for ava-ont).
  overhang   target = a 6 kb stretch, query = junk[:o1] + 2 kb of it + junk[:o2]; o1 (o2 = 0) and o2 (o1 = 0) sweep +-40 around
             ratio * 2000 for ratio 0.2 and 0.05; "ovm": the same with the roles mirrored.  A few bases inserted into the middle of
             the 2 kb (meta "ins") bring maplen to 5 (20) times the overhang, the overhang less one and plus one, in the cases
             near the centre of a sweep: overhang / maplen == ratio exactly, and overhang == (i32)(maplen * ratio).
  both       query = g[a:b] + revcomp(g[c:d]): accepted chains on both strands of one pair; "both/fwd-int" / "both/rev-int":
             one of the two is internal under -F 0.2 (mapping.rs:59-77: overhang / maplen < ratio) and the other is not.
"""
import functools

import numpy as np

PRESETS = {"ont": dict(k=15, w=5, hpc=False, bw=2000), "pb": dict(k=19, w=5, hpc=True, bw=500)}
MAX_GAP = 5000
RATIOS = (0.2, 0.05)
CORE = 2000          # overhang family: bases of the target the query repeats
SWEEP = 40

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_CODE = np.zeros(256, dtype=np.uint64)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b


def revcomp(s):
    return _COMP[np.asarray(s)[::-1]]


class Case:
    def __init__(self, label, family, q, t, **meta):
        self.label, self.family, self.meta = label, family, meta
        self.q, self.t = np.asarray(q, dtype=np.uint8).tobytes(), np.asarray(t, dtype=np.uint8).tobytes()


# ------------------------------------------------------------------------------------------
# the minimizer rule, vectorised (mm2:sketch.c:mm_sketch for A/C/G/T only; equal hashes inside one window are not handled)
# ------------------------------------------------------------------------------------------
def _hash64(key, mask):
    key = (~key + (key << np.uint64(21))) & mask
    key = key ^ key >> np.uint64(24)
    key = ((key + (key << np.uint64(3))) + (key << np.uint64(8))) & mask
    key = key ^ key >> np.uint64(14)
    key = ((key + (key << np.uint64(2))) + (key << np.uint64(4))) & mask
    key = key ^ key >> np.uint64(28)
    key = (key + (key << np.uint64(31))) & mask
    return key


def minimizers(seq, k, w, hpc):
    """(hash, last base, span, strand) of the minimizers of seq, ascending by position"""
    seq = np.asarray(seq, dtype=np.uint8)
    c = _CODE[seq]
    n = len(c)
    if hpc:
        first = np.flatnonzero(np.concatenate(([True], c[1:] != c[:-1])))
        last = np.concatenate((first[1:], [n])) - 1
        c = c[first]
    else:
        first = last = np.arange(n)
    m = len(c) - k + 1
    if m < w:
        z = np.zeros(0, dtype=np.int64)
        return z.astype(np.uint64), z, z, z
    kf = np.zeros(m, dtype=np.uint64)
    kr = np.zeros(m, dtype=np.uint64)
    for j in range(k):
        kf = kf << np.uint64(2) | c[j:j + m]
        kr = kr | (np.uint64(3) - c[j:j + m]) << np.uint64(2 * j)
    strand = (kf > kr).astype(np.int64)
    h = _hash64(np.minimum(kf, kr), np.uint64((1 << 2 * k) - 1))
    span = last[k - 1:] + 1 - first[:m]
    x = h << np.uint64(8) | span.astype(np.uint64)
    win = np.lib.stride_tricks.sliding_window_view(x, w)
    pick = np.unique(np.arange(m - w + 1) + (w - 1 - np.argmin(win[:, ::-1], axis=1)))   # right-most smallest of each window
    pick = pick[span[pick] < 256]
    return h[pick], last[k - 1:][pick].astype(np.int64), span[pick].astype(np.int64), strand[pick]


def pair_anchors(q, t, p):
    """same-strand anchors of query q on target t as (target last base, query last base, span), ascending by target position"""
    hq, pq, sq, zq = minimizers(q, p["k"], p["w"], p["hpc"])
    ht, pt, st, zt = minimizers(t, p["k"], p["w"], p["hpc"])
    order = np.argsort(ht, kind="stable")
    hts = ht[order]
    lo, hi = np.searchsorted(hts, hq, "left"), np.searchsorted(hts, hq, "right")
    out = []
    for i in np.flatnonzero(hi > lo):
        for j in order[lo[i]:hi[i]]:
            if zq[i] == zt[j]:
                out.append((int(pt[j]), int(pq[i]), int(sq[i])))
    return sorted(out)


# ------------------------------------------------------------------------------------------
# families
# ------------------------------------------------------------------------------------------
def _rand(rng, n):
    return _ACGT[rng.integers(0, 4, size=int(n), dtype=np.uint8)]


def _other(rng, *forbidden):
    """a random letter that is none of `forbidden` (at most three)"""
    ok = [c for c in _ACGT if c not in forbidden]
    return ok[int(rng.integers(0, len(ok)))]


def _unlike(rng, n, first=(), last=()):
    """n random bases that begin with none of `first` and end with none of `last`.  At a junction the two reads of a pair must
    differ in their first base (else what they share grows by the bases that agree by chance), and neither may continue the
    homopolymer run of the shared side (else HPC moves the k-mers next to it)."""
    s = _rand(rng, n)
    if n == 1:
        s[0] = _other(rng, *first, *last)
    elif n:
        s[0], s[-1] = _other(rng, *first), _other(rng, *last)
    return s


def _diagonals(q, t, p):
    return {x - y for x, y, _ in pair_anchors(q, t, p)}


def _flank_score(an):
    """what the DP gives a flank chained alone: anchors (target, query, span) on one diagonal, each linked to the one before it
    (mm2:lchain.c:comput_sc with dd = 0: the smaller of the predecessor's span and the distance)"""
    an = sorted(an, key=lambda a: a[1])
    return an[0][2] + sum(min(a[2], b[1] - a[1]) for a, b in zip(an, an[1:])) if an else 0


def _weak(rng):
    return int(rng.integers(70, 116))


def _flank(rng):
    return int(rng.integers(1500, 2501))


def _band(p, rng, add):
    bw = p["bw"]
    per = 3 if not p["hpc"] else 5      # bases per anchor, about: one minimizer per (w + 1) / 2 = 3 positions; a pb position is a run of 4 / 3 bases
    shortB = {"short": 30 if not p["hpc"] else 42, "mid": 75 if not p["hpc"] else 100}
    todo = [(D, None) for D in (1, 2, bw - 1, bw, bw + 1, bw + 2)] + [(D, v) for v in ("short", "mid") for D in (bw, bw + 1)]
    for D, variant in todo:
        for form in ("del", "ins"):
            while True:
                a = _rand(rng, _flank(rng))
                b = _unlike(rng, shortB[variant] if variant else _flank(rng), first=(a[-1],))
                x = _unlike(rng, D, first=(a[-1], b[0]), last=(a[-1], b[0]))
                plain, longer = np.concatenate((a, b)), np.concatenate((a, x, b))
                q, t = (plain, longer) if form == "del" else (longer, plain)
                diag = [x - y for x, y, _ in pair_anchors(q, t, p)]
                behind = diag.count(D if form == "del" else -D)
                if set(diag) <= {0, D if form == "del" else -D} and (      # (else: a k-mer of X recurs by chance; draw again)
                        3 <= behind < 8 if variant == "short" else 8 <= behind <= 32 if variant == "mid" else True):
                    break
            add("band/%s/D=%d%s" % (form, D, "/" + variant if variant else ""), "band", q, t,
                D=D, form=form, variant=variant, junction=len(a), bw=bw, decoys=(0, 0))
    # weak (ava-pb only): either flank alone scores 92 .. 99, below min_chain_score = 100, and the two together pay the 80 that dd = bw
    # costs: ONE chain is accepted at D = bw and NONE at bw + 1, so the band limit decides a COUNT (count-only runs go through
    # k_chain_lpg and see no chain records).  ava-ont cannot: its gap costs 245, more than two rejected flanks can bring.
    for D in ((bw, bw + 1) if p["hpc"] else ()):
        for form in ("del", "ins"):
            while True:
                a = _rand(rng, _weak(rng))
                b = _unlike(rng, _weak(rng), first=(a[-1],))
                x = _unlike(rng, D, first=(a[-1], b[0]), last=(a[-1], b[0]))
                plain, longer = np.concatenate((a, b)), np.concatenate((a, x, b))
                q, t = (plain, longer) if form == "del" else (longer, plain)
                an = pair_anchors(q, t, p)
                sa, sb = _flank_score([v for v in an if v[0] - v[1] == 0]), _flank_score([v for v in an if v[0] - v[1] != 0])
                if {v[0] - v[1] for v in an} == {0, D if form == "del" else -D} and 92 <= sa <= 99 and 92 <= sb <= 99:
                    break
            add("band/%s/D=%d/weak" % (form, D), "band", q, t, D=D, form=form, variant="weak", junction=len(a), bw=bw, decoys=(0, 0))
    # decoys: the end of X repeats n bases from the far end of B.  Their anchors sort between the last anchor of A and the first of B
    # (by target position) and are no predecessors of B's anchors (they lie behind them in the query), so the first anchor of B
    # meets its only cross-junction candidate 8 .. 32 candidates back (behind the first block of the k_chain_lpg window), 33 .. 64
    # back (outside that window, inside the 64 anchors k_chain_hw holds) or further (outside both: chain_slow_tail).
    for D in (bw, bw + 1):
        for lo, hi, n in ((8, 32, 15 * per), (33, 64, 47 * per), (65, 1000, 100 * per)):
            n = min(n, bw - 60)                                   # (X keeps a head of its own)
            while True:
                a = _rand(rng, _flank(rng))
                b = _unlike(rng, 2 * bw + 100 + n + int(rng.integers(0, 400)), first=(a[-1],))   # long enough for |D - e| > bw below
                e = max(i for i in range(len(b) - 40, len(b)) if b[i - 1] not in (a[-1], b[0]) and b[i] != b[0])   # the copy ends where B goes on differently
                x = np.concatenate((_unlike(rng, D - n, first=(a[-1], b[0]), last=(b[e - n - 1],)), b[e - n:e]))
                q, t = np.concatenate((a, b)), np.concatenate((a, x, b))
                # the decoys lie on the diagonal D - e: out of band of both flanks, they chain with neither
                diag = [x_ - y_ for x_, y_, _ in pair_anchors(q, t, p)]
                if set(diag) <= {0, D, D - e} and lo <= diag.count(D - e) <= hi and e - D > bw + 64:
                    break
            add("band/del/D=%d/decoys=%d" % (D, lo), "band", q, t,
                D=D, form="del", variant="decoys", junction=len(a), bw=bw, decoys=(lo, hi))


def _gap(p, rng, add):
    for want in (MAX_GAP - 1, MAX_GAP, MAX_GAP + 1):
        for kind, skew_q, skew_t in (("gap", 0, 0), ("gapq", 0, 2), ("gapr", 2, 0)):
            while True:
                q, t, junction = _gap_pair(p, rng, want, skew_q, skew_t)
                if _diagonals(q, t, p) <= {0, skew_q - skew_t}:                  # (else: the fillers share a k-mer by chance; draw again)
                    break
            add("%s/%d" % (kind, want), "gap", q, t, gap=want, dq=want - skew_q, dr=want - skew_t, junction=junction, weak=False)
    # weak: either flank alone scores 60 .. 99, below min_chain_score = 100, and the gap costs nothing (dd = 0) or 1 (dd = 2): ONE chain
    # is accepted at 5000 and NONE at 5001, so the reach limit decides a COUNT (count-only runs go through k_chain_lpg)
    for want in (MAX_GAP, MAX_GAP + 1):
        for kind, skew_q, skew_t in (("gap", 0, 0), ("gapq", 0, 2), ("gapr", 2, 0)):
            while True:
                q, t, junction = _gap_pair(p, rng, want, skew_q, skew_t, _weak)
                an = pair_anchors(q, t, p)
                sa, sb = _flank_score([v for v in an if v[1] < junction]), _flank_score([v for v in an if v[1] >= junction])
                if {v[0] - v[1] for v in an} <= {0, skew_q - skew_t} and 60 <= sa <= 99 and 60 <= sb <= 99:
                    break
            add("%s/%d/weak" % (kind, want), "gap", q, t, gap=want, dq=want - skew_q, dr=want - skew_t, junction=junction, weak=True)


def _gap_pair(p, rng, want, skew_q, skew_t, flank=_flank):
    a, b = _rand(rng, flank(rng)), _rand(rng, flank(rng))
    # first and last 40 bases of the two fillers: fixed while G varies, so the minimizers of the flanks stay where they are
    hq = _unlike(rng, 40, first=(a[-1],))
    ht = _unlike(rng, 40, first=(a[-1], hq[0]))
    tq = _unlike(rng, 40, last=(b[0],))
    tt = _unlike(rng, 40, last=(b[0], tq[-1]))
    mids = [_rand(rng, MAX_GAP + 200) for _ in range(2)]

    def flank_gap(G):
        fq = np.concatenate((hq, mids[0][:G - skew_q - 80], tq))
        ft = np.concatenate((ht, mids[1][:G - skew_t - 80], tt))
        q, t = np.concatenate((a, fq, b)), np.concatenate((a, ft, b))
        an = [(x, y) for x, y, _ in pair_anchors(q, t, p) if x - y in (0, skew_q - skew_t)]
        left = max(y for x, y in an if y < len(a))
        right = min(y for x, y in an if y >= len(a) + G - skew_q)
        return right - left, q, t

    G = MAX_GAP - 100
    G += want - (flank_gap(G)[0] + skew_q)             # the longer axis gets `want`
    got, q, t = flank_gap(G)
    assert got + skew_q == want, (want, skew_q, skew_t, got)
    return q, t, len(a)


def _shared(rng, s):
    """two unrelated reads that share exactly the bases s"""
    qa = _unlike(rng, 80, last=(s[0],))
    ta = _unlike(rng, 80, last=(s[0], qa[-1]))
    qb = _unlike(rng, 80, first=(s[-1],))
    tb = _unlike(rng, 80, first=(s[-1], qb[0]))
    return np.concatenate((qa, s, qb)), np.concatenate((ta, s, tb))


def _threshold(p, rng, add):
    # L = 60 .. 260 once; five more draws of every L whose chain can score about 100 (score = L less the end effects of the windows)
    for rep, Ls in [("", range(60, 261))] + [("/%d" % r, range(95, 126)) for r in range(1, 6)]:
        for L in Ls:
            q, t = _shared(rng, _rand(rng, L))
            add("threshold/L=%d%s" % (L, rep), "threshold", q, t, L=L, rep=rep)
    if p["hpc"]:
        for L in range(60, 261):
            letters = _rand(rng, L)
            letters = letters[np.concatenate(([True], letters[1:] != letters[:-1]))]
            q, t = _shared(rng, np.repeat(letters, rng.integers(1, 9, size=len(letters)))[:L])
            add("thrun/L=%d" % L, "threshold", q, t, L=L, rep="runs")


def _overhang(p, rng, add):
    c0 = 2000
    for mirrored in (False, True):
        for ratio in RATIOS:
            centre = int(round(ratio * CORE))
            per = int(round(1 / ratio))
            for side in (1, 2):
                for v in range(-SWEEP, SWEEP + 1):
                    o1, o2 = (centre + v, 0) if side == 1 else (0, centre + v)
                    g, junk = _rand(rng, 6000), _rand(rng, centre + SWEEP)
                    g[c0 - 1], g[c0 + CORE] = _other(rng, g[c0]), _other(rng, g[c0 + CORE - 1])   # no run of the target crosses an end of the core
                    core = g[c0:c0 + CORE]
                    left, right = junk[:o1].copy(), junk[:o2].copy()
                    if o1:
                        left[-1] = _other(rng, core[0], g[c0 - 1])
                    if o2:
                        right[0] = _other(rng, core[-1], g[c0 + CORE])
                    short = np.concatenate((left, core, right))
                    # chain ends inside the core: first and last anchor on the diagonal (end effects of the minimizer windows)
                    an = [(x, y, s) for x, y, s in pair_anchors(short, g[c0 - 100:c0 + CORE + 100], p) if (x + c0 - 100) - y == c0 - o1]
                    first, last = an[0], an[-1]
                    maplen = last[1] + 1 - (first[1] + 1 - first[2])
                    overhang = o1 + o2 + CORE - maplen
                    # maplen = max(query extent, target extent): bases inserted into the middle of the short read lengthen it alone.
                    # Near the centre of the sweep that brings overhang to maplen * ratio - 1, + 0, + 1 in turn.
                    ins = (overhang - (v % 3 - 1)) * per - maplen
                    if not 0 <= ins <= 100:
                        ins = 0
                    if ins:
                        mid = o1 + CORE // 2
                        x = _unlike(rng, ins, first=(short[mid - 1], short[mid]), last=(short[mid - 1], short[mid]))
                        short = np.concatenate((short[:mid], x, short[mid:]))
                    q, t = (g, short) if mirrored else (short, g)
                    add("%s/%g/o%d=%d" % ("ovm" if mirrored else "overhang", ratio, side, centre + v), "overhang", q, t,
                        ratio=ratio, mirrored=mirrored, side=side, v=v, ins=ins, overhang=overhang, maplen=maplen + ins,
                        twin=bool(ins) or abs(v) <= 2)


def _both(p, rng, add):
    # (a, c): starts of the forward and of the reverse-complemented part in a 6 kb target.  overhang of either chain =
    # min(2000, 6000 - end of its part): the other part of the query hangs over, and the target's tail bounds it.
    for label, a, c in (("both", 2500, 200), ("both/fwd-int", 3800, 500), ("both/rev-int", 500, 3800)):
        g = _rand(rng, 6000)
        q = np.concatenate((g[a:a + 2000], revcomp(g[c:c + 2000])))
        add(label, "both", q, g, a=a, c=c)


FAMILIES = (_band, _gap, _threshold, _overhang, _both)
_SEEDS = {"ont": 20240, "pb": 20241}


@functools.lru_cache(maxsize=None)
def build(preset):
    """every case of one preset, in a fixed order: (cases, query seqs, query names, target seqs, target names); read i of either
    set belongs to cases[i].  Every family is built twice, from different random draws: as described, and with every query
    reverse-complemented ("/rc"; the overhang sweeps only near their centre, where the inserted bases place the edge)."""
    p = PRESETS[preset]
    cases = []
    for rc in (False, True):
        def add(label, family, q, t, twin=True, **meta):
            if rc and not twin:
                return
            cases.append(Case(label + ("/rc" if rc else ""), family, revcomp(q) if rc else q, t, rc=rc, **meta))

        for f, fam in enumerate(FAMILIES):
            fam(p, np.random.Generator(np.random.PCG64([_SEEDS[preset], f, int(rc)])), add)
    qnames = [b"q%04d" % i for i in range(len(cases))]
    tnames = [b"t%04d" % i for i in range(len(cases))]
    return cases, [c.q for c in cases], qnames, [c.t for c in cases], tnames
