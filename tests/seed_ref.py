"""Plain numpy / Python-int models of the stages between the sorted minimizer stream and the anchor sort -- the ordered hash table of
lrge_amd/csrc/k_index.h (home slot, placement, table image, histogram, lookup) and the seed side of lrge_amd/csrc/k_seed.h (kept counts,
expansion into anchors, the dead-pair filter) -- and the case families that tests/test_gpu_seed.py runs on the device.  The models know
nothing of tiles, wavefronts or LDS, except where a NEAR MISS needs a border to go wrong at.  Every model takes the name of a near miss (a
plausible wrong kernel); tests/test_seed_ref.py proves on the CPU that each family holds a case on which the near miss and the truth
differ, so that the device comparison could tell them apart.  No wrong kernel ever runs on a GPU."""
import functools

import numpy as np

from prims_ref import U64, M64, u64, mask, shr, shl

HT_EMPTY = M64
HT_CNT_BITS = 24
HT_CNT_MAX = (1 << 24) - 1
HT_INLINE = 1 << 63
PLACE_TILE = 2048
PLACE_COMP = 384
SCAN_CHUNK = 1024                   # tile maxima k_place_scan takes per step
OCC_LDS_BINS = 2048
MAX_BIN = 1000001                   # the histogram's last bin in the presets (max_mid_occ + 1)
PATTERN64 = 0xA5A5A5A5A5A5A5A5      # what the harness leaves where nothing wrote
EXPQ_THREADS = (256, 512, 1024)     # the three classes of k_expand_q ...
EXPQ_LOG2B = (14, 16, 17)           # ... the log2 of their census buckets ...
EXPQ_ROUND = tuple(t * 8 for t in EXPQ_THREADS)     # ... and the anchors one compaction round takes
EXPQ_SMALL_MAX, EXPQ_MID_MAX = 8192, 32768


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


# ------------------------------------------------------------------------------------------
# significance string (vectorised; prims_ref has the scalar forms) and the home slot
# ------------------------------------------------------------------------------------------
def sig_to_hash(s, nbits):
    """s: the hash's bytes low byte first as ONE number, the partial top byte last (the stream's order)"""
    s = u64(s)
    m = (nbits + 7) // 8
    tb = nbits - 8 * (m - 1)
    h = shl(s & U64(mask(tb)), 8 * (m - 1))
    s = shr(s, tb)
    for j in range(m - 2, -1, -1):
        h |= shl(s & U64(0xff), 8 * j)
        s = shr(s, 8)
    return h


def hash_to_sig(h, nbits):
    h = u64(h)
    m = (nbits + 7) // 8
    tb = nbits - 8 * (m - 1)
    s = np.zeros_like(h)
    for j in range(m - 1):
        s = shl(s, 8) | (shr(h, 8 * j) & U64(0xff))
    return shl(s, tb) | (shr(h, 8 * (m - 1)) & U64(mask(tb)))


def byte_swap(a):
    return u64(a).byteswap()


def clamp_power(k, pw):
    """the exponent the table really uses: u^pw must span the 8 output bits and fit 56"""
    part = (2 * k) % 8
    if part == 0 or pw == 0:
        return 0
    return min(max(pw, -(-8 // part)), 56 // part)


def mul_high(a, cap):
    """high 64 bits of a * cap for cap < 2^32, in 32-bit halves"""
    assert 0 < cap < (1 << 32)
    a = u64(a)
    lo, hi = a & U64(0xFFFFFFFF), a >> U64(32)
    return (hi * U64(cap) + ((lo * U64(cap)) >> U64(32))) >> U64(32)


def home(keys, cap, k, pw, miss=None):
    """Home slot of a 2k-bit hash: its position in the byte-reversed order scaled to [0, cap).  The hash's top byte holds only
    part = 2k mod 8 bits; it is stretched to a full byte (v << (8 - part)) or, pw != 0, sent through 256 * (1 - (1 - v / 2^part)^pw)."""
    bs = byte_swap(keys)
    part = (2 * k) % 8
    if part and miss != "home_no_stretch":
        at = 64 - 8 * ((2 * k + 7) // 8)            # where the hash's top byte lies after the swap
        v = shr(bs, at) & U64(0xff)
        assert int(v.max(initial=0)) < (1 << part)
        pw = 0 if miss == "power_ignored" else clamp_power(k, pw)
        if pw == 0:
            f = v << U64(8 - part)
        else:
            u = U64(1 << part) - v
            p = np.ones_like(u)
            for _ in range(pw):
                p = p * u
            f = np.minimum(U64(256) - (p >> U64(part * pw - 8)), U64(255))
        bs = (bs & U64(M64 ^ (0xff << at))) | shl(f, at)
    return mul_high(bs, cap).astype(np.int64)


# ------------------------------------------------------------------------------------------
# placement and the table image
# ------------------------------------------------------------------------------------------
PLACE_MISSES = ("restart_64", "restart_256", "restart_2048", "restart_1024_tiles", "home_no_stretch", "power_ignored", "count_unclamped", "tail_not_cleared")


def place_slots(hm, miss=None):
    """slot(r) = max(home(r), slot(r - 1) + 1)"""
    n = hm.size
    d = hm - np.arange(n, dtype=np.int64)
    border = {"restart_64": 64, "restart_256": 256, "restart_2048": PLACE_TILE, "restart_1024_tiles": SCAN_CHUNK * PLACE_TILE}.get(miss)
    if border is None:
        acc = np.maximum.accumulate(d)
    else:                           # the running maximum forgets what lies in front of every border
        pad = (-n) % border
        acc = np.maximum.accumulate(np.concatenate([d, np.full(pad, np.iinfo(np.int64).min)]).reshape(-1, border), axis=1).reshape(-1)[:n]
    return acc + np.arange(n, dtype=np.int64)


def table(keys, starts, n_entries, ys, cap, n_slots, k, pw, inline, fused, max_bin=MAX_BIN, miss=None):
    """keys: the distinct hashes in stream order; starts: where each one's run begins among the n_entries entries; ys: the y value of
    every run's FIRST entry.  Returns (image of 2 * n_slots words or None when the placement overflows, histogram, overflow flag,
    last slot, displacement sum)."""
    keys, starts = u64(keys), np.asarray(starts, dtype=np.int64)
    n = keys.size
    hm = home(keys, cap, k, pw, miss)
    slot = place_slots(hm, miss)
    cnt = np.diff(np.concatenate([starts, [n_entries]]))
    hist = np.bincount(np.minimum(cnt, max_bin), minlength=max_bin + 1).astype(np.uint32)
    overflow = int((slot + 1 >= n_slots).any())
    last = int(min(slot[-1], n_slots - 1))
    disp = int((slot - hm).sum())
    if overflow:
        return None, hist, 1, last, disp
    img = np.full(2 * n_slots, HT_EMPTY, dtype=np.uint64)
    if miss == "tail_not_cleared" and fused:
        img[2 * (last + 1):] = PATTERN64
    val = shl(u64(starts), HT_CNT_BITS) | u64(cnt if miss == "count_unclamped" else np.minimum(cnt, HT_CNT_MAX))
    if inline:
        val = np.where(cnt == 1, U64(HT_INLINE) | u64(ys), val)
    img[2 * slot] = keys
    img[2 * slot + 1] = val
    return img, hist, 0, last, disp


LOOKUP_MISSES = ("mid_lt",)


def kept_len(c, mid_occ, miss=None):
    c = np.asarray(c, dtype=np.int64)
    return u32(np.where((c > 0) & ((c < mid_occ) if miss == "mid_lt" else (c <= mid_occ)), c, 0))


def lookup(keys, starts, n_entries, ys, inline, q_hash, mid_occ, miss=None, by_value=None):
    """dictionary semantics: hs = where the list lives (its start, or HT_INLINE | y of a singleton), hc = its length clamped to 2^24 - 1, hn
    (by_value: the keys' order by value, when the caller kept it)"""
    keys, q_hash = u64(keys), u64(q_hash)
    cnt = np.diff(np.concatenate([np.asarray(starts, dtype=np.int64), [n_entries]]))
    by_value = np.argsort(keys, kind="stable") if by_value is None else by_value
    at = np.minimum(np.searchsorted(keys[by_value], q_hash), keys.size - 1)
    r = by_value[at]
    found = keys[r] == q_hash
    single = found & (cnt[r] == 1) & bool(inline)
    hs = np.where(single, U64(HT_INLINE) | u64(ys)[r], np.where(found, u64(starts)[r], U64(0)))
    hc = u32(np.where(found, np.minimum(cnt[r], HT_CNT_MAX), 0))
    return u64(hs), hc, kept_len(hc, mid_occ, miss)


# ------------------------------------------------------------------------------------------
# the seed side
# ------------------------------------------------------------------------------------------
class Seeds:
    """the inputs of k_seed_counts / k_expand / k_expand_q as arrays (fields as in SeedParams and the kernels' arguments)"""
    pk_pos1 = 0
    pk_ybits = 0
    check_names = 0
    no_dual = 0
    krank = None

    def y_of(self, w):
        w = u64(w)
        if self.pk_ybits == 0:
            return w
        yb = w & U64(mask(self.pk_ybits))
        return shl(shr(yb, self.pk_pos1), 32) | (yb & U64(mask(self.pk_pos1)))


SEED_MISSES = ("mid_lt", "diag_ignores_len", "no_dual_ge", "ties_first_lane", "offset_absolute", "rev_qpos_no_span")


def _hits(S, n, b, e, origin, miss):
    """the hits of the minimizers [b, e) in minimizer order then list order: (owning minimizer, y, fields come from a real minimizer).
    origin: where the 64-minimizer stretches that share a scan start (the tie rule can only go wrong inside one)."""
    idx = np.arange(b, e, dtype=np.int64)
    nn = n[b:e].astype(np.int64)
    own = np.repeat(idx, nn)
    j = np.arange(own.size, dtype=np.int64) - np.repeat(np.cumsum(nn) - nn, nn)
    real = np.ones(own.size, dtype=bool)
    if miss == "ties_first_lane":
        # a hit goes to the FIRST minimizer of its stretch whose scanned start equals its owner's: the empty lists in front of the owner
        # inside the same stretch of 64 win, and an empty list carries no fields (all zero, its list "starts" at pos[0])
        first = idx.copy()
        for t in range(1, idx.size):
            if nn[t - 1] == 0 and (idx[t] - origin) // 64 == (idx[t - 1] - origin) // 64:
                first[t] = first[t - 1]
        real = np.repeat(first == idx, nn)
    st = S.hs[own]
    inl = (st & U64(HT_INLINE)) != 0
    st = np.where(real, st, U64(0))
    inl &= real
    at = np.where(inl, 0, (st & U64(HT_INLINE - 1)).astype(np.int64) + j)
    y = np.where(inl, st & U64(HT_INLINE - 1), S.y_of(S.pos[at]) if S.pos.size else U64(0))
    return own, u64(y), real


def _fields(S, own, y, real):
    z = lambda a: np.where(real, a, 0)
    qy = S.qy[own]
    q = z((qy >> U64(32)).astype(np.int64))
    qpos = z(((qy & U64(0xFFFFFFFF)) >> U64(1)).astype(np.int64))
    qs = z((qy & U64(1)).astype(np.int64))
    span = z((S.qx[own] & U64(0xff)).astype(np.int64)) if S.qx is not None else np.zeros(own.size, dtype=np.int64)
    ql = z(S.q_len[q].astype(np.int64))
    qr = z(S.q_rank[q].astype(np.int64))
    rid = (y >> U64(32)).astype(np.int64)
    rpos = ((y & U64(0xFFFFFFFF)) >> U64(1)).astype(np.int64)
    ts = (y & U64(1)).astype(np.int64)
    return q, qpos, qs, span, ql, qr, rid, rpos, ts


def _name_rules(S, ql, qr, qpos, rid, rpos, miss):
    """(dropped, same read): the exact diagonal of a read against itself goes; NO_DUAL keeps only qr <= tr"""
    if not S.check_names:
        return np.zeros(rid.size, dtype=bool), np.zeros(rid.size, dtype=bool)
    tr = S.t_rank[rid].astype(np.int64)
    same = (qr == tr) & (S.t_len[rid].astype(np.int64) == ql)
    diag = ((qr == tr) if miss == "diag_ignores_len" else same) & (rpos == qpos)
    drop = diag.copy()
    if S.no_dual:
        drop |= (qr >= tr) if miss == "no_dual_ge" else (qr > tr)
    return drop, same


def counts(S, miss=None):
    """hn = the list length of a kept seed (0 < c <= mid_occ), hv = its hits that survive the name rules"""
    hn = kept_len(S.hc, S.mid_occ, miss)
    own, y, real = _hits(S, hn, 0, hn.size, 0, None)
    q, qpos, qs, span, ql, qr, rid, rpos, ts = _fields(S, own, y, real)
    drop, _ = _name_rules(S, ql, qr, qpos, rid, rpos, miss)
    hv = np.bincount(own[~drop], minlength=hn.size).astype(np.uint32)
    return hn, hv


def scan0(a):
    return u32(np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(np.asarray(a, dtype=np.uint64))]) & U64(0xFFFFFFFF))


def expand(S, hn, aoff, b, e, q0, kl, packed_bits_qy=0, origin=None, miss=None):
    """The anchors of the minimizers [b, e), in minimizer order then list order, at aoff[minimizer] - aoff[b].  kl = (bits_rpos, bits_rid,
    bits_q).  Returns (key, value) of aoff[e] - aoff[b] entries, or the packed words and None.  Entries nothing wrote hold PATTERN64."""
    origin = b if origin is None else origin
    own, y, real = _hits(S, hn, b, e, origin, miss)
    q, qpos, qs, span, ql, qr, rid, rpos, ts = _fields(S, own, y, real)
    drop, same = _name_rules(S, ql, qr, qpos, rid, rpos, miss)
    slf = (same & (ts == qs)).astype(np.uint64)
    rev = ts != qs
    back = (ql - qpos - 1) if miss == "rev_qpos_no_span" else (ql - (qpos + 1 - span) - 1)
    qp = u64(np.where(rev, back, qpos) & 0xFFFFFFFF)
    sh_rev, sh_rid, sh_q = kl[0], kl[0] + 1, kl[0] + 1 + kl[1]
    key = shl(u64((q - q0) & 0xFFFFFFFF), sh_q) | shl(u64(rid), sh_rid) | shl(u64(rev), sh_rev) | u64(rpos)
    rank = np.zeros(own.size, dtype=np.uint64)
    if S.krank is not None:
        rank = u64(np.where(real, (S.krank[own].astype(np.int64) - S.krank[S.qmz_off[q]].astype(np.int64)) & 0xFFFFF, 0))
    val = shl(rank, 44) | shl(slf, 43) | shl(u64(span), 32) | qp
    keep = ~drop
    key, val = key[keep], val[keep]
    n_out = int(aoff[e]) - int(aoff[b])
    # where the stretch of 64 minimizers that holds the owner starts writing, plus the hit's rank among the stretch's survivors
    w0 = origin + (own[keep] - origin) // 64 * 64
    w0 = np.maximum(w0, b)
    base = aoff[w0].astype(np.int64) - (0 if miss == "offset_absolute" else int(aoff[b]))
    first_of_w0 = np.searchsorted(w0, w0, side="left")
    at = base + (np.arange(w0.size) - first_of_w0)
    ok = (at >= 0) & (at < n_out)
    ok_k = np.full(n_out, PATTERN64, dtype=np.uint64)
    ok_v = np.full(n_out, PATTERN64, dtype=np.uint64)
    if packed_bits_qy:
        sb = sh_q
        pk = (key & U64(mask(sb))) | shl(val & U64(0xFFFFFFFF), sb) | shl(shr(val, 32) & U64(0xff), sb + packed_bits_qy) | shl(shr(val, 43) & U64(1), sb + packed_bits_qy + 8)
        ok_k[at[ok]] = pk[ok]
        return ok_k, None
    ok_k[at[ok]] = key[ok]
    ok_v[at[ok]] = val[ok]
    return ok_k, ok_v


def pair_bucket(rid_rev, log2b):
    """the documented multiplicative hash of rid << 1 | rev"""
    return ((u64(rid_rev) * U64(0x9E3779B1)) & U64(0xFFFFFFFF)) >> U64(32 - log2b)


def expq_class(total, smax=EXPQ_SMALL_MAX, mmax=EXPQ_MID_MAX):
    return 0 if total <= smax else 1 if total <= mmax else 2


EXPQ_MISSES = ("threshold_minus_1", "swap_waves", "swap_rounds", "ties_first_lane", "rev_qpos_no_span")


def expand_q(S, hn, aoff, mz_begin, q, q0, kl, bits_qy, n_planes, smax, mmax, miss=None):
    """One query of a k_expand_q launch: (where its slot starts in the buffer, the slot's size, the survivors in emission order).  An
    anchor survives when its pair's bucket -- the class's hash of rid << 1 | rev -- received at least n_planes of the query's anchors."""
    mb, me = int(S.qmz_off[q]), int(S.qmz_off[q + 1])
    seg0, tot = int(aoff[mb]) - int(aoff[mz_begin]), int(aoff[me]) - int(aoff[mb])
    if tot == 0:
        return seg0, 0, np.zeros(0, dtype=np.uint64)
    cls = expq_class(tot, smax, mmax)
    pm = miss if miss in ("ties_first_lane", "rev_qpos_no_span") else None
    pk, _ = expand(S, hn, aoff, mb, me, q0, kl, bits_qy, origin=mb, miss=pm)
    sb = kl[0] + 1 + kl[1]
    b = pair_bucket((pk & U64(mask(sb))) >> U64(kl[0]), EXPQ_LOG2B[cls]).astype(np.int64)
    cnt = np.bincount(b, minlength=1 << EXPQ_LOG2B[cls])
    live = cnt[b] >= (n_planes - 1 if miss == "threshold_minus_1" else n_planes)
    order = np.arange(tot)
    R = EXPQ_ROUND[cls]
    if miss == "swap_waves" and tot > 512:          # the survivors of the first two wavefronts' items change places in every round
        for r0 in range(0, tot, R):
            a, m, z = r0, min(r0 + 512, tot), min(r0 + 1024, tot)
            order = np.concatenate([order[:a], order[m:z], order[a:m], order[z:]])
    if miss == "swap_rounds" and tot > R:
        order = np.concatenate([order[R:min(2 * R, tot)], order[:R], order[min(2 * R, tot):]])
    return seg0, tot, pk[order][live[order]]


# ==========================================================================================
# case families (fixed seeds)
# ==========================================================================================
def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _distinct_sigs(rng, n, nbits, lo=0, hi=None):
    """n distinct sorted significance strings, uniform over [lo, hi)"""
    hi = (1 << nbits) if hi is None else hi
    assert hi - lo >= 2 * n
    s = np.unique(rng.integers(lo, hi, int(n * 1.1) + 16, dtype=np.uint64))
    while s.size < n:
        s = np.unique(np.concatenate([s, rng.integers(lo, hi, n, dtype=np.uint64)]))
    return np.sort(rng.choice(s, n, replace=False))


def _cluster(s, at, length, step=1):
    """the sigs [at, at + length) become an arithmetic stretch behind s[at]: neighbours in the order, nearly one home"""
    s = s.copy()
    length = min(length, s.size - at)
    s[at:at + length] = s[at] + U64(step) * np.arange(length, dtype=np.uint64)
    assert (np.diff(s.astype(np.int64)) > 0).all(), "the stretch ran into the next key"
    return s


def _boundary_sigs(rng, k, pw, cap, count):
    """Hashes whose home lies within the partial byte's reach of a slot border: everything but that byte puts them just below slot t,
    and whether the byte lifts them into t depends on what is made of it -- left as it is, stretched, or sent through the power map.
    (With a small table the partial byte moves a random key's home with a probability of the order of cap / 2^32; these keys make the
    stretch and the exponent visible at any cap.)  Half of them tell stretched from unstretched, half the power map from the stretch."""
    nbits, part = 2 * k, (2 * k) % 8
    at = 64 - 8 * ((nbits + 7) // 8)
    pw = clamp_power(k, pw)
    kinds = [[], []]
    tries = 0
    while part and tries < 200 * count and (len(kinds[0]) < count // 2 or (pw and len(kinds[1]) < count // 2)):
        tries += 1
        t = int(rng.integers(1, cap))
        rest = ((t << 64) // cap >> (at + 8)) << (at + 8)              # the swapped hash without its partial byte: home t - 1 or t
        need = (t << 64) - rest * cap                                   # the byte's value f reaches slot t when f * (cap << at) >= need
        for v in rng.permutation(np.arange(1, 1 << part)):
            v = int(v)
            up = [f * (cap << at) >= need for f in (v, v << (8 - part), min(255, 256 - ((((1 << part) - v) ** pw) >> (part * pw - 8))) if pw else 0)]
            which = 0 if up[0] != up[1] else 1 if pw and up[1] != up[2] else None
            if which is not None and len(kinds[which]) < count // 2:
                kinds[which].append(rest | v << at)
                break
    out = kinds[0] + kinds[1]
    return hash_to_sig(byte_swap(u64(out)), nbits) if out else np.zeros(0, dtype=np.uint64)


TABLE_N = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 3 * 2048 + 5)
TABLE_BIG_N = 1025 * 2048 + 1
TABLE_K = (13, 14, 15, 16, 19)
TABLE_PW = (0, 3, 1, 100)           # (1 and 100: clamped to the smallest and the largest exponent the width takes)
RUN_LENGTHS = (1, 2, 3, 2047, 2048, 2049, MAX_BIN - 1, MAX_BIN, MAX_BIN + 1, (1 << 24) - 1, 1 << 24, (1 << 24) + 1)
TABLE_FAMILIES = ("sizes", "big", "clustered", "sparse", "mixed", "grid_cap", "run_lengths", "widths", "overflow")


class TableCase:
    """sigs in stream order with their run lengths; cap / n_slots / grid_cap as the harness takes them"""

    def __init__(self, name, k, pw, sigs, lens=None, cap=None, slack=None, grid_cap=2048, seed=0, sparse=False, max_bin=MAX_BIN):
        self.name, self.k, self.pw, self.nbits = name, k, pw, 2 * k
        self.sigs = u64(sigs)
        n = self.n = self.sigs.size
        rng = _rng(1000 + seed)
        self.lens = np.asarray(lens, dtype=np.int64) if lens is not None else rng.choice([1, 1, 1, 2, 3], n).astype(np.int64)
        self.starts = np.concatenate([[0], np.cumsum(self.lens)[:-1]]).astype(np.int64)
        self.M = int(self.lens.sum())
        self.cap = cap if cap is not None else max(2 * n, 1024)
        self.n_slots = self.cap + (slack if slack is not None else max(n // 16, 4096))
        self.grid_cap, self.sparse, self.max_bin = grid_cap, sparse, max_bin
        self.keys = sig_to_hash(self.sigs, self.nbits)
        # the packed entry: hash << ybits | rid << pk_pos1 | pos << 1 | strand
        self.ybits = min(26, 64 - self.nbits)
        self.pk_pos1 = self.ybits - 8
        self.yb_head = rng.integers(0, 1 << self.ybits, n, dtype=np.uint64)         # of every run's first entry
        self.ypos_head = rng.integers(0, 1 << 62, n, dtype=np.uint64)

    def y_heads(self, packed):
        if not packed:
            return self.ypos_head
        return shl(shr(self.yb_head, self.pk_pos1), 32) | (self.yb_head & U64(mask(self.pk_pos1)))

    def stream(self, packed):
        """(skey, ypos or None, kshift): all M entries, or one per run when the case is sparse"""
        rep = (lambda a: a) if self.sparse else (lambda a: np.repeat(a, self.lens))
        if packed:
            w = rep(shl(self.keys, self.ybits) | self.yb_head)
            if not self.sparse:     # the entries behind a run's head carry other positions
                w = (w & ~U64(mask(self.ybits))) | ((w + u64(np.arange(w.size) * 7919)) & U64(mask(self.ybits)))
                w[self.starts] = shl(self.keys, self.ybits) | self.yb_head
            return w, None, self.ybits
        y = rep(self.ypos_head)
        if not self.sparse:
            y = y ^ u64(np.arange(y.size) * 3)
            y[self.starts] = self.ypos_head
        return rep(self.keys), y, 0

    def model(self, packed, inline, fused, miss=None):
        return table(self.keys, self.starts, self.M, self.y_heads(packed), self.cap, self.n_slots, self.k, self.pw, inline, fused, self.max_bin, miss)

    def lookup(self, packed, inline, q_hash, mid_occ):
        if not hasattr(self, "_by_value"):
            self._by_value = np.argsort(self.keys, kind="stable")
        return lookup(self.keys, self.starts, self.M, self.y_heads(packed), inline, q_hash, mid_occ, by_value=self._by_value)

    def absent(self):
        """hashes that are not in the table: below the smallest, above the largest, and between neighbours in the order"""
        cand = [int(self.sigs[0]) - 1, int(self.sigs[-1]) + 1] + [int(x) + 1 for x in self.sigs[:: max(1, self.n // 64)]]
        cand = u64([c for c in cand if 0 <= c < (1 << self.nbits)])
        return sig_to_hash(cand[~np.isin(cand, self.sigs)], self.nbits)


@functools.lru_cache(maxsize=None)
def table_cases(family):
    out = []
    if family == "sizes":
        for i, n in enumerate(TABLE_N):
            s = _distinct_sigs(_rng(10 + i), n, 38)
            if n > 300:             # one chain over every 64-lane and 256-thread border of its stretch, and over the tile border where there is one
                s = _cluster(s, min(n, 2048) - 300, 600, 2)
            elif n > 60:            # ... to the last run: over the border at 64 or 256 where the size has one
                s = _cluster(s, n // 4, n - n // 4, 2)
            out.append(TableCase("n%d" % n, 19, 3, s, seed=i))
    elif family == "big":           # k_place_scan's second chunk of 1024 tile maxima; a chain across the border between the two
        s = _distinct_sigs(_rng(30), TABLE_BIG_N, 38)
        s = _cluster(s, SCAN_CHUNK * PLACE_TILE - 40, 100, 2)
        out.append(TableCase("n%d" % TABLE_BIG_N, 19, 3, s, seed=30))
    elif family == "clustered":     # keys that share their low bytes: ONE displacement chain over wave, row and tile borders
        for i, n in enumerate((65, 257, 2049, 3 * 2048 + 5)):
            s = U64(0x12345 << 14) + U64(2) * np.arange(n, dtype=np.uint64)
            out.append(TableCase("chain%d" % n, 19, 3, s, slack=n + 4096, seed=40 + i))
    elif family == "sparse":        # a wavefront's slots span far more than PLACE_COMP
        for i, n in enumerate((65, 2049, 3 * 2048 + 5)):
            out.append(TableCase("sparse%d" % n, 19, 3, _distinct_sigs(_rng(50 + i), n, 38), cap=64 * n, seed=50 + i))
    elif family == "mixed":         # inside one tile: dense chains between sparse stretches
        n = 2 * 2048 + 77
        s = _distinct_sigs(_rng(60), n, 38)
        for at in (100, 700, 1500, 2040, 3000):
            s = _cluster(s, at, 130, 2)
        out.append(TableCase("mixed", 19, 3, s, cap=24 * n, seed=60))
        s = _distinct_sigs(_rng(61), n, 30)
        for at in (100, 700, 1500, 2040, 3000):
            s = _cluster(s, at, 130, 2)
        out.append(TableCase("mixed_k15_pw0", 15, 0, s, cap=24 * n, seed=61))
    elif family == "grid_cap":      # 2 blocks stride over 7 tiles
        n = 7 * 2048 - 3
        s = _cluster(_distinct_sigs(_rng(70), n, 38), 3 * 2048 - 50, 100, 2)
        out.append(TableCase("grid2", 19, 3, s, grid_cap=2, seed=70))
    elif family == "run_lengths":   # only the run heads are read: the harness places one entry per run
        lens = np.array(RUN_LENGTHS, dtype=np.int64)
        out.append(TableCase("lengths", 19, 3, _distinct_sigs(_rng(80), lens.size, 38), lens=lens, seed=80, sparse=True))
        out.append(TableCase("lengths_small_bins", 19, 3, _distinct_sigs(_rng(81), 9, 38), lens=[1, 2, 3, 2047, 2048, 2049, 4999, 5000, 5001], seed=81, sparse=True, max_bin=5000))
    elif family == "widths":        # partial widths 2, 4, 6, none, 6
        for k in TABLE_K:
            for pw in TABLE_PW:
                n = 2049
                s = _distinct_sigs(_rng(90 + k), n, 2 * k)
                s = _cluster(s, 1000, 90, 1)
                s = np.unique(np.concatenate([s, _boundary_sigs(_rng(190 + k), k, pw, max(2 * n, 1024), 64)]))[:n]
                out.append(TableCase("k%d_pw%d" % (k, pw), k, pw, s, seed=90 + k))
    elif family == "overflow":      # homes packed against the end: (too little slack, enough slack)
        n = 2049
        s = U64((1 << 38) - 1) - np.arange(n, dtype=np.uint64)[::-1]
        out.append(TableCase("short", 19, 3, s, slack=n - 300, seed=95))
        out.append(TableCase("short_by_one", 19, 3, s, slack=n - 1, seed=95))
        out.append(TableCase("enough", 19, 3, s, slack=n, seed=95))
        s = U64((1 << 38) - 1) - np.arange(64, dtype=np.uint64)[::-1]
        out.append(TableCase("short64_by_one", 19, 3, s, slack=63, seed=96))
        out.append(TableCase("enough64", 19, 3, s, slack=64, seed=96))
    return tuple(out)


# ---- segment-packed streams: the entry keeps the low nbits - 8 - e bits of the sig, the rest is the number of its segment ----
SEG_E = (0, 6)


class SegCase(TableCase):
    def __init__(self, name, e, sigs, **kw):
        TableCase.__init__(self, name, 19, 3, sigs, **kw)
        self.e = e
        self.nr = self.nbits - 8 - e
        self.ybits = min(26, 64 - self.nr)
        self.pk_pos1 = self.ybits - 8
        self.yb_head &= U64(mask(self.ybits))
        seg = shr(self.sigs, self.nr).astype(np.int64)
        per_run = np.bincount(seg, weights=self.lens, minlength=256 << e).astype(np.int64)
        self.seg_start = u32(np.concatenate([[0], np.cumsum(per_run)[:-1]]))
        self.seg_used = np.unique(seg)

    def stream(self, packed=True):
        w = np.repeat(shl(self.sigs & U64(mask(self.nr)), self.ybits) | self.yb_head, self.lens)
        w = (w & ~U64(mask(self.ybits))) | ((w + u64(np.arange(w.size) * 7919)) & U64(mask(self.ybits)))
        w[self.starts] = shl(self.sigs & U64(mask(self.nr)), self.ybits) | self.yb_head
        return w, None, self.ybits


@functools.lru_cache(maxsize=None)
def seg_cases():
    out = []
    for e in SEG_E:
        nr = 38 - 8 - e
        n_seg = 256 << e
        # occupied segments with empty ones in front, between and behind; the second group's segments are so thin that one tile crosses many
        used = np.array([3, 4, 5, 9] + list(range(n_seg // 2, n_seg // 2 + 40, 3)) + [n_seg - 7], dtype=np.int64)
        rng = _rng(200 + e)
        n = 3 * 2048 + 5
        per = np.full(used.size, 30, dtype=np.int64)
        per[:4] = (n - 30 * (used.size - 4)) // 4
        per[0] += n - per.sum()
        s = np.concatenate([_distinct_sigs(rng, int(c), 38, int(g) << nr, (int(g) + 1) << nr) for g, c in zip(used, per)])
        s = _cluster(np.sort(s), 2048 - 60, 120, 2)
        out.append(SegCase("seg_e%d" % e, e, s, seed=200 + e))
    return tuple(out)


# ---- the seed side: scenarios built from per-minimizer hit lists ----
MID_OCC = 70


def build_seeds(queries, nt, mid_occ=MID_OCC, packed_pos=False, check_names=0, no_dual=0, with_krank=False, seed=0, t_len=None, t_rank=None, q_len=None, q_rank=None,
                pos_prefix=3):
    """queries: per query a list of minimizers, each (kind, ys[, qpos, strand, span]) with kind 'absent' (no list), 'inline' (one hit in
    the slot), 'pos' (the list in pos[]) or 'over' (a list in pos[] one longer than mid_occ allows -- ys may be anything of that length)."""
    rng = _rng(5000 + seed)
    S = Seeds()
    S.mid_occ, S.check_names, S.no_dual = mid_occ, check_names, no_dual
    nq = S.nq = len(queries)
    S.nt = nt
    qx, qy, hs, hc, pos, off = [], [], [], [], [0] * pos_prefix, [0]
    if packed_pos:
        S.pk_pos1, S.pk_ybits = 20, 20 + max(1, int(nt - 1).bit_length())
    for q, mzs in enumerate(queries):
        at = 300                    # (a minimizer's position is its END: at least span - 1)
        for m in mzs:
            kind, ys = m[0], [int(v) for v in m[1]]
            qpos = m[2] if len(m) > 2 and m[2] is not None else at
            strand = m[3] if len(m) > 3 else int(rng.integers(0, 2))
            span = m[4] if len(m) > 4 else int(rng.integers(15, 40))
            at = qpos + int(rng.integers(1, 9))
            qx.append(int(rng.integers(0, 1 << 38)) << 8 | span)
            qy.append(q << 32 | qpos << 1 | strand)
            if kind == "absent":
                hs.append(0); hc.append(0)
            elif kind == "inline":
                assert len(ys) == 1
                hs.append(HT_INLINE | ys[0]); hc.append(1)
            else:
                hs.append(len(pos)); hc.append(len(ys))
                assert (kind == "over") == (len(ys) > mid_occ)
                for v in ys:
                    pos.append(((int(rng.integers(0, 1 << 10)) << S.pk_ybits) | (v >> 32) << S.pk_pos1 | (v & 0xFFFFFFFF)) if packed_pos else v)
                    assert not packed_pos or (v & 0xFFFFFFFF) < (1 << S.pk_pos1)
        off.append(len(qx))
    S.qx, S.qy, S.hs, S.hc, S.pos = u64(qx), u64(qy), u64(hs), u32(hc), u64(pos)
    S.n_mz = S.qx.size
    S.qmz_off = u32(off)
    qmax = [max([(int(v) & 0xFFFFFFFF) >> 1 for v in S.qy[off[q]:off[q + 1]]] + [0]) + 300 for q in range(nq)]
    S.q_len = u32(q_len if q_len is not None else qmax)
    S.q_rank = u32(q_rank if q_rank is not None else np.arange(nq) + 10)
    S.t_len = u32(t_len if t_len is not None else rng.integers(1000, 50000, nt))
    S.t_rank = u32(t_rank if t_rank is not None else np.arange(nt) + 10 + nq)
    if with_krank:      # the exclusive scan of "kept" over all minimizers
        S.krank = scan0(kept_len(S.hc, mid_occ) != 0)
    return S


def y_val(rid, rpos, strand):
    return rid << 32 | rpos << 1 | strand


def _list(rng, n, nt, bits_rpos=16):
    return [y_val(int(rng.integers(0, nt)), int(rng.integers(0, 1 << bits_rpos)), int(rng.integers(0, 2))) for _ in range(n)]


SEED_FAMILIES = ("lengths", "wave_totals", "zero_lists", "names", "layouts")


class SeedCase:
    """one launch of k_seed_counts + k_expand: the window [b, e) of the scenario's minimizers, the first query q0, the key layout"""

    def __init__(self, name, S, b=0, e=None, q0=0, kl=(17, 8, 6), bits_qy=0):
        self.name, self.S, self.b, self.e, self.q0, self.kl, self.bits_qy = name, S, b, S.n_mz if e is None else e, q0, kl, bits_qy

    def truth(self, miss=None):
        hn, hv = counts(self.S, miss if miss in ("mid_lt", "diag_ignores_len", "no_dual_ge") else None)
        aoff = scan0(hv)
        k, v = expand(self.S, hn, aoff, self.b, self.e, self.q0, self.kl, self.bits_qy, miss=miss)
        return (hn, hv, k) if v is None else (hn, hv, k, v)


@functools.lru_cache(maxsize=None)
def seed_cases(family):
    out = []
    nt = 200
    if family == "lengths":         # list lengths 0, 1 inline, 1 in pos[], 63, 64, 65, mid_occ, mid_occ + 1; a window inside the array
        rng = _rng(300)
        L = lambda n: _list(rng, n, nt)
        q0 = [("pos", L(5)), ("absent", []), ("inline", L(1)), ("pos", L(1)), ("pos", L(63)), ("pos", L(64)), ("absent", []), ("pos", L(65)),
              ("pos", L(MID_OCC)), ("over", L(MID_OCC + 1)), ("inline", L(1))]
        q1 = [("pos", L(int(rng.integers(1, 9)))) if i % 3 else ("absent", []) for i in range(150)]
        q2 = [("inline", L(1)) if i % 2 else ("pos", L(2)) for i in range(77)]
        for packed_pos in (False, True):
            for kr in (False, True):
                S = build_seeds([q0, q1, q2], nt, packed_pos=packed_pos, with_krank=kr, seed=300)
                tag = ("_pk" if packed_pos else "") + ("_rank" if kr else "")
                out.append(SeedCase("all" + tag, S))
                out.append(SeedCase("window" + tag, S, b=int(S.qmz_off[1]), e=int(S.qmz_off[2]) + 33, q0=1))
                out.append(SeedCase("window_packed" + tag, S, b=int(S.qmz_off[1]) + 5, e=S.n_mz - 3, q0=1, bits_qy=12))
    elif family == "wave_totals":   # 64 minimizers that sum to 64, 0, 65, 128 and 64 * mid_occ, one wave each
        rng = _rng(310)
        L = lambda n: _list(rng, n, nt)
        waves = [[("inline", L(1))] * 64, [("absent", [])] * 64, [("pos", L(1))] * 63 + [("pos", L(2))], [("pos", L(2))] * 64, [("pos", L(MID_OCC))] * 64,
                 [("pos", L(3))] * 37]
        mzs = [m for w in waves for m in w]
        S = build_seeds([mzs[:200], mzs[200:]], nt, seed=310, with_krank=True)
        out.append(SeedCase("waves", S))
        out.append(SeedCase("waves_packed", S, bits_qy=13))
        out.append(SeedCase("waves_shifted", S, b=64, e=S.n_mz - 1, q0=0))
    elif family == "zero_lists":    # empty lists first, last and between non-empty ones inside a stretch of 64
        rng = _rng(320)
        L = lambda n: _list(rng, n, nt)
        pat = []
        for i in range(64 * 3 + 21):
            w = i % 64
            pat.append(("absent", []) if w in (0, 1, 5, 6, 7, 20, 40, 41, 62, 63) or (i > 128 and i % 2) else ("pos", L(1 + i % 4)) if i % 5 else ("inline", L(1)))
        S = build_seeds([pat[:100], pat[100:]], nt, seed=320, with_krank=True)
        out.append(SeedCase("holes", S))
        out.append(SeedCase("holes_window", S, b=37, e=S.n_mz - 2))
        out.append(SeedCase("holes_packed", S, b=37, bits_qy=12))
    elif family == "names":         # the diagonal rule, the SELF bit and NO_DUAL
        nq_, nt_ = 4, 6
        # targets 0..3 are the queries themselves (same rank, same length); 4 shares query 1's rank with another length; 5 is a stranger
        q_len, q_rank = [5000, 6000, 7000, 8000], [20, 21, 22, 23]
        t_len, t_rank = q_len + [6001, 6000], q_rank + [21, 99]
        qs = []
        for q in range(nq_):
            mzs = []
            for i in range(70):
                qpos, strand = 100 + 31 * i, i & 1
                ys = [y_val(q, qpos, strand), y_val(q, qpos, strand ^ 1),                 # the exact diagonal, on both strand relations
                      y_val(q, qpos + 2, strand), y_val(q, qpos + 2, strand ^ 1),         # the same read at another position (SELF on one)
                      y_val(4, qpos, strand), y_val(5, qpos, strand)]                     # the same rank with another length; a stranger at that position
                ys += [y_val(t, 50 + i, i & 1) for t in range(nq_)]                       # qr <, =, > tr
                if i % 7 == 0:
                    mzs.append(("inline", [ys[i // 7 % len(ys)]], qpos, strand))
                elif i % 11 == 0:
                    mzs.append(("absent", [], qpos, strand))
                else:
                    mzs.append(("pos", ys[i % 3:], qpos, strand))
            qs.append(mzs)
        for cn, nd, tag in ((0, 0, "off"), (1, 0, "dual"), (1, 1, "no_dual")):
            S = build_seeds(qs, nt_, check_names=cn, no_dual=nd, with_krank=True, seed=330, t_len=t_len, t_rank=t_rank, q_len=q_len, q_rank=q_rank)
            out.append(SeedCase(tag, S, kl=(14, 3, 2)))
            out.append(SeedCase(tag + "_window_packed", S, b=75, e=S.n_mz - 9, q0=1, kl=(14, 3, 2), bits_qy=13))
    elif family == "layouts":       # 1-bit fields; the packed word filled to bit 63; span 255
        rng = _rng(340)
        mz = lambda n, sp: ("pos", [y_val(int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(0, 2))) for _ in range(n)], None, int(rng.integers(0, 2)), sp)
        S = build_seeds([[mz(1 + i % 5, 255 if i % 3 == 0 else 15) for i in range(90)], [mz(2, 255) for i in range(40)]], 2, seed=340, with_krank=True,
                        t_len=[900, 900], q_len=[1200, 1200])
        out.append(SeedCase("one_bit_fields", S, kl=(1, 1, 1)))
        out.append(SeedCase("one_bit_fields_packed", S, kl=(1, 1, 1), bits_qy=11))
        rng = _rng(341)
        nt2 = 1 << 12
        big = lambda n, sp: ("pos", [y_val(int(rng.integers(0, nt2)), int(rng.integers(0, 1 << 30)), int(rng.integers(0, 2))) for _ in range(n)], None, int(rng.integers(0, 2)), sp)
        S2 = build_seeds([[big(1 + i % 4, 255 if i % 2 else 21) for i in range(130)]], nt2, seed=341, q_len=[(1 << 12) - 1])
        kl = (30, 12, 1)            # sh_q = 43; 43 + 12 + 9 == 64
        assert kl[0] + 1 + kl[1] + 12 + 9 == 64
        out.append(SeedCase("word_filled", S2, kl=kl, bits_qy=12))
    return tuple(out)


# ---- k_expand_q ----
EXPQ_POPULATIONS = ("none", "all", "alternating", "one_bucket")
EXPQ_NT = 1 << 20


@functools.lru_cache(maxsize=None)
def _one_pair_per_bucket(log2b):
    x = np.arange(2, 2 * EXPQ_NT, dtype=np.uint64)
    _, first = np.unique(pair_bucket(x, log2b), return_index=True)
    return x[np.sort(first)]


def _distinct_bucket_pairs(log2b, n, avoid=()):
    """n values of rid << 1 | rev whose buckets differ from one another and from those of `avoid`"""
    x = _one_pair_per_bucket(log2b)
    if len(avoid):
        x = x[~np.isin(pair_bucket(x, log2b), pair_bucket(u64(avoid), log2b))]
    assert x.size >= n
    return x[:n]


@functools.lru_cache(maxsize=None)
def _same_bucket_pairs(log2b, n):
    x = np.arange(2, 2 * EXPQ_NT, dtype=np.uint64)
    b = pair_bucket(x, log2b)
    x = x[b == b[12345]]
    assert x.size >= n
    return x[:n]


def _expq_query(rng, total, population, log2b, n_planes):
    """the minimizers of one query whose lists hold exactly `total` hits"""
    if population == "none":
        pr = _distinct_bucket_pairs(log2b, total)
    elif population == "all":
        pr = u64(np.arange(total) % 5 + 2)
        if total < 5 * n_planes:                    # (too few anchors to fill five pairs: one pair takes them, dead when total < n_planes)
            pr = np.full(total, 2, dtype=np.uint64)
    elif population == "alternating":               # a live pair's anchor, a dead one's, ...: the dead pairs hold n_planes - 1 anchors each, one too few
        live = u64([2, 3, 4])
        dead = _distinct_bucket_pairs(log2b, total, avoid=live)
        pr = np.where(np.arange(total) % 2 == 0, live[np.arange(total) % 3], dead[np.arange(total) // 2 // (n_planes - 1)])
    else:                                           # many pairs in one bucket, each alone: the bucket's count keeps them all
        c = _same_bucket_pairs(log2b, 6)
        pr = c[np.arange(total) % 6]
    ys = [y_val(int(p) >> 1, int(rng.integers(0, 1 << 16)), 0) | (int(p) & 1) for p in pr]      # (query strand 0: the y's strand is `rev`)
    mzs, at, i = [], 0, 0
    while at < total or i < 3:
        n = min(total - at, (0, 1, 3, 1, 0, 17, 2, 64, 1, 5)[i % 10])
        if n == 0:
            mzs.append(("absent", [], None, 0))
        elif n == 1 and i % 4 == 1:
            mzs.append(("inline", ys[at:at + 1], None, 0))
        else:
            mzs.append(("pos", ys[at:at + n], None, 0))
        at += n
        i += 1
    return mzs


class ExpqCase:
    """one expand_q_launch: the scenario, the launch's queries [q0, q0 + nqb), the buffer's window of minimizers, the class thresholds"""

    def __init__(self, name, S, q0, nqb, smax, mmax, n_planes, kl=(17, 21, 4), bits_qy=16):
        self.name, self.S, self.q0, self.nqb, self.smax, self.mmax, self.n_planes, self.kl, self.bits_qy = name, S, q0, nqb, smax, mmax, n_planes, kl, bits_qy
        self.hn, hv = counts(S)
        self.aoff = scan0(hv)
        self.mz_begin = int(S.qmz_off[max(0, q0 - 1)])             # the slot of the query in front of the launch lies in the buffer ...
        self.mz_end = int(S.qmz_off[min(S.nq, q0 + nqb + 1)])      # ... and that of the one behind it
        self.n_out = int(self.aoff[self.mz_end]) - int(self.aoff[self.mz_begin])

    def totals(self):
        o = self.S.qmz_off
        return [int(self.aoff[o[q + 1]]) - int(self.aoff[o[q]]) for q in range(self.q0, self.q0 + self.nqb)]

    def truth(self, miss=None):
        """(the buffer with PATTERN64 wherever nothing is specified, kept[])"""
        buf = np.full(self.n_out, PATTERN64, dtype=np.uint64)
        kept = np.zeros(self.nqb, dtype=np.uint32)
        for q in range(self.q0, self.q0 + self.nqb):
            seg0, tot, live = expand_q(self.S, self.hn, self.aoff, self.mz_begin, q, self.q0, self.kl, self.bits_qy, self.n_planes, self.smax, self.mmax, miss)
            buf[seg0:seg0 + live.size] = live
            kept[q - self.q0] = live.size
        return buf, kept

    def specified(self, kept):
        """which words of the buffer the comparison may look at: all but what lies behind kept[q] in a launched query's slot"""
        m = np.ones(self.n_out, dtype=bool)
        o = self.S.qmz_off
        for q in range(self.q0, self.q0 + self.nqb):
            seg0 = int(self.aoff[o[q]]) - int(self.aoff[self.mz_begin])
            m[seg0 + int(kept[q - self.q0]):seg0 + int(self.aoff[o[q + 1]]) - int(self.aoff[o[q]])] = False
        return m

    def emitted(self, q):
        """every anchor of query q in emission order (no filter)"""
        mb, me = int(self.S.qmz_off[q]), int(self.S.qmz_off[q + 1])
        return expand(self.S, self.hn, self.aoff, mb, me, self.q0, self.kl, self.bits_qy, origin=mb)[0]


# the thresholds that force a class whatever the total: (smax, mmax)
EXPQ_FORCE = ((1 << 30, 1 << 30), (0, 1 << 30), (0, 0))


def expq_totals(cls):
    R = EXPQ_ROUND[cls]
    return (0, 1, R - 1, R, R + 1, 3 * R + 17)


@functools.lru_cache(maxsize=None)
def expq_cases(cls, n_planes, population):
    """queries of every total of the class, each launched alone between two neighbours that stay outside the launch"""
    out = []
    for i, total in enumerate(expq_totals(cls)):
        rng = _rng(400 + 10 * cls + i)
        nb = [("pos", _list(rng, 3, 50), None, 0), ("absent", [], None, 0), ("pos", _list(rng, 2, 50), None, 0)]
        S = build_seeds([nb, _expq_query(rng, total, population, EXPQ_LOG2B[cls], n_planes), nb], EXPQ_NT, seed=400 + i)
        out.append(ExpqCase("c%d_t%d" % (cls, total), S, 1, 1, EXPQ_FORCE[cls][0], EXPQ_FORCE[cls][1], n_planes))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expq_mixed_case(n_planes):
    """one launch over queries of all three classes by their own totals, a query without minimizers and one without hits among them"""
    rng = _rng(450)
    qs = [_expq_query(rng, 700, "alternating", 14, n_planes), [], _expq_query(rng, 40000, "alternating", 17, n_planes), _expq_query(rng, 0, "all", 14, n_planes),
          _expq_query(rng, 9000, "all", 16, n_planes), _expq_query(rng, 8192, "one_bucket", 14, n_planes), _expq_query(rng, 8193, "none", 16, n_planes),
          _expq_query(rng, 33, "all", 14, n_planes)]
    S = build_seeds(qs, EXPQ_NT, seed=450)
    return ExpqCase("mixed", S, 0, len(qs), EXPQ_SMALL_MAX, EXPQ_MID_MAX, n_planes)
