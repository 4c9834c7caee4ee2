"""The stages between the sorted minimizer stream and the anchor sort against the plain models of tests/seed_ref.py, bit for bit, on the
device: the ordered table build of lrge_amd/csrc/k_index.h (k_place_reduce / k_place_scan / k_place_apply / k_fill_tail through
place_table_launch: sizes around the lane, row and tile borders, the scan's second chunk of 1024 tiles, one displacement chain over every
border, sparse stretches beyond the LDS compose limit, a grid smaller than the tile count, run lengths at the count clamp and the
histogram's edges, every partial width of the hash with and without the power map, segment-packed streams, overflow by one slot), k_lookup
over every table that did not overflow, k_seed_counts and k_expand of lrge_amd/csrc/k_seed.h (list lengths and wave totals at the lane
count and the occurrence threshold, empty lists anywhere in a wave, windows off the wave grid, the name rules, tight key layouts) and
k_expand_q through expand_q_launch (every class at its compaction round's borders, both plane counts, four pair populations, mixed
launches).  tools/seed_check.hip (lrge_amd/_lib/libseed_check.so) includes the product's headers and goes through the product's own two
launch functions; inputs are synthetic arrays, no read set is sketched; every call also returns the stage's code and whether the guard
bands around its device buffers still hold their pattern.  tests/test_seed_ref.py proves on the CPU that these cases can tell near misses
apart.

Measured on one MI355X: the module's 108 tests take 15.2 s, the slowest of them 1.56 s (test_table_and_lookup[big-fused-inline-pairs]: 2 099 201
runs, a 69 MB table and 2.1 M lookups; its seven sister forms 1.3 s each); every other test stays below 0.25 s."""
import ctypes as C

import numpy as np
import pytest

import seed_ref as R

pytestmark = pytest.mark.gpu

LRGE_OK, LRGE_ERR_DEVICE, SC_ERR_HARNESS = 0, -5, -1000
V, U6, U3, I = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class ScSeed(C.Structure):
    _fields_ = [("qx", V), ("qy", V), ("n_mz", U6), ("hs", V), ("hc", V), ("hn", V), ("pos", V), ("n_pos", U6), ("t_len", V), ("t_rank", V), ("nt", U3),
                ("q_len", V), ("q_rank", V), ("nq", U3), ("qmz_off", V), ("aoff", V), ("krank", V), ("pk_pos1", U3), ("pk_ybits", U3),
                ("mid_occ", C.c_int32), ("check_names", C.c_int32), ("no_dual", C.c_int32), ("bits_rpos", U3), ("bits_rid", U3), ("bits_q", U3)]


class SeedLib:
    def __init__(self):
        from lrge_amd import build as Bd
        self.L = L = C.CDLL(Bd.build_seed_check())
        L.sc_last_error.restype = C.c_char_p
        L.sc_fix.restype, L.sc_fix.argtypes = U3, [I, U3]
        L.sc_seg_hash.restype, L.sc_seg_hash.argtypes = U6, [U6, U3, U3, U3]
        L.sc_table.argtypes = [V, V, V, U3, U6, I, U6, U6, U3, U3, I, U3, U3, V, U3, U3, U3, U3, V, V, V, V, V, V]
        L.sc_lookup.argtypes = [V, U6, C.c_int32, V, V, V, V]
        L.sc_counts.argtypes = [V, V, V, V]
        L.sc_expand.argtypes = [V, U6, U6, U3, U3, U6, V, V, V]
        L.sc_expand_q.argtypes = [V, U6, U6, U3, U3, U3, U3, U3, U3, U6, V, V, V]
        assert L.sc_init(256) == LRGE_OK, "no device"

    def _done(self, rc, g, want_rc=LRGE_OK):
        if rc == LRGE_ERR_DEVICE:       # a failed launch or a fault: nothing more is started on this device
            pytest.exit("device failure in libseed_check: %r" % self.L.sc_last_error(), returncode=3)
        assert rc == want_rc, (rc, self.L.sc_last_error())
        if want_rc == LRGE_OK:
            assert g.value == 1, "a guard band was written"

    def table(self, c, packed, inline, fused, seg=None):
        skey, ypos, kshift = c.stream(packed)
        ht = np.zeros(2 * c.n_slots, dtype=np.uint64)
        occ = np.zeros(c.max_bin + 1, dtype=np.uint32)
        ov, last, disp, g = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64), C.c_int(0)
        rc = self.L.sc_table(_p(R.u64(skey)), _p(ypos), _p(R.u32(c.starts)), c.n, c.M, int(c.sparse), c.cap, c.n_slots, kshift, self.L.sc_fix(c.k, c.pw),
                             int(fused), c.pk_pos1 if packed else 0, int(inline), _p(seg.seg_start) if seg else None, seg.e if seg else 0, c.nbits, c.max_bin, c.grid_cap,
                             _p(ht), _p(occ), _p(ov), _p(last), _p(disp), C.byref(g))
        self._done(rc, g)
        return ht, occ, int(ov[0]), int(last[0]), int(disp[0])

    def lookup(self, q_hash, mid_occ, with_hn=True, want_rc=LRGE_OK):
        qx = R.u64(R.u64(q_hash) << np.uint64(8) | np.uint64(19))
        hs, hc, hn, g = np.zeros(qx.size, dtype=np.uint64), np.zeros(qx.size, dtype=np.uint32), np.zeros(qx.size, dtype=np.uint32), C.c_int(0)
        self._done(self.L.sc_lookup(_p(qx), qx.size, mid_occ, _p(hs), _p(hc), _p(hn) if with_hn else None, C.byref(g)), g, want_rc)
        return hs, hc, hn

    def _seed(self, S, hn=None, aoff=None):
        keep = [R.u64(S.qx), R.u64(S.qy), R.u64(S.hs), R.u32(S.hc), None if hn is None else R.u32(hn), R.u64(S.pos), R.u32(S.t_len), R.u32(S.t_rank),
                R.u32(S.q_len), R.u32(S.q_rank), R.u32(S.qmz_off), None if aoff is None else R.u32(aoff), None if S.krank is None else R.u32(S.krank)]
        s = ScSeed(_p(keep[0]), _p(keep[1]), S.n_mz, _p(keep[2]), _p(keep[3]), _p(keep[4]), _p(keep[5]), keep[5].size, _p(keep[6]), _p(keep[7]), S.nt,
                   _p(keep[8]), _p(keep[9]), S.nq, _p(keep[10]), _p(keep[11]), _p(keep[12]), S.pk_pos1, S.pk_ybits, S.mid_occ, S.check_names, S.no_dual, 0, 0, 0)
        return s, keep

    def counts(self, S):
        s, keep = self._seed(S)
        hn, hv, g = np.zeros(S.n_mz, dtype=np.uint32), np.zeros(S.n_mz, dtype=np.uint32), C.c_int(0)
        self._done(self.L.sc_counts(C.byref(s), _p(hn), _p(hv), C.byref(g)), g)
        return hn, hv

    def expand(self, S, hn, aoff, b, e, q0, kl, bits_qy):
        s, keep = self._seed(S, hn, aoff)
        s.bits_rpos, s.bits_rid, s.bits_q = kl
        n_out = int(aoff[e]) - int(aoff[b])
        k, v, g = np.full(max(1, n_out), R.PATTERN64, dtype=np.uint64), np.full(max(1, n_out), R.PATTERN64, dtype=np.uint64), C.c_int(0)
        self._done(self.L.sc_expand(C.byref(s), b, e, q0, bits_qy, n_out, _p(k), _p(v), C.byref(g)), g)
        return k[:n_out], v[:n_out]

    def expand_q(self, c):
        s, keep = self._seed(c.S, c.hn, c.aoff)
        s.bits_rpos, s.bits_rid, s.bits_q = c.kl
        buf, kept, g = np.full(c.n_out, R.PATTERN64, dtype=np.uint64), np.full(c.nqb, 0xDEADBEEF, dtype=np.uint32), C.c_int(0)
        self._done(self.L.sc_expand_q(C.byref(s), c.mz_begin, c.mz_end, c.q0, c.nqb, c.smax, c.mmax, c.n_planes, c.bits_qy, c.n_out, _p(buf), _p(kept), C.byref(g)), g)
        return buf, kept


@pytest.fixture(scope="module")
def sc():
    s = SeedLib()
    yield s
    s.L.sc_shutdown()


def same(a, b, what=""):
    assert a.shape == b.shape and np.array_equal(a, b), what


def test_fix_word_of_the_header_holds_the_clamped_exponent(sc):
    for k in R.TABLE_K + (17, 20, 21):
        for pw in R.TABLE_PW + (2, 9, 10):
            part = (2 * k) % 8
            want = 0 if part == 0 else (64 - 8 * ((2 * k + 7) // 8)) | (8 - part) << 8 | R.clamp_power(k, pw) << 16
            assert sc.L.sc_fix(k, pw) == want, (k, pw)


# ------------------------------------------------------------------------------------------
# table and lookup
# ------------------------------------------------------------------------------------------
FORMS = [(fused, inline, packed) for fused in (True, False) for inline in (True, False) for packed in (False, True)]
FORM_IDS = ["%s-%s-%s" % ("fused" if f else "memset", "inline" if i else "lists", "packed" if p else "pairs") for f, i, p in FORMS]


def check_table(sc, c, packed, inline, fused, seg=None):
    img, hist, ov, last, disp = c.model(packed, inline, fused)
    ht, occ, d_ov, d_last, d_disp = sc.table(c, packed, inline, fused, seg)
    assert d_ov == ov, c.name
    same(occ, hist, c.name)
    if fused:
        assert d_last == last, c.name           # (clamped to the last slot when the placement overflows)
    if ov:
        # nothing of an overflowed table is specified but the flag (and that nothing was written outside it: the bands); no lookup is
        # ever run on it -- the harness refuses, its probes would have no end
        sc.lookup(c.keys[:1], 2, want_rc=SC_ERR_HARNESS)
        return
    assert d_disp == disp, c.name
    bad = np.flatnonzero(ht != img)
    assert bad.size == 0, (c.name, "first differing word %d (slot %d) of %d" % (bad[0], bad[0] // 2, bad.size))
    assert ht[-2] == R.HT_EMPTY and ht[-1] == R.HT_EMPTY, "the last slot stays empty"
    # lookups: every present key, then absent ones below, above and between; hn around the threshold (run lengths 1, 2, 3)
    q = np.concatenate([c.keys, c.absent()])
    for mid, with_hn in ((2, True), (1, True), (2, False)):
        hs, hc, hn = sc.lookup(q, mid, with_hn)
        w_hs, w_hc, w_hn = c.lookup(packed, inline, q, mid)
        same(hs, w_hs, c.name); same(hc, w_hc, c.name)
        if with_hn:
            same(hn, w_hn, c.name)
    for n_mz in (1, 255, 256, 257):
        qq = np.resize(q[::-1], n_mz)
        hs, hc, hn = sc.lookup(qq, 2)
        w = c.lookup(packed, inline, qq, 2)
        same(hs, w[0]); same(hc, w[1]); same(hn, w[2])


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("family", R.TABLE_FAMILIES)
def test_table_and_lookup(sc, family, form):
    fused, inline, packed = form
    for c in R.table_cases(family):
        check_table(sc, c, packed, inline, fused)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "memset"])
@pytest.mark.parametrize("inline", [True, False], ids=["inline", "lists"])
def test_table_of_a_segment_packed_stream(sc, inline, fused):
    for c in R.seg_cases():
        # the harness's seg_hash is the model's: the segment's number on top of the stored bits, as a hash
        for r in (0, c.n // 2, c.n - 1):
            s = int(c.sigs[r])
            assert sc.L.sc_seg_hash(s & R.mask(c.nr), s >> c.nr, c.e, c.nbits) == int(c.keys[r])
        check_table(sc, c, True, inline, fused, seg=c)


# ------------------------------------------------------------------------------------------
# counts and expansion
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.SEED_FAMILIES)
def test_counts_and_expansion(sc, family):
    for c in R.seed_cases(family):
        t = c.truth()
        hn, hv = sc.counts(c.S)
        same(hn, t[0], c.name); same(hv, t[1], c.name)
        aoff = R.scan0(t[1])
        k, v = sc.expand(c.S, t[0], aoff, c.b, c.e, c.q0, c.kl, c.bits_qy)
        assert k.size == int(hv[c.b:c.e].sum()), "as many anchors as the counts say"
        same(k, t[2], c.name)
        if c.bits_qy == 0:
            same(v, t[3], c.name)
        if c.S.krank is not None and c.bits_qy == 0:      # the same launch without ranks: the rank field stays zero
            kr, c.S.krank = c.S.krank, None
            try:
                k0, v0 = sc.expand(c.S, t[0], aoff, c.b, c.e, c.q0, c.kl, 0)
            finally:
                c.S.krank = kr
            same(k0, t[2], c.name); same(v0, t[3] & np.uint64(R.mask(44)), c.name)


# ------------------------------------------------------------------------------------------
# k_expand_q
# ------------------------------------------------------------------------------------------
def check_expand_q(sc, c):
    want, want_kept = c.truth()
    buf, kept = sc.expand_q(c)
    same(kept, want_kept, c.name)
    m = c.specified(kept)
    bad = np.flatnonzero((buf != want) & m)
    assert bad.size == 0, (c.name, "first differing word %d of %d" % (bad[0], bad.size))
    # independently of the hash: every pair with at least n_planes anchors survives whole and in order
    sb = c.kl[0] + 1 + c.kl[1]
    pair = lambda w: (w & np.uint64(R.mask(sb))) >> np.uint64(c.kl[0])
    for q in range(c.q0, c.q0 + c.nqb):
        e = c.emitted(q)
        if e.size == 0:
            continue
        seg0 = int(c.aoff[c.S.qmz_off[q]]) - int(c.aoff[c.mz_begin])
        got = buf[seg0:seg0 + int(kept[q - c.q0])]
        pr, n = np.unique(pair(e), return_counts=True)
        big = pr[n >= c.n_planes]
        same(got[np.isin(pair(got), big)], e[np.isin(pair(e), big)], c.name)


@pytest.mark.parametrize("population", R.EXPQ_POPULATIONS)
@pytest.mark.parametrize("n_planes", [2, 3])
@pytest.mark.parametrize("cls", [0, 1, 2], ids=["256x14", "512x16", "1024x17"])
def test_expand_q_classes_at_their_round_borders(sc, cls, n_planes, population):
    for c in R.expq_cases(cls, n_planes, population):
        check_expand_q(sc, c)


@pytest.mark.parametrize("n_planes", [2, 3])
def test_expand_q_mixed_launch(sc, n_planes):
    check_expand_q(sc, R.expq_mixed_case(n_planes))
