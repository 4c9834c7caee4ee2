"""The primitives of lrge_amd/csrc/k_prims.h against the plain models of tests/prims_ref.py, bit for bit, on the device: the exclusive scan
(both levels, the vector and the scalar branches, k_scan_small's carry loop), radix_sort_pairs / radix_sort_keys (sizes around the tile and
the XCD map, partial top digits, both digit orders, pass ranges, with and without next-pass digit bytes), the first pass from slots (descriptor,
LDS-cached offsets, per-entry search), the packed segmented sort beside all three k_seg_sort_local variants, the segment-packed index sort (index_sort_seg: pairs, dense SEGW
entries and wave-dense slots give the same words and segment starts), and the run heads with forced boundaries.  tools/prims_check.hip (lrge_amd/_lib/libprims_check.so) includes the product's header and launches exactly what the product
launches; values are input positions, so stability shows; every call also returns the primitive's code and whether the guard bands around
its device buffers still hold their pattern.  tests/test_prims_ref.py proves on the CPU that these cases can tell near misses apart.

Measured on one MI355X: the module's 71 tests take 3.1 s, the slowest of them 0.26 s (test_whole_sorts[sizes]; the two 134 MB scans 0.17 s each;
the 18 index sort tests 0.5 s together, the slowest of those 0.14 s, test_index_sort[layouts])."""
import ctypes as C
import functools

import numpy as np
import pytest

import prims_ref as R

pytestmark = pytest.mark.gpu

LRGE_OK, LRGE_ERR_DEVICE, LRGE_ERR_INVALID = 0, -5, -9
PATTERN32 = 0xA5A5A5A5


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Prims:
    def __init__(self):
        from lrge_amd import build as Bd
        self.L = L = C.CDLL(Bd.build_prims_check())
        L.pc_last_error.restype = C.c_char_p
        for f in (L.pc_hash_to_sig, L.pc_sig_to_hash):
            f.restype, f.argtypes = C.c_uint64, [C.c_uint64, C.c_uint32]
        V, U6, U3, I, S = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_char_p
        L.pc_scan.argtypes = [V, U6, U3, U3, I, I, I, V, V, V]
        L.pc_scan_small.argtypes = [V, U3, I, V, V]
        L.pc_sort_pairs.argtypes = [V, V, U6, I, I, I, I, I, U3, U3, V, V, V]
        L.pc_sort_keys.argtypes = [V, U6, I, I, I, I, I, S, U3, U3, V, V]
        L.pc_sort_keys_from_slots.argtypes = [V, V, U3, U3, U6, I, I, I, I, S, V, V]
        L.pc_anchor_sort.argtypes = [V, U6, U6, I, U3, U3, U3, V, V, V, U3, U6, I, S, V, V, V]
        L.pc_heads.argtypes = [V, U6, U3, V, U3, I, V, V, V]
        L.pc_index_sort.argtypes = [I, V, V, V, V, V, U3, U3, U6, I, U3, U3, U3, S, V, V, V]
        m = C.c_int(0)
        assert L.pc_init(C.byref(m)) == LRGE_OK, "no device"
        self.lsort_mask = m.value

    def _done(self, rc, g, want_rc=LRGE_OK):
        if rc == LRGE_ERR_DEVICE:       # a failed launch or a fault: nothing more is started on this device
            pytest.exit("device failure in libprims_check: %r" % self.L.pc_last_error(), returncode=3)
        assert rc == want_rc, (rc, self.L.pc_last_error())
        assert g.value == 1, "a guard band was written"

    def scan(self, a, in_off=0, out_off=0, inplace=False, total_mode=1, bs_mode=0, want_rc=LRGE_OK):
        a = np.ascontiguousarray(a, dtype=np.uint32)
        out, tot, g = np.zeros(max(1, a.size), dtype=np.uint32), np.full(1, 0xDEADBEEF, dtype=np.uint32), C.c_int(0)
        rc = self.L.pc_scan(_p(a), a.size, in_off, out_off, int(inplace), total_mode, bs_mode, _p(out), _p(tot), C.byref(g))
        self._done(rc, g, want_rc)
        return out[:a.size], int(tot[0])

    def scan_small(self, a, with_total):
        d = np.ascontiguousarray(a, dtype=np.uint32).copy()
        tot, g = np.zeros(1, dtype=np.uint32), C.c_int(0)
        self._done(self.L.pc_scan_small(_p(d), d.size, int(with_total), _p(tot), C.byref(g)), g)
        return d, int(tot[0])

    def sort_pairs(self, k, v, b, nb, rev, pb=0, pe=-1, off0=0, off1=0):
        k, v = R.u64(k), R.u64(v)
        ok, ov, g = np.zeros(max(1, k.size), dtype=np.uint64), np.zeros(max(1, k.size), dtype=np.uint64), C.c_int(0)
        self._done(self.L.pc_sort_pairs(_p(k), _p(v), k.size, b, nb, int(rev), pb, pe, off0, off1, _p(ok), _p(ov), C.byref(g)), g)
        return ok[:k.size], ov[:k.size]

    def sort_keys(self, k, b, nb, rev, pb=0, pe=-1, opts=None, off0=0, off1=0):
        k = R.u64(k)
        out, g = np.zeros(max(1, k.size), dtype=np.uint64), C.c_int(0)
        self._done(self.L.pc_sort_keys(_p(k), k.size, b, nb, int(rev), pb, pe, opts, off0, off1, _p(out), C.byref(g)), g)
        return out[:k.size]

    def from_slots(self, slots, counts, cap, b, nb, rev, rest, opts=None):
        counts = np.asarray(counts, dtype=np.uint64)
        offs = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint32)
        n = int(counts.sum())
        out, g = np.zeros(max(1, n), dtype=np.uint64), C.c_int(0)
        self._done(self.L.pc_sort_keys_from_slots(_p(R.u64(slots)), _p(offs), counts.size, cap, n, b, nb, int(rev), int(rest), opts, _p(out), C.byref(g)), g)
        return out[:n]

    def anchor_sort(self, pk, n_out, nbits, local, tiles, n_local, src_first=False, opts=None):
        sb, bits_qy, sh_q = R.seg_payload_bits(nbits)
        segs = np.ascontiguousarray(np.concatenate([x.reshape(-1) for x in local]), dtype=np.uint32) if sum(x.size for x in local) else np.zeros(4, dtype=np.uint32)
        n_segs = np.array([x.shape[0] for x in local], dtype=np.uint32)
        tl = np.ascontiguousarray(tiles.reshape(-1), dtype=np.uint32) if tiles.size else np.zeros(8, dtype=np.uint32)
        ok, ov, g = np.zeros(max(1, n_out), dtype=np.uint64), np.zeros(max(1, n_out), dtype=np.uint64), C.c_int(0)
        rc = self.L.pc_anchor_sort(_p(R.u64(pk)), pk.size, n_out, nbits, sb, bits_qy, sh_q, _p(segs), _p(n_segs), _p(tl), tiles.shape[0], n_out - n_local,
                                   int(src_first), opts, _p(ok), _p(ov), C.byref(g))
        self._done(rc, g)
        return ok[:n_out], ov[:n_out]

    def index_sort(self, form, n, nbits, ybits, pos1, e, x, y=None, dig=None, counts=None, cap=0, opts=None):
        x = R.u64(x)
        y = None if y is None else R.u64(y)
        dig = None if dig is None else np.ascontiguousarray(dig, dtype=np.uint32)
        offs = None
        if counts is not None:
            counts = np.ascontiguousarray(counts, dtype=np.uint32)
            offs = np.concatenate([[0], np.cumsum(counts.astype(np.uint64))[:-1]]).astype(np.uint32)
        words, starts, g = np.zeros(n, dtype=np.uint64), np.zeros((256 << e) + 1, dtype=np.uint32), C.c_int(0)
        rc = self.L.pc_index_sort(form, _p(x), _p(y), _p(dig), _p(counts), _p(offs), 0 if counts is None else counts.size, cap, n, nbits, ybits, pos1, e, opts,
                                  _p(words), _p(starts), C.byref(g))
        self._done(rc, g)
        return words, starts

    def heads(self, keys, shift, forced=None, use_async=False):
        keys = R.u64(keys)
        st, nh, g = np.zeros(keys.size + 1, dtype=np.uint32), np.zeros(1, dtype=np.uint32), C.c_int(0)
        f = None if forced is None else np.ascontiguousarray(forced, dtype=np.uint32)
        self._done(self.L.pc_heads(_p(keys), keys.size, shift, _p(f), 0 if f is None else f.size - 1, int(use_async), _p(st), _p(nh), C.byref(g)), g)
        assert nh[0] <= keys.size
        return st[:int(nh[0])]


@pytest.fixture(scope="module")
def pc():
    p = Prims()
    yield p
    p.L.pc_shutdown()


def same(a, b, what=""):
    assert a.shape == b.shape and np.array_equal(a, b), what


def test_the_device_takes_all_three_lds_sort_variants(pc):
    assert pc.lsort_mask == 7, "k_seg_sort_local variants refused by the device: mask %d" % pc.lsort_mask


def test_significance_string_of_the_header_is_the_bytewise_one(pc):
    for nbits in R.SIG_NBITS:
        rng = np.random.Generator(np.random.PCG64(nbits))
        for h in [0, 1, R.mask(nbits)] + [int(x) & R.mask(nbits) for x in rng.integers(0, 1 << 63, 300)]:
            s = pc.L.pc_hash_to_sig(h, nbits)
            assert s == R.hash_to_sig(h, nbits) and pc.L.pc_sig_to_hash(s, nbits) == h


# ------------------------------------------------------------------------------------------
# scan
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SCAN_SMALL_N)
def test_scan_small_sizes(pc, n):
    for fill in R.SCAN_FILLS:
        a = R.scan_input(n, fill)
        want, total = R.scan_exclusive(a)
        if fill == "max_total" and n:
            assert total == (1 << 32) - 1
        # in place at every input misalignment; apart, the same and an output shifted off an aligned input
        layouts = [(True, o, 0) for o in range(4)] + [(False, o, 0) for o in range(4)] + [(False, 0, 1), (False, 3, 1)]
        for inplace, in_off, out_off in layouts:
            for total_mode in (0, 1, 2):        # null, a word of its own, the word directly behind the output
                out, tot = pc.scan(a, in_off, out_off, inplace, total_mode)
                same(out, want, (n, fill, inplace, in_off, out_off, total_mode))
                assert tot == (total if total_mode else 0xDEADBEEF)


@functools.lru_cache(maxsize=None)
def _big(n):
    a = R.scan_input(n, "big")
    return a, R.scan_exclusive(a)


@pytest.mark.parametrize("n", R.SCAN_BIG_N)
def test_scan_last_single_level_and_first_two_level_size(pc, n):
    a, (want, total) = _big(n)
    out, tot = pc.scan(a)
    same(out, want)
    assert tot == total


def test_scan_with_the_callers_block_sums(pc):
    n = R.SCAN_GROUP * R.SCAN_TILE                      # 8192 tiles: accepted
    a, (want, total) = _big(n)
    out, tot = pc.scan(a, bs_mode=1)
    same(out, want)
    assert tot == total
    for m in (1, 4097):
        b = R.scan_input(m, "random")
        same(pc.scan(b, bs_mode=1)[0], R.scan_exclusive(b)[0])
    a1, _ = _big(n + 1)                                 # 8193 tiles: refused before any launch
    out, tot = pc.scan(a1, bs_mode=1, want_rc=LRGE_ERR_INVALID)
    assert (out == PATTERN32).all() and tot == PATTERN32


@pytest.mark.parametrize("n", R.SS_N)
def test_scan_small_kernel_alone(pc, n):
    for fill in ("random", "ends", "max_total"):
        a = R.scan_input(n, fill, seed=3)
        want, total = R.scan_exclusive(a)
        for with_total in (False, True):
            out, tot = pc.scan_small(a, with_total)
            same(out, want, (n, fill))
            assert tot == (total if with_total else PATTERN32)


# ------------------------------------------------------------------------------------------
# whole and partial sorts
# ------------------------------------------------------------------------------------------
def _check_sorts(pc, keys, b, nb, rev, pb, pe, perm_keys, perm_pairs, what, offs=(0, 0)):
    vals = np.arange(keys.size, dtype=np.uint64)
    got = pc.sort_keys(keys, b, nb, rev, pb, pe, None, *offs)
    same(got, keys[perm_keys], ("keys",) + what)
    same(pc.sort_keys(keys, b, nb, rev, pb, pe, b"NO_DIGIT_BYTES", *offs), got, ("keys, no digit bytes",) + what)
    k, v = pc.sort_pairs(keys, vals, b, nb, rev, pb, pe, *offs)
    same(v, perm_pairs.astype(np.uint64), ("pair values",) + what)
    same(k, keys[perm_pairs], ("pair keys",) + what)


@pytest.mark.parametrize("group", R.SORT_GROUPS)
def test_whole_sorts(pc, group):
    for i, case in enumerate(R.sort_cases(group)):
        kind, n, b, nb, rev = case
        keys = R.sort_keys_of(kind, n, b, nb)
        offs = (1, 3) if i % 4 == 3 else (0, 0)         # buffers 8 and 24 bytes off their alignment
        _check_sorts(pc, keys, b, nb, rev, 0, -1, R.sort_whole(keys, b, nb, rev, False), R.sort_whole(keys, b, nb, rev, True), case, offs)


def test_pass_ranges(pc):
    for case in R.range_cases():
        n, b, nb, rev, pb, pe = case
        keys = R.sort_keys_of("third_repeated", n, b, nb)
        _check_sorts(pc, keys, b, nb, rev, pb, pe, R.sort_passes(keys, b, nb, rev, False, pb, pe), R.sort_passes(keys, b, nb, rev, True, pb, pe), case)


@pytest.mark.parametrize("table", R.slot_tables(), ids=lambda t: t[0])
def test_first_pass_from_slots(pc, table):
    name, cap, counts = table
    n = int(counts.sum())
    for b, nb in ((0, 30), (0, 9)):
        dense = R.sort_keys_of("third_repeated", n, b, nb)
        slots = R.slots_fill(cap, counts, dense)
        for rev in (False, True):
            first = pc.from_slots(slots, counts, cap, b, nb, rev, rest=False)
            same(first, dense[R.sort_passes(dense, b, nb, rev, False, 0, 1)], (name, b, nb, rev, "first pass"))
            whole = dense[R.sort_whole(dense, b, nb, rev, False)]
            same(pc.from_slots(slots, counts, cap, b, nb, rev, rest=True), whole, (name, b, nb, rev, "whole"))
            same(pc.from_slots(slots, counts, cap, b, nb, rev, rest=True, opts=b"NO_DIGIT_BYTES"), whole, (name, b, nb, rev, "whole, no digit bytes"))


# ------------------------------------------------------------------------------------------
# packed anchors: the tiled segmented sort and the three LDS variants
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits", R.SEG_NBITS)
def test_anchor_sorts_agree(pc, nbits):
    assert pc.lsort_mask == 7
    sb, bits_qy, sh_q = R.seg_payload_bits(nbits)
    n_out = sum(R.SEG_LENS)
    for kind in R.SEG_KINDS:
        pk, segs = R.seg_words(kind, R.SEG_LENS, nbits)
        want_k, want_v = R.anchor_sort(pk, segs, nbits, sb, bits_qy, sh_q)
        for v in range(3):      # every segment through every variant that holds it; the longer ones tiled behind them (delta != 0)
            local, tiles, n_local = R.plan_anchor_sort(segs, lambda c: v if c <= R.LSORT_CAP[v] else None)
            k, val = pc.anchor_sort(pk, n_out, nbits, local, tiles, n_local)
            same(k, want_k, (kind, "variant", v, "keys")); same(val, want_v, (kind, "variant", v, "values"))
        local, tiles, n_local = R.plan_anchor_sort(segs, lambda c: None)         # all tiled
        for opts in (None, b"NO_DIGIT_BYTES"):
            k, val = pc.anchor_sort(pk, n_out, nbits, local, tiles, n_local, opts=opts)
            same(k, want_k, (kind, "tiled", opts, "keys")); same(val, want_v, (kind, "tiled", opts, "values"))
        # the sparse layout of the dead-pair filter: every segment read from its slot, classes as the product picks them
        pk, segs = R.seg_words(kind, R.SEG_LENS, nbits, slack=5)
        want_k, want_v = R.anchor_sort(pk, segs, nbits, sb, bits_qy, sh_q)
        local, tiles, n_local = R.plan_anchor_sort(segs, lambda c: 0 if c <= 2048 else 1 if c <= 8192 and c % 2 else None)
        k, val = pc.anchor_sort(pk, n_out, nbits, local, tiles, n_local, src_first=True)
        same(k, want_k, (kind, "sparse keys")); same(val, want_v, (kind, "sparse values"))


# ------------------------------------------------------------------------------------------
# the segment-packed index sort: pairs, dense SEGW entries and wave-dense slots, with and without next-pass digit bytes
# ------------------------------------------------------------------------------------------
def _check_index_sort(pc, h, y, nbits, ybits, pos1, e, cap, counts, what):
    n = h.size
    want_w, want_s = R.index_sort(h, y, nbits, ybits, pos1, e)
    (_, _), (w, d), (sw, sd, cnt) = R.index_forms(h, y, nbits, ybits, pos1, cap, counts)
    for opts in (None, b"NO_DIGIT_BYTES"):
        for form, got in (("pairs", pc.index_sort(0, n, nbits, ybits, pos1, e, h, y=y, opts=opts)),
                          ("segw", pc.index_sort(1, n, nbits, ybits, pos1, e, w, dig=d, opts=opts)),
                          ("wave", pc.index_sort(2, n, nbits, ybits, pos1, e, sw, dig=sd, counts=cnt, cap=cap, opts=opts))):
            same(got[0], want_w, what + (form, opts, "words"))
            same(got[1], want_s, what + (form, opts, "segment starts"))


@pytest.mark.parametrize("group", R.INDEX_GROUPS)
def test_index_sort(pc, group):
    for case in R.index_cases(group):
        kind, n, nbits, e, tight = case
        ybits, pos1 = R.index_layout(nbits, e, tight)
        h, y = R.index_entries(kind, n, nbits, ybits, pos1, e)
        _check_index_sort(pc, h, y, nbits, ybits, pos1, e, *R.wave_table_for(n), case)


@pytest.mark.parametrize("table", R.index_slot_tables(), ids=lambda t: t[0])
def test_index_sort_from_the_slot_tables(pc, table):
    name, cap, counts = table
    n = int(counts.sum())
    for nbits, e, tight in ((30, 0, False), (38, 6, True)):
        ybits, pos1 = R.index_layout(nbits, e, tight)
        h, y = R.index_entries("uniform", n, nbits, ybits, pos1, e)
        _check_index_sort(pc, h, y, nbits, ybits, pos1, e, cap, counts, (name, nbits, e))


# ------------------------------------------------------------------------------------------
# run heads
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.HEAD_STREAMS)
def test_run_heads(pc, kind):
    for n in R.HEAD_N:
        for shift in R.HEAD_SHIFTS:
            keys = R.head_stream(kind, n, shift)
            want = R.heads(keys, shift)
            same(pc.heads(keys, shift), want, (kind, n, shift))
            same(pc.heads(keys, shift, use_async=True), want, (kind, n, shift, "async"))
            for n_seg in (256, 2048):
                forced = R.head_boundaries(keys, shift, n_seg)
                same(pc.heads(keys, shift, forced), R.heads(keys, shift, forced), (kind, n, shift, n_seg))
