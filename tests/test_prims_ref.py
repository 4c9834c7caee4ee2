"""The case families of tests/prims_ref.py can tell a right primitive from a plausibly wrong one (no GPU): for every family that
tests/test_gpu_prims.py runs against lrge_amd/csrc/k_prims.h, the model's answer is computed together with the answers of named near-miss
models -- an unstable sort, the other digit mask, a lost carry, a forgotten head ... -- and at least one case of the family must separate
each near miss from the truth.  Also: the per-pass sort model over all passes is the composed-key model, the paths of the slot reader
are all reached by the chunk tables, the index sort model is the plain sort of the significance strings, and hash_to_sig / sig_to_hash
are inverse."""
import numpy as np
import pytest

import prims_ref as R


def separated(cases, truth, wrong):
    """number of cases on which the two models differ"""
    n = 0
    for c in cases:
        a, b = truth(c), wrong(c)
        a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
        if any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(a, b)):
            n += 1
    return n


# ---- scan ----
@pytest.mark.parametrize("miss", ["inclusive", "no_tile_carry"])
def test_scan_cases_separate(miss):
    cases = [(n, f) for n in R.SCAN_SMALL_N for f in R.SCAN_FILLS]
    assert separated(cases, lambda c: R.scan_exclusive(R.scan_input(*c))[0], lambda c: R.scan_exclusive(R.scan_input(*c), miss)[0]) > 0


def test_scan_two_level_case_separates_a_lost_group_carry():
    # only the first two-level size can: item 33 554 432 is the first of the second group of 8192 tiles
    lo, hi = (R.scan_input(n, "big") for n in R.SCAN_BIG_N)
    assert np.array_equal(R.scan_exclusive(lo)[0], R.scan_exclusive(lo, "no_group_carry")[0])
    t, w = R.scan_exclusive(hi)[0], R.scan_exclusive(hi, "no_group_carry")[0]
    assert not np.array_equal(t, w) and np.array_equal(t[:-1], w[:-1])


def test_scan_fills_are_what_they_say():
    for n in R.SCAN_SMALL_N:
        if n:
            assert int(R.scan_input(n, "max_total").astype(np.uint64).sum()) == (1 << 32) - 1
            e = R.scan_input(n, "ends")
            assert e[0] and e[-1] and (n <= 2 or not e[1:-1].any())
    for n in R.SCAN_BIG_N:
        assert int(R.scan_input(n, "big").max()) <= 3


# ---- sorts ----
ALL_SORT_CASES = [c for g in R.SORT_GROUPS for c in R.sort_cases(g)]


def _perm(case, whole_bytes, miss=None):
    kind, n, b, nb, rev = case
    return R.sort_whole(R.sort_keys_of(kind, n, b, nb), b, nb, rev, whole_bytes, miss)


@pytest.mark.parametrize("whole_bytes", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("miss", R.SORT_MISSES)
def test_sort_cases_separate(miss, whole_bytes):
    for g in R.SORT_GROUPS:         # every group on its own: each is one GPU test
        if g == "sizes" and miss == "other_mask" and whole_bytes:
            continue                # (its bit ranges leave the pair sort's extra bits empty or absent; the other two groups have them)
        assert separated(R.sort_cases(g), lambda c: _perm(c, whole_bytes), lambda c: _perm(c, whole_bytes, miss)) > 0, g


def test_keys_above_the_field_stay_put_under_the_partial_mask_and_move_under_whole_bytes():
    seen = 0
    for case in R.sort_cases("bits"):
        kind, n, b, nb, rev = case
        if kind != "differ_above":
            continue
        assert np.array_equal(_perm(case, False), np.arange(n)), case
        if nb % 8 and b + nb < 64:
            assert not np.array_equal(_perm(case, True), np.arange(n)), case
            seen += 1
    assert seen >= 8


@pytest.mark.parametrize("whole_bytes", [False, True], ids=["keys", "pairs"])
def test_pass_model_over_all_passes_is_the_composed_key_model(whole_bytes):
    for case in ALL_SORT_CASES:
        kind, n, b, nb, rev = case
        if n > 3 * 4096:
            continue
        keys = R.sort_keys_of(kind, n, b, nb)
        assert np.array_equal(R.sort_passes(keys, b, nb, rev, whole_bytes), R.sort_whole(keys, b, nb, rev, whole_bytes)), case


def _range_perm(case, whole_bytes, miss=None):
    n, b, nb, rev, pb, pe = case
    return R.sort_passes(R.sort_keys_of("third_repeated", n, b, nb), b, nb, rev, whole_bytes, pb, pe, miss)


@pytest.mark.parametrize("whole_bytes", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("miss", R.RANGE_MISSES + ("unstable", "digits_not_reversed", "other_mask"))
def test_range_cases_separate(miss, whole_bytes):
    assert separated(R.range_cases(), lambda c: _range_perm(c, whole_bytes), lambda c: _range_perm(c, whole_bytes, miss)) > 0


def test_sort_sizes_cover_every_tile_count_around_the_xcd_map():
    tiles = {(n + R.RS_TILE - 1) // R.RS_TILE for n in R.SORT_N}
    assert set(range(0, 18)) <= tiles and 66 in tiles


# ---- slots ----
def test_slot_tables_reach_every_path_and_separate_the_wrong_chunk():
    SLOT_LDS = 384
    names = set()
    for name, cap, counts in R.slot_tables():
        total = int(counts.sum())
        dense = R.sort_keys_of("uniform", total, 0, 30)
        slots = R.slots_fill(cap, counts, dense)
        assert np.array_equal(R.slots_dense(slots, counts, cap), dense)
        assert not np.array_equal(R.slots_dense(slots, counts, cap, "first_chunk_of_equal_offsets"), dense), name
        assert counts[0] == 0 and counts[-1] == 0 and total % R.RS_TILE == int(name[-1])
        z = "".join("0" if c == 0 else "1" for c in counts).strip("0")
        assert "00" in z, name                              # a run of empty chunks in the middle
        spans = R.slot_tile_spans(cap, counts)
        if name.startswith("cap8"):
            assert max(spans) > SLOT_LDS - 2                # the per-entry search
        elif name.startswith("cap64"):
            assert 6 < max(spans) <= SLOT_LDS - 2 and cap < 1024      # offsets cached in LDS (no descriptor below cap 1024)
        else:
            assert cap >= 1024 and min(spans[:-1] if total % R.RS_TILE else spans) <= 6 < max(spans), (name, spans)     # the descriptor, and its fall-back past six slots
        names.add(name[:-2])
    assert any(7 in R.slot_tile_spans(cap, counts) for name, cap, counts in R.slot_tables() if "seventh" in name)
    assert len(names) == 6


# ---- packed anchors ----
@pytest.mark.parametrize("miss", ["unstable", "swap_shq_sb"])
def test_anchor_cases_separate(miss):
    n = 0
    for nbits in R.SEG_NBITS:
        sb, bits_qy, sh_q = R.seg_payload_bits(nbits)
        assert sb + bits_qy + 9 == 64
        for kind in R.SEG_KINDS:
            pk, segs = R.seg_words(kind, R.SEG_LENS[:8], nbits)
            t, w = R.anchor_sort(pk, segs, nbits, sb, bits_qy, sh_q), R.anchor_sort(pk, segs, nbits, sb, bits_qy, sh_q, miss)
            n += not (np.array_equal(t[0], w[0]) and np.array_equal(t[1], w[1]))
    assert n > 0


def test_anchor_words_use_the_whole_payload_and_the_plan_has_every_shape():
    for nbits in R.SEG_NBITS:
        pk, segs = R.seg_words("uniform", R.SEG_LENS, nbits)
        assert int(np.bitwise_or.reduce(pk)) == R.M64 and int(np.bitwise_and.reduce(pk)) == 0       # self, span and qpos up to the top
    pk, segs = R.seg_words("uniform", R.SEG_LENS, 17, slack=3)
    assert [s for s, _, _ in segs][1] == R.SEG_LENS[0] + 3
    for v in range(3):
        loc, tiles, n_local = R.plan_anchor_sort(segs, lambda c: v if c <= R.LSORT_CAP[v] else None)
        assert loc[v].shape[0] == sum(1 for c in R.SEG_LENS if c <= R.LSORT_CAP[v]) and n_local == sum(c for c in R.SEG_LENS if c <= R.LSORT_CAP[v])
        if v < 2:
            assert tiles.shape[0] and tiles[:, 5].min() > 0                          # mixed: local segments in front, delta != 0
            assert (tiles[:, 6] != tiles[:, 0]).any()                                # sparse: src differs from start
    loc, tiles, n_local = R.plan_anchor_sort(segs, lambda c: None)
    assert n_local == 0 and tiles.shape[0] == sum((c + 4095) // 4096 for c in R.SEG_LENS) and not tiles[:, 5].any()
    # the lengths fill each variant exactly, one short and one over
    for cap in R.LSORT_CAP:
        assert {cap - 1, cap} <= set(R.SEG_LENS) and (cap + 1 in R.SEG_LENS or cap == 16384)


# ---- the segment-packed index sort ----
def _index_sort(case, miss=None):
    kind, n, nbits, e, tight = case
    ybits, pos1 = R.index_layout(nbits, e, tight)
    h, y = R.index_entries(kind, n, nbits, ybits, pos1, e)
    return R.index_sort(h, y, nbits, ybits, pos1, e, miss)


ALL_INDEX_CASES = [c for g in R.INDEX_GROUPS for c in R.index_cases(g)]


@pytest.mark.parametrize("miss", R.INDEX_SORT_MISSES)
def test_index_sort_cases_separate(miss):
    # the groups that must tell the near miss from the truth on their own (each is one GPU test): the rest of them hold no case that could
    groups = {"unstable": ("all_equal", "a2_bits_only", "below_a2_only", "sizes"), "a2_low_bits": ("layouts", "uniform", "a2_bits_only", "below_a2_only"),
              "e_minus_1": ("layouts", "sizes", "uniform", "a2_bits_only")}.get(miss, R.INDEX_GROUPS)
    for g in groups:
        assert separated(R.index_cases(g), _index_sort, lambda c: _index_sort(c, miss)) > 0, g


def test_index_sort_cases_are_what_they_say():
    for g in R.INDEX_GROUPS:
        for kind, n, nbits, e, tight in R.index_cases(g):
            nr = nbits - 8 - e
            ybits, pos1 = R.index_layout(nbits, e, tight)
            assert nr >= 1 and nbits - 16 >= 8 and nr + ybits <= 64 and (nr + ybits == 64) == tight and pos1 < 32 and ybits - pos1 <= 32
            h, y = R.index_entries(kind, n, nbits, ybits, pos1, e)
            assert h.size == n and int(h.max()) <= R.mask(nbits)
            S = R.sig_of(h, nbits)
            segs = np.unique(R.shr(S, nr)).size
            if kind == "one_b0":
                assert np.unique(h & R.U64(0xff)).size == 1 and np.unique(h).size > n // 2
            if kind == "one_per_segment":
                assert n < 256 and np.unique(h & R.U64(0xff)).size == n
            if kind == "all_equal":
                assert segs == 1 and np.unique(h).size == 1
            if kind == "a2_bits_only":
                assert segs == min(n, 1 << e) and np.unique(S & R.U64(R.mask(nr))).size == 1
            if kind == "below_a2_only":
                assert segs == 1 and np.unique(h).size == 1 << (8 - e)
            # the positions hold the input index, and the read numbers reach their top bit
            rid, low = R.y_fields(y, pos1)
            assert np.array_equal((rid & R.U64(31)) << R.U64(pos1) | low, np.arange(n, dtype=np.uint64))
            assert n < 64 or int(rid.max()) >> (ybits - pos1 - 1) == 1
    assert {c[1] for c in ALL_INDEX_CASES} >= set(R.INDEX_N) and {c[2] for c in ALL_INDEX_CASES} == set(R.INDEX_NBITS) and {c[3] for c in ALL_INDEX_CASES} == set(R.INDEX_E)


def test_index_sort_model_is_the_plain_sort_of_the_strings():
    for case in R.index_cases("layouts") + R.index_cases("all_equal"):
        kind, n, nbits, e, tight = case
        ybits, pos1 = R.index_layout(nbits, e, tight)
        h, y = R.index_entries(kind, n, nbits, ybits, pos1, e)
        assert np.array_equal(R.sig_of(h[:200], nbits), np.array([R.hash_to_sig(int(v), nbits) for v in h[:200]], dtype=np.uint64))
        words, starts = R.index_sort(h, y, nbits, ybits, pos1, e)
        ent = sorted((R.hash_to_sig(int(a), nbits), i, int(b)) for i, (a, b) in enumerate(zip(h[:600], y[:600])))      # ties: input order
        w600, s600 = R.index_sort(h[:600], y[:600], nbits, ybits, pos1, e)
        nr = nbits - 8 - e
        assert [int(v) for v in w600] == [(S & R.mask(nr)) << ybits | (b >> 32) << pos1 | (b & R.mask(pos1)) for S, _, b in ent]
        if e <= 1:                                      # (a quadratic count: the small tables only)
            assert [int(v) for v in s600] == [sum(1 for S, _, _ in ent if S >> nr < s) for s in range(256 << e)] + [600]
        assert starts.size == (256 << e) + 1 and starts[-1] == n and (np.diff(starts.astype(np.int64)) >= 0).all()
        # the SEGW form of an entry holds the same string, DIG on top of the word's hash field, over the same squeezed position
        w, d = R.segw_entries(h, y, nbits, ybits, pos1)
        rid, low = R.y_fields(y, pos1)
        assert np.array_equal(R.shl(d.astype(np.uint64), nbits - 16) | R.shr(w, ybits), R.sig_of(h, nbits))
        assert np.array_equal(w & R.U64(R.mask(ybits)), R.shl(rid, pos1) | low)


def test_wave_tables_hold_the_entries_in_slots_a_sketch_could_leave():
    for n in R.INDEX_N:
        cap, counts = R.wave_table_for(n)
        assert cap % 64 == 0 and cap <= R.RS_TILE and int(counts.sum()) == n and counts.max() <= cap and counts[0] == 0 and counts[-1] == 0
    assert len(R.index_slot_tables()) == 10 and all(cap % 64 == 0 and cap <= R.RS_TILE for _, cap, _ in R.index_slot_tables())
    spans = [s for _, cap, counts in R.index_slot_tables() for s in R.slot_tile_spans(cap, counts)]
    assert min(spans) <= 3 and 7 in spans and max(spans) > 90                # the one-load descriptor, and the offsets through LDS behind it
    h, y = R.index_entries("uniform", 4097, 30, 30, 12, 0)
    cap, counts = R.wave_table_for(4097)
    (_, _), (w, d), (sw, sd, _) = R.index_forms(h, y, 30, 30, 12, cap, counts)
    assert np.array_equal(R.slots_dense(sw, counts, cap), w) and np.array_equal(R.slots_dense(sd.astype(np.uint64), counts, cap), d.astype(np.uint64))


# ---- run heads ----
@pytest.mark.parametrize("miss", ["no_head_at_0", "line_start_missed"])
def test_head_cases_separate(miss):
    assert separated(R.head_cases(), lambda c: R.heads(R.head_stream(*c[:2], c[2]), c[2]), lambda c: R.heads(R.head_stream(*c[:2], c[2]), c[2], None, miss)) > 0


@pytest.mark.parametrize("n_seg", [256, 2048])
@pytest.mark.parametrize("miss", ["forced_ignored", "forced_at_n", "line_start_missed"])
def test_forced_boundary_cases_separate(miss, n_seg):
    def both(c, m):
        keys = R.head_stream(*c[:2], c[2])
        return R.heads(keys, c[2], R.head_boundaries(keys, c[2], n_seg), m)
    assert separated(R.head_cases(), lambda c: both(c, None), lambda c: both(c, miss)) > 0


def test_forced_boundaries_have_every_kind():
    keys = R.head_stream("random", 5 * 4096 + 9, 13)
    n = keys.size
    nat = set(R.heads(keys, 13).tolist())
    for n_seg in (256, 2048):
        b = R.head_boundaries(keys, 13, n_seg)
        assert b.size == n_seg + 1 and (np.diff(b.astype(np.int64)) >= 0).all() and b[0] == 0 and b[-1] == n
        inner = [x for x in b.tolist() if 0 < x < n]
        assert any(x in nat for x in inner) and any(x not in nat for x in inner)
        assert (np.diff(b.astype(np.int64)) == 0).any() and (b == n).sum() >= 2
    for kind, n, shift in R.head_cases():
        k = R.head_stream(kind, n, shift)
        h = R.heads(k, shift)
        if kind == "every_16" and shift < 63 and n > 16:
            assert np.array_equal(h, np.arange(0, n, 16))
        if kind == "all_distinct":
            assert h.size == n
        if kind == "last_alone" and n > 1:
            assert h.tolist() == [0, n - 1]


# ---- the significance string ----
@pytest.mark.parametrize("nbits", R.SIG_NBITS)
def test_hash_to_sig_and_back(nbits):
    rng = np.random.Generator(np.random.PCG64(nbits))
    hs = [0, 1, R.mask(nbits), R.mask(nbits) - 1, 1 << (nbits - 1), 0xff, 0x100 & R.mask(nbits)] + [int(x) & R.mask(nbits) for x in rng.integers(0, 1 << 63, 2000)]
    for h in hs:
        s = R.hash_to_sig(h, nbits)
        assert 0 <= s <= R.mask(nbits) and R.sig_to_hash(s, nbits) == h
        assert R.hash_to_sig(R.sig_to_hash(h, nbits), nbits) == h
    # the string orders by the low byte first
    assert R.hash_to_sig(1, nbits) > R.hash_to_sig(R.mask(nbits) & ~0xff, nbits)
