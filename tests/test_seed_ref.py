"""The case families of tests/seed_ref.py can tell a right kernel from a plausibly wrong one (no GPU): for every family that
tests/test_gpu_seed.py runs against lrge_amd/csrc/k_index.h and k_seed.h, the model's answer is computed together with the answers of named
near-miss models -- a prefix-max that restarts at a lane, row, tile or scan-chunk border, a home without the stretch, an unclamped count, a
tail left uncleared, `<` for `<=`, a diagonal rule without the length, a first-lane tie rule, a lost offset, swapped waves or rounds ... --
and at least one case of every family a near miss applies to must separate it from the truth.  Also: the closed-form placement is linear
probing in stream order, the home slot in split halves is the home slot in Python integers, and the models of lookup and expansion agree
with plain loops."""
import numpy as np
import pytest

import seed_ref as R


def differ(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            if x is None or y is None or x.shape != y.shape or not np.array_equal(x, y):
                return True
        elif x != y:
            return True
    return False


# ---- the table ----
# which families must catch which near miss (a family whose keys never meet the miss's border, width or length cannot)
PLACE_APPLIES = {
    "restart_64": ("sizes", "clustered", "mixed", "grid_cap", "widths"),
    "restart_256": ("sizes", "clustered", "mixed", "grid_cap"),
    "restart_2048": ("sizes", "clustered", "mixed", "grid_cap"),
    "restart_1024_tiles": ("big",),
    "home_no_stretch": ("widths",),
    "power_ignored": ("widths",),
    "count_unclamped": ("run_lengths",),
    "tail_not_cleared": ("sizes", "clustered", "sparse", "mixed", "grid_cap", "run_lengths", "widths", "overflow"),
}


def test_every_placement_miss_has_a_family():
    assert set(PLACE_APPLIES) == set(R.PLACE_MISSES)
    assert set(f for fs in PLACE_APPLIES.values() for f in fs) == set(R.TABLE_FAMILIES)


@pytest.mark.parametrize("miss", R.PLACE_MISSES)
def test_table_cases_separate(miss):
    for fam in PLACE_APPLIES[miss]:
        n = sum(differ(c.model(True, True, True), c.model(True, True, True, miss)) for c in R.table_cases(fam))
        assert n > 0, fam


def test_only_the_big_case_reaches_the_scan_chunk_border():
    for fam in R.TABLE_FAMILIES:
        if fam != "big":
            assert all(c.n <= R.SCAN_CHUNK * R.PLACE_TILE for c in R.table_cases(fam))
    (c,) = R.table_cases("big")
    assert c.n == 1025 * 2048 + 1
    hm = R.home(c.keys, c.cap, c.k, c.pw)
    border = R.SCAN_CHUNK * R.PLACE_TILE
    assert R.place_slots(hm)[border] > hm[border], "the run behind the border must be displaced by runs in front of it"


@pytest.mark.parametrize("miss", ["restart_64", "restart_256", "restart_2048"])
def test_segment_packed_cases_separate(miss):
    for c in R.seg_cases():
        assert differ(c.model(True, True, True), c.model(True, True, True, miss)), c.name


def test_segment_packed_cases_have_empty_segments_everywhere_and_a_tile_over_many_borders():
    for c in R.seg_cases():
        n_seg = 256 << c.e
        used = c.seg_used
        assert used[0] > 0 and used[-1] < n_seg - 1 and (np.diff(used) > 1).any()
        assert c.seg_start.size == n_seg and c.seg_start[0] == 0 and (np.diff(c.seg_start.astype(np.int64)) >= 0).all()
        seg_of_run = (c.sigs >> np.uint64(c.nr)).astype(np.int64)
        assert max(np.unique(seg_of_run[t:t + R.PLACE_TILE]).size for t in range(0, c.n, R.PLACE_TILE)) >= 10
        # the stream's hash field and the segment's number give the hash back
        w, _, kshift = c.stream()
        seg_of_entry = np.searchsorted(c.seg_start, c.starts, side="right") - 1
        assert np.array_equal(R.sig_to_hash(R.u64(seg_of_entry) << np.uint64(c.nr) | (w[c.starts] >> np.uint64(kshift)), c.nbits), c.keys)


def test_sparse_and_mixed_cases_hold_waves_on_both_sides_of_the_compose_limit():
    def spans(c):
        slot = R.place_slots(R.home(c.keys, c.cap, c.k, c.pw))
        out = []
        for w0 in range(0, c.n, 64):
            first = slot[w0 - 1] + 1 if w0 else 0
            out.append(int(slot[min(w0 + 64, c.n) - 1] - first + 1))
        return np.array(out)
    for c in R.table_cases("sparse"):
        assert (spans(c) > R.PLACE_COMP).any(), c.name
    for c in R.table_cases("mixed"):
        s = spans(c)
        tile0 = s[:R.PLACE_TILE // 64]
        assert (tile0 > R.PLACE_COMP).any() and (tile0 <= R.PLACE_COMP).any(), c.name
    for c in R.table_cases("sizes"):
        assert c.n <= 64 or (spans(c)[1:] <= R.PLACE_COMP).any(), c.name


def test_run_length_case_meets_every_edge_of_count_and_histogram():
    (c, small) = R.table_cases("run_lengths")
    assert tuple(c.lens) == R.RUN_LENGTHS and c.max_bin == R.MAX_BIN
    _, hist, _, _, _ = c.model(False, True, True)
    assert hist[R.MAX_BIN] == 5 and hist[R.MAX_BIN - 1] == 1 and hist[R.OCC_LDS_BINS] == 1 and hist[R.OCC_LDS_BINS - 1] == 1 and hist[R.OCC_LDS_BINS + 1] == 1
    _, hist, _, _, _ = small.model(False, True, True)
    assert hist[5000] == 2 and hist[4999] == 1


def test_width_cases_cover_the_partial_widths_and_the_clamped_exponents():
    parts = [(2 * k) % 8 for k in R.TABLE_K]
    assert parts == [2, 4, 6, 0, 6]
    assert [R.clamp_power(13, p) for p in R.TABLE_PW] == [0, 4, 4, 28]
    assert [R.clamp_power(14, p) for p in R.TABLE_PW] == [0, 3, 2, 14]
    assert [R.clamp_power(15, p) for p in R.TABLE_PW] == [0, 3, 2, 9]
    assert [R.clamp_power(16, p) for p in R.TABLE_PW] == [0, 0, 0, 0]
    for c in R.table_cases("widths"):
        hm = R.home(c.keys, c.cap, c.k, c.pw)
        assert (np.diff(hm) >= 0).all(), "the home is monotone in the stream's order"
        if c.nbits % 8:
            assert (hm != R.home(c.keys, c.cap, c.k, c.pw, "home_no_stretch")).sum() >= 16, c.name
            if c.pw:
                assert (hm != R.home(c.keys, c.cap, c.k, 0)).sum() >= 16, c.name


def test_overflow_cases_overflow_by_one_slot_and_fit_with_one_more():
    flags = {c.name: c.model(False, True, True)[2] for c in R.table_cases("overflow")}
    assert flags == {"short": 1, "short_by_one": 1, "enough": 0, "short64_by_one": 1, "enough64": 0}
    for c in R.table_cases("overflow"):
        img, _, ov, last, _ = c.model(False, True, True)
        if not ov:
            assert last == c.n_slots - 2 and img[-2] == R.HT_EMPTY and img[-1] == R.HT_EMPTY


def test_home_in_split_halves_is_the_home_in_python_integers():
    for c in R.table_cases("widths") + R.table_cases("mixed"):
        part = c.nbits % 8
        at = 64 - 8 * ((c.nbits + 7) // 8)
        pw = R.clamp_power(c.k, c.pw)
        hm = R.home(c.keys, c.cap, c.k, c.pw)
        for i in list(range(0, c.n, 97)) + [c.n - 1]:
            bs = int.from_bytes(int(c.keys[i]).to_bytes(8, "little"), "big")
            if part:
                v = (bs >> at) & 0xff
                f = v << (8 - part) if pw == 0 else min(255, 256 - 256 * ((1 << part) - v) ** pw // (1 << part) ** pw)
                bs = bs & ~(0xff << at) | f << at
            assert int(hm[i]) == bs * c.cap >> 64, (c.name, i)


def test_closed_form_placement_is_linear_probing_in_stream_order():
    for fam in ("sizes", "clustered", "mixed"):
        for c in R.table_cases(fam):
            if c.n > 3000:
                continue
            hm = R.home(c.keys, c.cap, c.k, c.pw)
            taken, want = set(), []
            for h in hm:
                s = int(h)
                while s in taken:
                    s += 1
                taken.add(s)
                want.append(s)
            assert np.array_equal(R.place_slots(hm), np.array(want)), c.name


def test_stream_order_is_the_byte_reversed_order_and_sig_maps_are_inverse():
    for c in R.table_cases("widths") + R.table_cases("sizes") + R.seg_cases():
        assert (np.diff(R.byte_swap(c.keys).astype(np.float64)) > 0).all() or (np.diff(R.byte_swap(c.keys) >> np.uint64(1)).astype(np.int64) >= 0).all()
        assert np.array_equal(R.hash_to_sig(c.keys, c.nbits), c.sigs)
        assert int(c.keys.max()) < (1 << c.nbits)


def test_streams_carry_the_heads_the_model_reads():
    for c in R.table_cases("sizes")[-3:] + R.table_cases("run_lengths"):
        for packed in (False, True):
            w, y, kshift = c.stream(packed)
            heads = np.arange(c.n) if c.sparse else c.starts
            assert w.size == (c.n if c.sparse else c.M)
            assert np.array_equal(w[heads] >> np.uint64(kshift), c.keys)
            if packed:
                yb = w[heads] & np.uint64(R.mask(kshift))
                assert np.array_equal((yb >> np.uint64(c.pk_pos1)) << np.uint64(32) | (yb & np.uint64(R.mask(c.pk_pos1))), c.y_heads(True))
            else:
                assert np.array_equal(y[heads], c.y_heads(False))
            if not c.sparse:        # runs are runs of ONE hash, and neighbours differ
                h = w >> np.uint64(kshift)
                assert np.array_equal(np.flatnonzero(np.concatenate([[True], h[1:] != h[:-1]])), c.starts)


# ---- lookup ----
def lookup_queries(c):
    """(hashes, mid_occ): every present key, then the absent ones"""
    return np.concatenate([c.keys, c.absent()]), 2


def test_lookup_cases_separate_the_threshold_and_hold_absent_keys_on_every_side():
    for fam in ("sizes", "clustered", "mixed"):
        seen = 0
        for c in R.table_cases(fam):
            q, mid = lookup_queries(c)
            ys = c.y_heads(False)
            t = R.lookup(c.keys, c.starts, c.M, ys, True, q, mid)
            w = R.lookup(c.keys, c.starts, c.M, ys, True, q, mid, "mid_lt")
            seen += differ(t, w)
            a = R.hash_to_sig(c.absent(), c.nbits)
            if c.n > 60:
                assert (a < c.sigs[0]).any() and (a > c.sigs[-1]).any() and ((a > c.sigs[0]) & (a < c.sigs[-1])).any(), c.name
            assert not t[1][c.n:].any() and t[1][:c.n].all()
        assert seen > 0, fam


def test_lookup_model_is_a_dictionary():
    c = R.table_cases("sizes")[5]
    q, mid = lookup_queries(c)
    ys = c.y_heads(True)
    hs, hc, hn = R.lookup(c.keys, c.starts, c.M, ys, True, q, mid)
    d = {int(k): r for r, k in enumerate(c.keys)}
    for i, x in enumerate(q):
        r = d.get(int(x))
        if r is None:
            assert (hs[i], hc[i], hn[i]) == (0, 0, 0)
        else:
            ln = int(c.lens[r])
            assert hc[i] == ln and hn[i] == (ln if ln <= mid else 0)
            assert hs[i] == (R.HT_INLINE | int(ys[r]) if ln == 1 else int(c.starts[r]))


# ---- counts and expansion ----
SEED_APPLIES = {
    "mid_lt": ("lengths", "wave_totals"),
    "diag_ignores_len": ("names",),
    "no_dual_ge": ("names",),
    "ties_first_lane": ("lengths", "zero_lists", "names"),
    "offset_absolute": ("lengths", "wave_totals", "zero_lists", "names"),
    "rev_qpos_no_span": R.SEED_FAMILIES,
}


def test_every_seed_miss_has_a_family():
    assert set(SEED_APPLIES) == set(R.SEED_MISSES)
    assert set(f for fs in SEED_APPLIES.values() for f in fs) == set(R.SEED_FAMILIES)


@pytest.mark.parametrize("miss", R.SEED_MISSES)
def test_seed_cases_separate(miss):
    for fam in SEED_APPLIES[miss]:
        assert sum(differ(c.truth(), c.truth(miss)) for c in R.seed_cases(fam)) > 0, fam


def test_seed_cases_emit_what_they_count_and_fill_their_window():
    for fam in R.SEED_FAMILIES:
        for c in R.seed_cases(fam):
            t = c.truth()
            hn, hv, key = t[0], t[1], t[2]
            assert not (key == R.PATTERN64).any(), c.name
            assert key.size == int(hv[c.b:c.e].sum())
            assert (hv <= hn).all() and (c.S.check_names or np.array_equal(hv, hn))


def test_expansion_model_is_the_plain_loop():
    for fam, idx in (("names", 4), ("lengths", 6), ("layouts", 0)):
        c = R.seed_cases(fam)[idx]
        S = c.S
        hn, hv = R.counts(S)
        keys, vals = [], []
        for i in range(c.b, c.e):
            qy, n = int(S.qy[i]), int(hn[i])
            q, qpos, qs, span = qy >> 32, (qy & 0xFFFFFFFF) >> 1, qy & 1, int(S.qx[i]) & 0xff
            kept = 0
            for j in range(n):
                st = int(S.hs[i])
                y = st & ~R.HT_INLINE if st & R.HT_INLINE else int(S.y_of(S.pos[st + j:st + j + 1])[0])
                rid, rpos, ts = y >> 32, (y & 0xFFFFFFFF) >> 1, y & 1
                slf = 0
                if S.check_names:
                    same = S.q_rank[q] == S.t_rank[rid] and S.t_len[rid] == S.q_len[q]
                    if same and rpos == qpos:
                        continue
                    if S.no_dual and S.q_rank[q] > S.t_rank[rid]:
                        continue
                    slf = int(same and ts == qs)
                rev = int(ts != qs)
                qp = int(S.q_len[q]) - (qpos + 1 - span) - 1 if rev else qpos
                rank = (int(S.krank[i]) - int(S.krank[S.qmz_off[q]])) & 0xFFFFF if S.krank is not None else 0
                keys.append((q - c.q0) << (c.kl[0] + 1 + c.kl[1]) | rid << (c.kl[0] + 1) | rev << c.kl[0] | rpos)
                vals.append(rank << 44 | slf << 43 | span << 32 | qp)
                kept += 1
            assert kept == hv[i]
        k, v = R.expand(S, hn, R.scan0(hv), c.b, c.e, c.q0, c.kl)
        assert np.array_equal(k, R.u64(keys)) and np.array_equal(v, R.u64(vals)), c.name


def test_seed_families_hold_what_they_name():
    S = R.seed_cases("lengths")[0].S
    assert set(S.hc.tolist()) >= {0, 1, 63, 64, 65, R.MID_OCC, R.MID_OCC + 1}
    assert ((S.hs & np.uint64(R.HT_INLINE)) != 0).any() and ((S.hc == 1) & ((S.hs & np.uint64(R.HT_INLINE)) == 0)).any()
    assert any(c.b % 64 and c.e % 64 and (c.e - c.b) % 64 for c in R.seed_cases("lengths"))
    S = R.seed_cases("wave_totals")[0].S
    hn, _ = R.counts(S)
    assert [int(hn[w:w + 64].sum()) for w in range(0, 320, 64)] == [64, 0, 65, 128, 64 * R.MID_OCC]
    S = R.seed_cases("layouts")[0].S
    assert 255 in (S.qx & np.uint64(0xff)).tolist()
    c = R.seed_cases("layouts")[-1]
    assert c.kl[0] + 1 + c.kl[1] + c.bits_qy + 9 == 64 and (c.truth()[2] >> np.uint64(63)).any() is not None
    # names: every relation of the ranks, both strand relations of a read against itself, a same-rank read of another length
    c = R.seed_cases("names")[2]
    t = c.truth()
    assert (t[3] >> np.uint64(43) & np.uint64(1)).any() and not (t[3] >> np.uint64(43) & np.uint64(1)).all()
    assert int(t[1].sum()) < int(R.seed_cases("names")[0].truth()[1].sum())
    assert int(R.seed_cases("names")[4].truth()[1].sum()) < int(t[1].sum())


# ---- k_expand_q ----
@pytest.mark.parametrize("n_planes", [2, 3])
@pytest.mark.parametrize("cls", [0, 1, 2])
@pytest.mark.parametrize("miss", R.EXPQ_MISSES)
def test_expand_q_cases_separate(miss, cls, n_planes):
    n = 0
    for pop in R.EXPQ_POPULATIONS:
        for c in R.expq_cases(cls, n_planes, pop):
            assert all(R.expq_class(t, c.smax, c.mmax) == cls for t in c.totals() if t)
            n += differ(c.truth(), c.truth(miss))
    assert n > 0


@pytest.mark.parametrize("cls", [0, 1, 2])
def test_expand_q_cases_hold_the_round_borders_and_the_populations(cls):
    R_ = R.EXPQ_ROUND[cls]
    assert R_ == (2048, 4096, 8192)[cls]
    for pop in R.EXPQ_POPULATIONS:
        cases = R.expq_cases(cls, 2, pop)
        assert [c.totals()[0] for c in cases] == [0, 1, R_ - 1, R_, R_ + 1, 3 * R_ + 17]
        for c in cases:
            tot = c.totals()[0]
            _, kept = c.truth()
            if pop == "none":
                assert kept[0] == 0
            elif pop in ("all", "one_bucket") and tot >= 12:
                assert kept[0] == tot
            elif pop == "alternating" and tot >= 12:
                assert kept[0] == (tot + 1) // 2
            # the neighbours' slots lie in the buffer, in front of and behind the launch's
            assert c.n_out > tot and c.mz_begin < c.S.qmz_off[c.q0] and c.mz_end > c.S.qmz_off[c.q0 + c.nqb]
    # one_bucket: pairs that are ALONE (a single anchor each would be dead) survive through the bucket they share
    c = R.expq_cases(cls, 3, "one_bucket")[3]
    e = c.emitted(1)
    pairs = (e & np.uint64(R.mask(c.kl[0] + 1 + c.kl[1]))) >> np.uint64(c.kl[0])
    assert np.unique(pairs).size == 6 and np.unique(R.pair_bucket(pairs, R.EXPQ_LOG2B[cls])).size == 1


def test_expand_q_mixed_case_holds_every_class_and_the_empty_queries():
    for n_planes in (2, 3):
        c = R.expq_mixed_case(n_planes)
        cl = [R.expq_class(t) for t in c.totals()]
        assert set(cl) == {0, 1, 2} and 0 in c.totals()
        assert (np.diff(c.S.qmz_off.astype(np.int64)) == 0).any(), "a query without minimizers"
        assert 8192 in c.totals() and 8193 in c.totals()
        for miss in R.EXPQ_MISSES:
            assert differ(c.truth(), c.truth(miss)), miss
