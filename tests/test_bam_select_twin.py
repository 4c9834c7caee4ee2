"""The sampled ingest of unaligned BAM without a GPU (lrge_amd/csrc/fx_window.h FxKeepMode over bam_round.h):
the host twin runs the BAM windows in the two modes of the sampled ingest -- the census, which keeps nothing, and the selection,
which keeps the records of an ascending list of ordinals -- against the host parser (lrge_hip_read_records) on the same bytes.
The mode changes what is kept, not what is proven: the well-formed corpus, baits included, is proven at every segment, window and
piece, the count and the base sum are the host's, read j of a selection is record sel[j] of the host, the store is the chosen
records' packed bytes, dense, and the counts say what was seen and kept."""
import ctypes as C
import random

import numpy as np
import pytest

import bam_corpus as B
from test_bam_twin import OK, UNPROVEN, FxRec, load_twin
from test_bam_window_twin import SEGMENTS, WINDOWS, pieces_for, small_big_small
from test_bam_window_twin import host   # noqa: F401  (fixture)

INVALID = -2


def bind(L):
    """the prototypes of the twin's sampled entries (the seek-twin test and the GPU suite bind them too)"""
    L.bam_twin_census.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64 * 4)]
    L.bam_twin_selected.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    L.bam_twin_windowed_select_stats.argtypes = [C.POINTER(C.c_uint64 * 4)]
    L.bam_twin_windowed_cuts.argtypes = [C.c_void_p, C.c_uint64]
    L.bam_twin_windowed_cuts.restype = C.c_uint64
    L.bam_twin_windowed_count.restype = C.c_uint64
    L.bam_twin_windowed_table.argtypes = [C.c_void_p]
    L.bam_twin_windowed_stats.argtypes = [C.POINTER(C.c_uint64 * 5)]
    L.bam_twin_windowed_bam_stats.argtypes = [C.c_void_p]
    L.bam_twin_windowed_store.argtypes = [C.c_char_p]
    L.bam_twin_windowed_store.restype = C.c_uint64
    L.bam_twin_windowed_seq.argtypes = [C.c_uint64, C.c_uint32, C.c_char_p]
    L.bam_twin_windowed_seq.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def twin():
    return bind(load_twin())


def census(L, data, S, window, piece):
    """(verdict, [records, bases, text bytes, windows]) of the counting twin"""
    out = (C.c_uint64 * 4)()
    rc = L.bam_twin_census(data, len(data), S, window, piece, C.byref(out))
    return rc, list(out)


def window_records(L):
    """the records of every window of the run that just ended"""
    k = L.bam_twin_windowed_cuts(None, 0)
    a = np.zeros(max(1, k), dtype=np.uint64)
    L.bam_twin_windowed_cuts(a.ctypes.data, k)
    return a[:k].tolist()


def read_kept(L, data):
    """([(name, sequence)], store, select stats) of the run that just ended: the table is dense, in file order, packed"""
    n = L.bam_twin_windowed_count()
    tab = (FxRec * max(1, n))()
    L.bam_twin_windowed_table(tab)
    ss = (C.c_uint64 * 4)()
    L.bam_twin_windowed_select_stats(C.byref(ss))
    store = C.create_string_buffer(max(1, L.bam_twin_windowed_store(None)))
    n_store = L.bam_twin_windowed_store(store)
    out, at = [], 0
    buf = C.create_string_buffer(max(1, max((tab[i].seq_len for i in range(n)), default=0)))
    for i in range(n):
        r = tab[i]
        assert r.name_off + r.name_len <= len(data) and r.seq_off == at and r.seq_span == (r.seq_len + 1) // 2
        assert L.bam_twin_windowed_seq(i, i % 4, buf) == r.seq_len
        out.append((data[r.name_off:r.name_off + r.name_len], buf.raw[:r.seq_len]))
        at += r.seq_span
    assert n_store == at
    return out, store.raw[:n_store], list(ss)


def selected(L, data, S, window, piece, sel):
    """(verdict, [(name, sequence)], store, select stats) of the selecting twin"""
    a = np.ascontiguousarray(sel, dtype=np.uint32)
    rc = L.bam_twin_selected(data, len(data), S, window, piece, a.ctypes.data if a.size else None, a.size)
    if rc != OK:
        assert L.bam_twin_windowed_count() == 0 and L.bam_twin_windowed_store(None) == 0     # (a refused call keeps nothing)
        return rc, None, None, None
    return (rc,) + read_kept(L, data)


def selections(n, per_window):
    """the selections of one run over n records whose windows held per_window records each"""
    rng = np.random.default_rng(5)
    sels = {"empty": [], "all": list(range(n)), "every third": list(range(0, n, 3)), "seeded half": sorted(rng.permutation(n)[:n // 2].tolist())}
    if n:
        sels["first"], sels["last"] = [0], [n - 1]
    edges, r0 = set(), 0
    for m in per_window:                                            # the records on either side of every cut
        if m:
            edges |= {r0, r0 + m - 1}
        r0 += m
    assert r0 == n
    if len([m for m in per_window if m]) > 1:
        sels["around the cuts"] = sorted(edges)
    return sels


def check_kept(got, rec_h, bases, sel, what):
    rc, rec, store, ss = got
    assert rc == OK, (what, rc)                                     # a condition, not a hope: zero unproven verdicts
    want = [rec_h[i] for i in sel]
    assert rec == want, what
    assert store == b"".join(B.pack_seq(s) for _, s in want), what
    assert ss == [len(rec_h), len(sel), bases, sum(len(s) for _, s in want)], (what, ss)


@pytest.mark.parametrize("S", SEGMENTS)
def test_census_equals_host_parser(twin, host, S):
    """records and bases of every well-formed case and bait at every window and piece: the host parser's; zero unproven verdicts"""
    cases = B.well_formed()
    assert {n for n, _ in B.baits()} <= {n for n, _ in cases}
    n_runs = n_multi = 0
    for name, data in cases:
        rc_h, rec_h, msg = host(data)
        assert rc_h == 0, (name, msg)
        bases = sum(len(s) for _, s in rec_h)
        for window in WINDOWS:
            for piece in pieces_for(data, window):
                rc, out = census(twin, data, S, window, piece)
                assert rc == OK, (name, S, window, piece, rc)
                assert out[:3] == [len(rec_h), bases, len(data)], (name, S, window, piece, out)
                assert sum(window_records(twin)) == len(rec_h)
                assert twin.bam_twin_windowed_count() == 0 and twin.bam_twin_windowed_store(None) == 0      # the census keeps nothing
                n_runs += 1
                n_multi += out[3] > 1
    assert n_runs > 200 and n_multi > 100                           # (not vacuous: many runs went through several windows)


@pytest.mark.parametrize("S", SEGMENTS)
def test_selections_equal_host_subset(twin, host, S):
    """every well-formed case and bait at every window and piece: the empty selection, the first record, the last, all, every third,
    a seeded half and the records on either side of every cut -- identifiers, sequences, the packed store and the counts"""
    n_sel = n_cut = 0
    for name, data in B.well_formed():
        rec_h = host(data)[1]
        bases = sum(len(s) for _, s in rec_h)
        for window in WINDOWS:
            for piece in pieces_for(data, window):
                rc, out = census(twin, data, S, window, piece)
                assert rc == OK, (name, S, window, piece)
                for kind, sel in selections(len(rec_h), window_records(twin)).items():
                    check_kept(selected(twin, data, S, window, piece, sel), rec_h, bases, sel, (name, S, window, piece, kind))
                    n_sel += 1
                    n_cut += kind == "around the cuts"
    assert n_sel > 1500 and n_cut > 100


def test_unproven_list(twin):
    """what the windowed scan leaves to the host stays unproven in both modes, and nothing is kept"""
    for name, data in B.unproven():
        for window in [4, 17] + WINDOWS:
            for piece in (1, 61, window):
                for S in (64, 4096):
                    rc, out = census(twin, data, S, window, piece)
                    assert rc == UNPROVEN and out == [0, 0, 0, 0], (name, window, piece, S)
                    assert twin.bam_twin_windowed_count() == 0 and twin.bam_twin_windowed_store(None) == 0
                    for sel in ([], [0]):
                        assert selected(twin, data, S, window, piece, sel)[0] == UNPROVEN, (name, window, piece, S, sel)


def test_bad_selections(twin, host):
    """descending, repeated and out-of-range ordinals are invalid, at one window and at many; nothing is left behind"""
    data = dict(B.well_formed())["bait_quality"]
    n = len(host(data)[1])
    assert n > 10
    for window in (257, len(data) + 1):
        for sel in ([5, 3], [0, 4, 4, 9], [n], [0, n - 1, n], [n + 7]):
            assert selected(twin, data, 64, window, 61, sel)[0] == INVALID, (window, sel)
        assert selected(twin, data, 64, window, 61, [n - 1])[0] == OK
    hdr = B.header()
    assert selected(twin, hdr, 64, 64, 1, [0])[0] == INVALID and selected(twin, hdr, 64, 64, 1, [])[0] == OK


def test_header_that_ends_the_text(twin, host):
    """an empty census and an empty selection, whether the header is cut off as a window of its own or scanned resident"""
    for hdr in (B.header(), B.header(b""), B.header(refs=[(b"chr1", 1000)])):
        assert host(hdr)[:2] == (0, [])
        for window in (4, 8, len(hdr) - 1, len(hdr), len(hdr) + 1):
            for piece in (1, len(hdr)):
                rc, out = census(twin, hdr, 64, window, piece)
                assert rc == OK and out[:3] == [0, 0, len(hdr)] and out[3] <= 1, (window, piece, out)
                assert selected(twin, hdr, 64, window, piece, []) == (OK, [], b"", [0, 0, 0, 0])


def test_odd_and_zero_lengths_side_by_side_in_the_store(twin, host):
    """every chosen record starts on a byte of the store; an odd length keeps its pad nibble, an empty sequence takes nothing"""
    seqs = [b"ACG", b"", b"T", b"", b"", b"GA", b"NACGT", b"", b"C"]
    data = B.bam([B.record(b"o%d" % i, s) for i, s in enumerate(seqs)])
    rec_h = host(data)[1]
    assert [s for _, s in rec_h] == seqs
    bases = sum(len(s) for s in seqs)
    n_multi = 0
    for window in (64, 100, 257):
        rc, out = census(twin, data, 64, window, 61)
        assert rc == OK and out[:2] == [len(seqs), bases]
        n_multi += out[3] > 1
        for sel in (list(range(0, 9, 2)), list(range(1, 9, 2)), [0, 1, 2], [3, 4], [6, 7, 8]):     # alternating: odd beside empty either way round
            check_kept(selected(twin, data, 64, window, 61, sel), rec_h, bases, sel, (window, sel))
    assert n_multi >= 2


def test_small_record_in_front_of_a_large_one(twin, host):
    """a record of many windows between two small ones, chosen and not chosen"""
    data, recs = small_big_small()
    rec_h = host(data)[1]
    assert [len(s) for _, s in rec_h] == [2, 40001, 3]
    for window, piece in ((64, 3001), (64, 61), (3001, 3001)):
        rc, out = census(twin, data, 64, window, piece)
        assert rc == OK and out[:2] == [3, 40006] and out[3] >= 2, (window, out)
        for sel in ([], [0], [1], [2], [0, 2], [0, 1], [1, 2], [0, 1, 2]):
            check_kept(selected(twin, data, 64, window, piece, sel), rec_h, 40006, sel, (window, piece, sel))


def test_mapped_record_in_the_third_window(twin, host):
    """two windows are proven before the mapped record's bytes arrive: the census and the selection are unproven, nothing is kept"""
    rng = random.Random(53)
    recs = [B.record(b"m%d" % i, B._seq(rng, 30)) for i in range(12)]
    window = 200
    k = next(i for i in range(12) if len(B.header()) + sum(len(r) for r in recs[:i]) > 2 * window)
    rc, out = census(twin, B.bam(recs), 64, window, window)
    assert rc == OK and out[0] == 12 and out[3] >= 3
    bad = B.bam(recs[:k] + [B.record(b"mapped", B._seq(rng, 30), flag=0)] + recs[k:])
    assert host(bad)[0] != 0
    assert census(twin, bad, 64, window, window) == (UNPROVEN, [0, 0, 0, 0])
    assert selected(twin, bad, 64, window, window, [0, 1])[0] == UNPROVEN        # (records of the first window, which was proven)
    for tail in (1, 2, 3):                                                       # 1-3 trailing bytes
        assert census(twin, B.bam(recs) + bytes(tail), 64, window, window)[0] == UNPROVEN
        assert selected(twin, B.bam(recs) + bytes(tail), 64, window, window, [0])[0] == UNPROVEN


def test_arguments(twin):
    data = B.header()
    out = (C.c_uint64 * 4)()
    assert twin.bam_twin_census(data, len(data), 63, 64, 1, C.byref(out)) == -1           # a segment has 64 bytes or more
    assert twin.bam_twin_selected(data, len(data), 64, 64, 0, None, 0) == -1              # a piece has bytes
