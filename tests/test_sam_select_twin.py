"""The sampled ingest of unaligned SAM without a GPU (lrge_amd/csrc/fx_window.h FxKeepMode over the SAM windows, DESIGN section
27): the host twin runs the SAM windows in the two modes of the sampled ingest -- the census, which keeps nothing, and the
selection, which keeps the records of an ascending list of ordinals -- against the host parser (lrge_hip_read_records) on the
same bytes.  The mode changes what is kept, not what is proven: the well-formed corpus is proven at every window and piece, the
count and the base sum are the host's, read j of a selection is record sel[j] of the host, the store is the chosen records'
bases, dense, and the counts say what was seen and kept."""
import ctypes as C
import random

import numpy as np
import pytest

import sam_corpus as S
from test_bam_select_twin import selections
from test_sam_twin import OK, UNPROVEN, FxRec, load_twin
from test_sam_window_twin import WINDOWS
from test_sam_window_twin import host   # noqa: F401  (fixture)

INVALID = -2


def bind(L):
    """the prototypes of the twin's sampled entries (the seek-twin test and the GPU suite bind them too)"""
    L.sam_twin_census.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64 * 4)]
    L.sam_twin_selected.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    L.sam_twin_windowed_select_stats.argtypes = [C.POINTER(C.c_uint64 * 4)]
    L.sam_twin_windowed_cuts.argtypes = [C.c_void_p, C.c_uint64]
    L.sam_twin_windowed_cuts.restype = C.c_uint64
    L.sam_twin_windowed_count.restype = C.c_uint64
    L.sam_twin_windowed_table.argtypes = [C.c_void_p]
    L.sam_twin_windowed_stats.argtypes = [C.POINTER(C.c_uint64 * 4)]
    L.sam_twin_windowed_store.argtypes = [C.c_char_p]
    L.sam_twin_windowed_store.restype = C.c_uint64
    L.sam_twin_windowed_seq.argtypes = [C.c_uint64, C.c_char_p]
    L.sam_twin_windowed_seq.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def twin():
    return bind(load_twin())


def pieces_for(window):
    return sorted({1, 61, window})


def census(L, data, window, piece):
    """(verdict, [records, bases, text bytes, windows]) of the counting twin"""
    out = (C.c_uint64 * 4)()
    rc = L.sam_twin_census(data, len(data), window, piece, C.byref(out))
    return rc, list(out)


def window_records(L):
    """the records of every window of the run that just ended"""
    k = L.sam_twin_windowed_cuts(None, 0)
    a = np.zeros(max(1, k), dtype=np.uint64)
    L.sam_twin_windowed_cuts(a.ctypes.data, k)
    return a[:k].tolist()


def read_kept(L, data):
    """([(name, sequence)], store, select stats) of the run that just ended: the table is dense, in file order"""
    n = L.sam_twin_windowed_count()
    tab = (FxRec * max(1, n))()
    L.sam_twin_windowed_table(tab)
    ss = (C.c_uint64 * 4)()
    L.sam_twin_windowed_select_stats(C.byref(ss))
    store = C.create_string_buffer(max(1, L.sam_twin_windowed_store(None)))
    n_store = L.sam_twin_windowed_store(store)
    out, at = [], 0
    for i in range(n):
        r = tab[i]
        assert r.name_off + r.name_len <= len(data) and r.seq_off == at and r.seq_span == r.seq_len
        out.append((data[r.name_off:r.name_off + r.name_len], store.raw[at:at + r.seq_len]))
        at += r.seq_len
    assert n_store == at
    return out, store.raw[:n_store], list(ss)


def selected(L, data, window, piece, sel):
    """(verdict, [(name, sequence)], store, select stats) of the selecting twin"""
    a = np.ascontiguousarray(sel, dtype=np.uint32)
    rc = L.sam_twin_selected(data, len(data), window, piece, a.ctypes.data if a.size else None, a.size)
    if rc != OK:
        assert L.sam_twin_windowed_count() == 0 and L.sam_twin_windowed_store(None) == 0     # (a refused call keeps nothing)
        return rc, None, None, None
    return (rc,) + read_kept(L, data)


def check_kept(got, rec_h, bases, sel, what):
    rc, rec, store, ss = got
    assert rc == OK, (what, rc)                                     # a condition, not a hope: zero unproven verdicts
    want = [rec_h[i] for i in sel]
    assert rec == want, what
    assert store == b"".join(s for _, s in want), what              # the store is dense: the chosen bases and nothing else
    assert ss == [len(rec_h), len(sel), bases, sum(len(s) for _, s in want)], (what, ss)


def test_census_equals_host_parser(twin, host):
    """records and bases of every well-formed case at every window and piece: the host parser's; zero unproven verdicts"""
    n_runs = n_multi = 0
    for name, data in S.well_formed():
        rc_h, rec_h, msg = host(data)
        assert rc_h == 0, (name, msg)
        bases = sum(len(s) for _, s in rec_h)
        for window in WINDOWS:
            for piece in pieces_for(window):
                rc, out = census(twin, data, window, piece)
                assert rc == OK, (name, window, piece, rc)
                assert out[:3] == [len(rec_h), bases, len(data)], (name, window, piece, out)
                assert sum(window_records(twin)) == len(rec_h)
                assert twin.sam_twin_windowed_count() == 0 and twin.sam_twin_windowed_store(None) == 0      # the census keeps nothing
                n_runs += 1
                n_multi += out[3] > 1
    assert n_runs > 300 and n_multi > 150                           # (not vacuous: many runs went through several windows)


def test_selections_equal_host_subset(twin, host):
    """every well-formed case at every window: the empty selection, the first record, the last, all, every third, a seeded half and
    the records on either side of every cut -- identifiers, sequences, the dense store and the counts"""
    n_sel = n_cut = 0
    for name, data in S.well_formed():
        rec_h = host(data)[1]
        bases = sum(len(s) for _, s in rec_h)
        for window in WINDOWS:
            for piece in (61, window):
                rc, out = census(twin, data, window, piece)
                assert rc == OK, (name, window, piece)
                for kind, sel in selections(len(rec_h), window_records(twin)).items():
                    check_kept(selected(twin, data, window, piece, sel), rec_h, bases, sel, (name, window, piece, kind))
                    n_sel += 1
                    n_cut += kind == "around the cuts"
    assert n_sel > 1500 and n_cut > 100


def test_one_byte_pieces(twin, host):
    """a piece of one byte: blocks end between the CR and the LF of a line, inside @CO lines and behind the last byte of a text
    without a final line feed"""
    cases = dict(S.well_formed())
    for name in ("crlf", "co_and_empty_lines", "no_final_lf", "no_final_lf_empty_quality", "final_cr_after_crlf", "names", "star_star_sequence"):
        data = cases[name]
        rec_h = host(data)[1]
        bases = sum(len(s) for _, s in rec_h)
        for window in (64, 257):
            rc, out = census(twin, data, window, 1)
            assert rc == OK and out[:2] == [len(rec_h), bases], (name, window)
            for kind, sel in selections(len(rec_h), window_records(twin)).items():
                check_kept(selected(twin, data, window, 1, sel), rec_h, bases, sel, (name, window, kind))


def test_unproven_list(twin):
    """what the windowed scan leaves to the host stays unproven in both modes at every window, and nothing is kept"""
    for name, data, _ in S.unproven():
        for window in [4, 17] + WINDOWS:
            for piece in (1, 61, window):
                rc, out = census(twin, data, window, piece)
                assert rc == UNPROVEN and out == [0, 0, 0, 0], (name, window, piece)
                assert twin.sam_twin_windowed_count() == 0 and twin.sam_twin_windowed_store(None) == 0
                for sel in ([], [0]):
                    assert selected(twin, data, window, piece, sel)[0] == UNPROVEN, (name, window, piece, sel)


def test_bad_selections(twin, host):
    """descending, repeated and out-of-range ordinals are invalid, at one window and at many; nothing is left behind"""
    data = dict(S.well_formed())["plain_40"]
    n = len(host(data)[1])
    assert n == 40
    for window in (257, len(data) + 1):
        for sel in ([5, 3], [0, 4, 4, 9], [n], [0, n - 1, n], [n + 7]):
            assert selected(twin, data, window, 61, sel)[0] == INVALID, (window, sel)
        assert selected(twin, data, window, 61, [n - 1])[0] == OK
    assert selected(twin, S.HD, 64, 1, [0])[0] == INVALID and selected(twin, S.HD, 64, 1, [])[0] == OK


def test_header_that_ends_the_text(twin, host):
    """an empty census and an empty selection, whether the header is cut off as a window of its own or scanned resident"""
    cases = dict(S.well_formed())
    for hdr in (cases["header_only"], cases["header_no_lf"], cases["header_three_lines"]):
        assert host(hdr)[:2] == (0, [])
        for window in (4, 8, len(hdr) - 1, len(hdr), len(hdr) + 1):
            for piece in (1, len(hdr)):
                rc, out = census(twin, hdr, window, piece)
                assert rc == OK and out[:3] == [0, 0, len(hdr)], (window, piece, out)
                assert selected(twin, hdr, window, piece, []) == (OK, [], b"", [0, 0, 0, 0])


def test_star_and_empty_sequences_side_by_side_in_the_store(twin, host):
    """'*' and an empty field are length 0 and take nothing of the store; their neighbours lie back to back"""
    seqs = [b"ACG", b"*", b"T", b"", b"*", b"GA", b"NACGT", b"", b"C"]
    data = S.sam([S.rec(b"o%d" % i, s, qual=b"*") for i, s in enumerate(seqs)])
    rec_h = host(data)[1]
    assert [s for _, s in rec_h] == [b"" if s == b"*" else s for s in seqs]
    bases = sum(len(s) for _, s in rec_h)
    n_multi = 0
    for window in (64, 100, 257):
        rc, out = census(twin, data, window, 61)
        assert rc == OK and out[:2] == [len(seqs), bases]
        n_multi += out[3] > 1
        for sel in (list(range(0, 9, 2)), list(range(1, 9, 2)), [0, 1, 2], [3, 4], [6, 7, 8]):
            check_kept(selected(twin, data, window, 61, sel), rec_h, bases, sel, (window, sel))
    assert n_multi >= 2


def small_big_small():
    """small, 200 000 bases, small: the large record spans many windows and many cells, a small one lies directly in front of it"""
    rng = random.Random(51)
    return S.sam([S.rec(b"s", b"AC"), S.rec(b"big", S._seq(rng, 200000, b"ACGTN"), qual=b"*"), S.rec(b"t", b"GGA")])


def test_small_record_in_front_of_a_large_one(twin, host):
    """a record of 200 KB over many windows between two small ones, chosen and not chosen"""
    data = small_big_small()
    rec_h = host(data)[1]
    assert [len(s) for _, s in rec_h] == [2, 200000, 3]
    for window, piece in ((64, 3001), (64, 61), (3001, 3001)):
        rc, out = census(twin, data, window, piece)
        assert rc == OK and out[:2] == [3, 200005] and out[3] >= 2, (window, out)
        for sel in ([], [0], [1], [2], [0, 2], [0, 1], [1, 2], [0, 1, 2]):
            check_kept(selected(twin, data, window, piece, sel), rec_h, 200005, sel, (window, piece, sel))


def test_bad_record_in_the_third_window(twin, host):
    """two windows are proven before the bad line arrives -- a mapped record, a line of nine tabs, a bad flag: the census and the
    selection are unproven, nothing is kept"""
    rng = random.Random(53)
    lines = [S.rec(b"m%d" % i, S._seq(rng, 30)) for i in range(12)]
    window = 200
    k = next(i for i in range(12) if len(S.HD) + sum(len(r) for r in lines[:i]) > 2 * window)
    rc, out = census(twin, S.sam(lines), window, window)
    assert rc == OK and out[0] == 12 and out[3] >= 3
    nine = b"\t".join([b"nine", b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0", b"ACGT"]) + b"\n"
    for line in (S.rec(b"mapped", S._seq(rng, 30), flag=b"0"), nine, S.rec(b"fx", b"ACGT", flag=b"4x")):
        bad = S.sam(lines[:k] + [line] + lines[k:])
        assert host(bad)[0] != 0
        assert census(twin, bad, window, window) == (UNPROVEN, [0, 0, 0, 0])
        assert selected(twin, bad, window, window, [0, 1])[0] == UNPROVEN        # (records of the first window, which was proven)


def test_arguments(twin):
    out = (C.c_uint64 * 4)()
    assert twin.sam_twin_census(S.HD, len(S.HD), 64, 0, C.byref(out)) == -1              # a piece has bytes
    assert twin.sam_twin_selected(S.HD, len(S.HD), 64, 0, None, 0) == -1
