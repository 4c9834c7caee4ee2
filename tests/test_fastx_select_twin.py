"""The sampled ingest without a GPU (lrge_amd/csrc/fx_window.h FxKeepMode): the host twin runs the window
driver in its two new modes -- the census, which keeps nothing, and the selection, which keeps the records of an ascending list
of ordinals -- against the host parser (lrge_hip_read_records) on the same bytes.  The mode changes what is kept, not what is
proven: the well-formed corpus is proven at every window and piece, the count and the base sum are the host's, read j of a
selection is record sel[j] of the host, the store is dense, and the counts say what was seen and kept."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fastx_corpus as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OK, UNPROVEN, INVALID = 0, 1, -2
PIECES = [1, 7, 61, 4096]
CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_char), C.c_uint64, C.POINTER(C.c_char), C.c_uint64)
NEW = ["lrge_hip_reads_census", "lrge_hip_reads_census_mem", "lrge_hip_reads_open_selected", "lrge_hip_reads_open_selected_mem", "lrge_hip_reads_select_stats"]


def windows_for(text):
    n = len(text)
    return sorted({1, 17, 64, 257, 1000, 4096, max(1, n - 1), max(1, n), n + 1})


class FxRec(C.Structure):
    _fields_ = [("name_off", C.c_uint64), ("seq_off", C.c_uint64), ("seq_span", C.c_uint64), ("name_len", C.c_uint32), ("seq_len", C.c_uint32)]


@pytest.fixture(scope="module")
def twin():
    from lrge_amd import build as B
    L = C.CDLL(B.build_fastx_twin())
    L.fastx_twin_census.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64 * 4)]
    L.fastx_twin_selected.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    L.fastx_twin_select_stats.argtypes = [C.POINTER(C.c_uint64 * 4)]
    L.fastx_twin_windowed_count.restype = C.c_uint64
    L.fastx_twin_windowed_table.argtypes = [C.c_void_p]
    L.fastx_twin_windowed_stats.argtypes = [C.POINTER(C.c_uint64 * 4)]
    L.fastx_twin_windowed_seq.argtypes = [C.c_uint64, C.c_char_p]
    L.fastx_twin_windowed_seq.restype = C.c_uint64
    L.fastx_twin_windowed_store.argtypes = [C.c_char_p, C.c_uint64]
    L.fastx_twin_windowed_store.restype = C.c_uint64
    L.fastx_twin_windowed_cuts.argtypes = [C.c_void_p, C.c_uint64]
    L.fastx_twin_windowed_cuts.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """text -> (rc, [(name, sequence)], message) of the host parser, computed once per text"""
    from lrge_amd import _ffi
    L = _ffi.lib()
    L.lrge_hip_read_records.argtypes = [C.c_char_p, CB, C.c_void_p, C.c_char_p, C.c_uint64]
    p = tmp_path_factory.mktemp("host") / "in.txt"
    seen = {}

    def run(text):
        if text not in seen:
            p.write_bytes(text)
            out = []
            cb = CB(lambda u, n, nl, b, bl: out.append((C.string_at(n, nl), C.string_at(b, bl))))
            err = C.create_string_buffer(512)
            rc = L.lrge_hip_read_records(os.fsencode(str(p)), cb, None, err, 512)
            seen[text] = (rc, out, err.value.decode())
        return seen[text]
    return run


def census(L, text, window, piece, tile=64):
    """(verdict, [records, bases, text bytes, windows]) of the counting twin"""
    out = (C.c_uint64 * 4)()
    rc = L.fastx_twin_census(text, len(text), tile, window, piece, C.byref(out))
    return rc, list(out)


def window_records(L):
    """the records of every window of the run that just ended"""
    k = L.fastx_twin_windowed_cuts(None, 0)
    a = np.zeros(max(1, k), dtype=np.uint64)
    L.fastx_twin_windowed_cuts(a.ctypes.data, k)
    return a[:k].tolist()


def selected(L, text, window, piece, sel, tile=64):
    """(verdict, [(name, sequence)], store, select stats) of the selecting twin"""
    a = np.ascontiguousarray(sel, dtype=np.uint32)
    rc = L.fastx_twin_selected(text, len(text), tile, window, piece, a.ctypes.data if a.size else None, a.size)
    if rc != OK:
        return rc, None, None, None
    n = L.fastx_twin_windowed_count()
    tab = (FxRec * max(1, n))()
    L.fastx_twin_windowed_table(tab)
    st, ss = (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
    L.fastx_twin_windowed_stats(C.byref(st))
    L.fastx_twin_select_stats(C.byref(ss))
    out, at, buf = [], 0, C.create_string_buffer(max(1, max((tab[i].seq_len for i in range(n)), default=0)))
    for i in range(n):
        r = tab[i]
        assert r.name_off + r.name_len <= len(text) and r.seq_off == at and r.seq_span == r.seq_len     # dense, in file order
        assert L.fastx_twin_windowed_seq(i, buf) == r.seq_len
        out.append((text[r.name_off:r.name_off + r.name_len], buf.raw[:r.seq_len]))
        at += r.seq_len
    assert st[1] == at
    store = C.create_string_buffer(max(1, at))
    assert L.fastx_twin_windowed_store(store, at) == at
    return rc, out, store.raw[:at], list(ss)


def selections(n, per_window):
    """the selections of one run over n records whose windows held per_window records each"""
    rng = np.random.default_rng(5)
    sels = {"empty": [], "all": list(range(n)), "every third": list(range(0, n, 3)), "random half": sorted(rng.permutation(n)[:n // 2].tolist())}
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


def check_selection(L, text, rec_h, window, piece, sel, what):
    rc, rec, store, ss = selected(L, text, window, piece, sel)
    assert rc == OK, (what, rc)
    want = [rec_h[i] for i in sel]
    assert rec == want, what
    assert store == b"".join(s for _, s in want), what
    assert ss == [len(rec_h), len(sel), sum(len(s) for _, s in rec_h), sum(len(s) for _, s in want)], (what, ss)


def test_census_equals_host_parser(twin, host):
    """count and base sum of every well-formed case at every window and piece: the host parser's; zero unproven verdicts"""
    n_runs = n_multi = 0
    for name, text in F.well_formed():
        rc_h, rec_h, msg = host(text)
        assert rc_h == 0, (name, msg)
        bases = sum(len(s) for _, s in rec_h)
        for window in windows_for(text):
            for piece in PIECES:
                rc, out = census(twin, text, window, piece)
                assert rc == OK, (name, window, piece, rc)          # the mode changes what is kept, not what is proven
                assert out[:3] == [len(rec_h), bases, len(text)], (name, window, piece, out)
                assert sum(window_records(twin)) == len(rec_h)
                n_runs += 1
                n_multi += out[3] > 1
    assert n_runs > 1000 and n_multi > 400                          # (not vacuous: many runs went through several windows)


@pytest.mark.parametrize("piece", [7, 4096])
def test_selections_equal_host_subset(twin, host, piece):
    """every well-formed case at every window: the empty selection, the first record, the last, all, every third, a random half
    and the records on either side of every cut -- identifiers, sequences, the dense store and the counts"""
    n_sel = n_cut = 0
    for name, text in F.well_formed():
        rec_h = host(text)[1]
        for window in windows_for(text):
            rc, out = census(twin, text, window, piece)
            assert rc == OK, (name, window, piece)
            for kind, sel in selections(len(rec_h), window_records(twin)).items():
                check_selection(twin, text, rec_h, window, piece, sel, (name, window, piece, kind))
                n_sel += 1
                n_cut += kind == "around the cuts"
    assert n_sel > 2000 and n_cut > 100


def test_selection_at_the_tiles_of_the_device(twin, host):
    """the big cases at the device's tile and the windows of the GPU suite"""
    cases = dict(F.well_formed())
    for name in ("fq_big", "fa_big_w60_crlf", "fq_empty_seqs", "fq_size_4096"):
        rec_h = host(cases[name])[1]
        for window in (3001, 20000):
            rc, out = census(twin, cases[name], window, 3000, tile=4096)
            assert rc == OK and out[0] == len(rec_h), (name, window)
            for kind, sel in selections(len(rec_h), window_records(twin)).items():
                rc, rec, store, ss = selected(twin, cases[name], window, 3000, sel, tile=4096)
                assert rc == OK and rec == [rec_h[i] for i in sel] and ss[:2] == [len(rec_h), len(sel)], (name, window, kind)


def test_unproven_list(twin, host):
    """the inputs the scan leaves to the host: unproven in both modes, or the host's count and the host's subset -- never other
    records"""
    for name, text in F.unproven():
        rc_h, rec_h, _ = host(text)
        for window in windows_for(text):
            for piece in (1, 7, 4096):
                rc, out = census(twin, text, window, piece)
                assert rc in (OK, UNPROVEN), (name, window, piece, rc)
                if name in ("sam_header", "bam_magic"):
                    assert rc == UNPROVEN, (name, window, piece)
                if rc == OK:
                    assert rc_h == 0 and out[0] == len(rec_h) and out[1] == sum(len(s) for _, s in rec_h), (name, window, piece)
                sel = list(range(0, len(rec_h) if rc_h == 0 else 0, 2))
                rc2, rec, _, ss = selected(twin, text, window, piece, sel)
                assert rc2 == rc, (name, window, piece, rc, rc2)     # the same windows, the same proof
                if rc2 == OK:
                    assert rec == [rec_h[i] for i in sel], (name, window, piece)


def test_bad_selections(twin, host):
    """descending, repeated and out-of-range ordinals are invalid, at one window and at many; nothing is left behind"""
    text = dict(F.well_formed())["fq_big"]
    n = len(host(text)[1])
    for window in (3001, len(text) + 1):
        for sel in ([5, 3], [0, 4, 4, 9], [n], [0, n - 1, n], [n + 7]):
            assert selected(twin, text, window, 4096, sel)[0] == INVALID, (window, sel)
            assert twin.fastx_twin_windowed_count() == 0
        assert selected(twin, text, window, 4096, [n - 1])[0] == OK
    assert selected(twin, b"", 64, 1, [0])[0] == INVALID and selected(twin, b"", 64, 1, [])[0] == OK


def test_arguments(twin):
    out = (C.c_uint64 * 4)()
    assert twin.fastx_twin_census(b">a\nA\n", 5, 100, 64, 1, C.byref(out)) == -1      # the tile is a multiple of 16
    assert twin.fastx_twin_selected(b">a\nA\n", 5, 64, 64, 0, None, 0) == -1          # a piece has bytes


def test_abi_has_the_selected_ingest():
    from lrge_amd import _ffi
    L = _ffi.lib()
    hdr = open(os.path.join(ROOT, "include", "lrge_hip.h")).read()
    for s in NEW:
        assert s in _ffi.EXPORTS and hasattr(L, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    for cite in ("io.rs:140-145", "lib.rs:189-204", "twoset.rs:122-201"):
        assert cite in hdr


def test_new_kernels_resources(tmp_path):
    """k_fx_keep copies with the body of k_fx_store: no scratch, no spills, and no more LDS than the wave scan needs"""
    import subprocess
    src = tmp_path / "k.hip"
    src.write_text('#include "%s"\n' % os.path.join(ROOT, "lrge_amd", "csrc", "k_fastx.h"))
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-o", str(tmp_path / "k.o"), str(src),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    txt = r.stderr
    for k in ("k_fx_keep", "k_fx_pick", "k_fx_bases"):
        i = txt.index("Function Name: _Z%d%s" % (len(k), k))
        block = txt[i:i + 2000]
        val = lambda key: int(re.search(key + r": (\d+)", block).group(1))   # noqa: E731
        assert val(r"ScratchSize \[bytes/lane\]") == 0, k
        assert val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0, k
        assert val(r"LDS Size \[bytes/block\]") <= 4096, k
