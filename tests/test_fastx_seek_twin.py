"""The seek map and the mapped second pass without a GPU (lrge_amd/csrc/fx_seek.h): the host twin makes the
map of a text through the point rule the device uses, plans a selection with the planner the device uses, builds the sub-text
of the runs and scans it through the windows -- against a reference of the points the test computes from the text itself, and
against the host parser's subset (lrge_hip_read_records).  The condition of the whole design is checked, not hoped for: over
the well-formed corpus no sub-text is unproven, and every sub-text holds exactly the planner's records."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import fastx_corpus as F
from test_fastx_select_twin import FxRec, OK, UNPROVEN, INVALID, selected, selections, window_records
from test_fastx_select_twin import host, twin as _select_twin   # noqa: F401  (fixtures)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ["lrge_hip_reads_census_map", "lrge_hip_reads_census_map_mem", "lrge_hip_read_map_free", "lrge_hip_read_map_stats", "lrge_hip_read_map_points",
       "lrge_hip_reads_open_mapped", "lrge_hip_reads_open_mapped_mem", "lrge_hip_reads_seek_stats"]


def bind(L):
    """the prototypes of the twin's map entries (the GPU suite binds them too)"""
    L.fastx_twin_census.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64 * 4)]
    L.fastx_twin_census_map.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64 * 4)]
    L.fastx_twin_map_points.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.fastx_twin_map_points.restype = C.c_uint64
    L.fastx_twin_seek_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64 * 4)]
    L.fastx_twin_plan_runs.argtypes = [C.c_void_p, C.c_uint64]
    L.fastx_twin_plan_runs.restype = C.c_uint64
    L.fastx_twin_plan_sel.argtypes = [C.c_void_p]
    L.fastx_twin_mapped.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    L.fastx_twin_windowed_cuts.argtypes = [C.c_void_p, C.c_uint64]
    L.fastx_twin_windowed_cuts.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def twin(_select_twin):
    return bind(_select_twin)


def reference_points(text, n_rec, stride):
    """[(ordinal, text offset)] by the rule of the issue, from the text alone: a FASTA record starts at a '>' at offset 0 or behind a
    line feed, FASTQ record i at the start of line l0 + 4i (l0: the first line that is not empty); the first start of every cell"""
    if not n_rec:
        return []
    if text.lstrip(b"\r\n")[:1] == b">":
        starts = [m.start() for m in re.finditer(rb"(?:^|(?<=\n))>", text)]
    else:
        line_at, lines = [0], text.split(b"\n")
        for ln in lines[:-1]:
            line_at.append(line_at[-1] + len(ln) + 1)
        l0 = next(i for i, ln in enumerate(lines) if ln.rstrip(b"\r"))
        starts = [line_at[l0 + 4 * i] for i in range(n_rec)]
    assert len(starts) == n_rec
    pts, cell = [], None
    for i, s in enumerate(starts):
        if s // stride != cell:
            pts.append((i, s))
            cell = s // stride
    return pts


def census_map(L, text, window, piece, stride, tile=64):
    """(verdict, counts, [(ordinal, offset)]) of the twin's census with a map"""
    out = (C.c_uint64 * 4)()
    rc = L.fastx_twin_census_map(text, len(text), tile, window, piece, stride, C.byref(out))
    if rc != OK:
        return rc, list(out), None
    k = L.fastx_twin_map_points(None, None, 0)
    a, b = np.zeros(max(1, k), dtype=np.uint64), np.zeros(max(1, k), dtype=np.uint64)
    L.fastx_twin_map_points(a.ctypes.data, b.ctypes.data, k)
    return rc, list(out), list(zip(a[:k].tolist(), b[:k].tolist()))


def bgzf_table(data):
    """(member lengths, text sizes) of a BGZF file, by its BC subfields"""
    c_len, isize, off = [], [], 0
    while off < len(data):
        xlen = struct.unpack_from("<H", data, off + 10)[0]
        x, bsize = off + 12, None
        while x < off + 12 + xlen:
            si1, si2, slen = struct.unpack_from("<BBH", data, x)
            if (si1, si2, slen) == (66, 67, 2):
                bsize = struct.unpack_from("<H", data, x + 4)[0]
            x += 4 + slen
        c_len.append(bsize + 1)
        isize.append(struct.unpack_from("<I", data, off + bsize + 1 - 4)[0])
        off += bsize + 1
    assert off == len(data)
    return np.array(c_len, dtype=np.uint32), np.array(isize, dtype=np.uint32)


def seek_plan(L, sel, table=None, file_len=0):
    """(verdict, (runs, text bytes, file bytes, blocks), [(ord0, n_rec, t0, t1)], renumbered selection) of the last map"""
    a = np.ascontiguousarray(sel, dtype=np.uint32)
    out = (C.c_uint64 * 4)()
    cl, isz = table if table is not None else (np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32))
    rc = L.fastx_twin_seek_plan(cl.ctypes.data, isz.ctypes.data, len(cl) if table is not None else 0, file_len, a.ctypes.data if a.size else None, a.size, C.byref(out))
    if rc != OK:
        return rc, None, None, None
    k = L.fastx_twin_plan_runs(None, 0)
    runs = np.zeros((max(1, k), 4), dtype=np.uint64)
    L.fastx_twin_plan_runs(runs.ctypes.data, k)
    re_sel = np.zeros(max(1, a.size), dtype=np.uint32)
    L.fastx_twin_plan_sel(re_sel.ctypes.data)
    return rc, tuple(int(x) for x in out), [tuple(r) for r in runs[:k].tolist()], re_sel[:a.size].tolist()


def mapped(L, text, window, piece, sel, tile=64):
    """(verdict, [(name, sequence)], store, select stats) of the twin's mapped pass on the last map, as `selected` reads a run"""
    a = np.ascontiguousarray(sel, dtype=np.uint32)
    rc = L.fastx_twin_mapped(text, len(text), tile, window, piece, a.ctypes.data if a.size else None, a.size)
    if rc != OK:
        return rc, None, None, None
    n = L.fastx_twin_windowed_count()
    tab = (FxRec * max(1, n))()
    L.fastx_twin_windowed_table(tab)
    ss = (C.c_uint64 * 4)()
    L.fastx_twin_select_stats(C.byref(ss))
    out, at, buf = [], 0, C.create_string_buffer(max(1, max((tab[i].seq_len for i in range(n)), default=0)))
    for i in range(n):
        r = tab[i]
        assert r.name_off + r.name_len <= len(text) and r.seq_off == at and r.seq_span == r.seq_len
        assert L.fastx_twin_windowed_seq(i, buf) == r.seq_len
        out.append((text[r.name_off:r.name_off + r.name_len], buf.raw[:r.seq_len]))
        at += r.seq_len
    store = C.create_string_buffer(max(1, at))
    assert L.fastx_twin_windowed_store(store, at) == at
    return rc, out, store.raw[:at], list(ss)


def strides_for(text):
    return [1, 64, 512, 3000, 70000, len(text) + 1]


def seek_selections(n, per_window, pts):
    """the selections of the select-twin test, the records on either side of every point, and two records in neighbouring cells"""
    sels = selections(n, per_window)
    if n:
        sels["around the points"] = sorted({o for o, _ in pts} | {o - 1 for o, _ in pts if o} | {n - 1})
    if len(pts) >= 3:
        sels["neighbouring cells"] = [pts[1][0], pts[2][0]]
    if len(pts) >= 5:
        sels["far apart"] = [pts[0][0], pts[len(pts) // 2][0], pts[-1][0]]
    return sels


def test_points_equal_the_reference(twin, host):
    """every well-formed case: the twin's points are those the rule gives on the text, whatever the window and the piece"""
    n_runs = n_many = 0
    for name, text in F.well_formed():
        rec_h = host(text)[1]
        bases = sum(len(s) for _, s in rec_h)
        for stride in strides_for(text):
            want = reference_points(text, len(rec_h), stride)
            assert not want or want[0][0] == 0
            assert all(a[0] < b[0] and a[1] < b[1] for a, b in zip(want, want[1:]))
            for window in (64, 3001, 20000, len(text) + 1):
                for piece in (1, 7, 61, 4096):
                    rc, out, pts = census_map(twin, text, window, piece, stride)
                    assert rc == OK, (name, stride, window, piece)
                    assert out[:3] == [len(rec_h), bases, len(text)], (name, stride, window, piece, out)
                    assert pts == want, (name, stride, window, piece)
                    n_runs += 1
                    n_many += len(pts) > 3
    assert n_runs > 3000 and n_many > 800


def test_mapped_equals_host_subset(twin, host):
    """every well-formed case, stride and window: each selection through the map gives the host's records; zero unproven verdicts"""
    n_sel = n_points = n_merge = 0
    for name, text in F.well_formed():
        rec_h = host(text)[1]
        bases = sum(len(s) for _, s in rec_h)
        for stride in strides_for(text):
            for window in (64, 3001, len(text) + 1):
                piece = 61 if window == 64 else 4096
                out0 = (C.c_uint64 * 4)()
                assert twin.fastx_twin_census(text, len(text), 64, window, piece, C.byref(out0)) == OK
                per_window = window_records(twin)
                rc, out, pts = census_map(twin, text, window, piece, stride)
                assert rc == OK and list(out) == list(out0), (name, stride, window)         # the map changes no count
                for kind, sel in seek_selections(len(rec_h), per_window, pts).items():
                    what = (name, stride, window, kind)
                    rc, rec, store, ss = mapped(twin, text, window, piece, sel)
                    assert rc == OK, (what, rc)                     # a condition, not a hope
                    want = [rec_h[i] for i in sel]
                    assert rec == want, what
                    assert store == b"".join(s for _, s in want), what
                    assert ss == [len(rec_h), len(sel), bases, sum(len(s) for _, s in want)], (what, ss)
                    n_sel += 1
                    n_points += kind == "around the points"
                    n_merge += kind == "neighbouring cells"
    assert n_sel > 5000 and n_points > 400 and n_merge > 100


def test_mapped_at_the_tiles_of_the_device(twin, host):
    """the cases, windows and strides of the GPU suite at the device's tile"""
    cases = dict(F.well_formed())
    for name in ("fq_big", "fa_big_w60_crlf", "fq_empty_seqs", "fq_size_4096"):
        text, rec_h = cases[name], host(cases[name])[1]
        for window in (3001, 20000):
            for stride in (512, 3000, 70000, 1 << 20):
                rc, out, pts = census_map(twin, text, window, window, stride, tile=4096)
                assert rc == OK and pts == reference_points(text, len(rec_h), stride), (name, window, stride)
                for kind, sel in seek_selections(len(rec_h), [len(rec_h)], pts).items():
                    rc, rec, _, ss = mapped(twin, text, window, window, sel, tile=4096)
                    assert rc == OK and rec == [rec_h[i] for i in sel] and ss[:2] == [len(rec_h), len(sel)], (name, window, stride, kind)


def test_planner(twin, host):
    """runs merge when they touch; the last run reaches the text end; a record spanning many cells is one run; the renumbered
    selection indexes the right records; the runs' record counts add up to what the scan of the sub-text sees"""
    text = dict(F.well_formed())["fq_big"]
    rec_h = host(text)[1]
    n = len(rec_h)
    rc, _, pts = census_map(twin, text, 3001, 4096, 3000)
    assert rc == OK and len(pts) > 10
    starts = dict(pts)

    def end_of(i):                                                  # where the run of point i ends
        return (pts[i + 1][0], pts[i + 1][1]) if i + 1 < len(pts) else (n, len(text))
    # one ordinal: its own run, from its point to the next
    rc, st, runs, rs = seek_plan(twin, [pts[3][0]])
    assert rc == OK and runs == [(pts[3][0], end_of(3)[0] - pts[3][0], pts[3][1], end_of(3)[1])] and rs == [0]
    assert st == (1, runs[0][3] - runs[0][2], runs[0][3] - runs[0][2], 0)
    # the record in front of a point belongs to the run of the point before
    if pts[4][0] - 1 > pts[3][0]:
        rc, st, runs, rs = seek_plan(twin, [pts[4][0] - 1])
        assert runs == [(pts[3][0], pts[4][0] - pts[3][0], pts[3][1], pts[4][1])] and rs == [pts[4][0] - 1 - pts[3][0]]
    # two runs that touch merge; two that do not, do not
    rc, st, runs, rs = seek_plan(twin, [pts[3][0], pts[4][0]])
    assert st[0] == 1 and runs == [(pts[3][0], end_of(4)[0] - pts[3][0], pts[3][1], end_of(4)[1])] and rs == [0, pts[4][0] - pts[3][0]]
    rc, st, runs, rs = seek_plan(twin, [pts[3][0], pts[5][0]])
    assert st[0] == 2 and runs[0][3] == pts[4][1] and runs[1][2] == pts[5][1] and rs == [0, runs[0][1]]
    # the last run reaches the end of the text
    rc, st, runs, rs = seek_plan(twin, [0, n - 1])
    assert runs[-1][3] == len(text) and runs[-1][0] + runs[-1][1] == n and runs[0][0] == 0 and runs[0][2] == starts[0]
    # every selection: the runs are disjoint and ascending, whole records, and the renumbered selection names the same records
    for kind, sel in seek_selections(n, [n], pts).items():
        rc, st, runs, rs = seek_plan(twin, sel)
        assert rc == OK and st[0] == len(runs) and st[1] == sum(r[3] - r[2] for r in runs) == st[2] and st[3] == 0, kind
        assert all(a[3] < b[2] and a[0] + a[1] < b[0] for a, b in zip(runs, runs[1:])), kind
        sub = b"".join(text[r[2]:r[3]] for r in runs)
        sub_h = host(sub)[1] if sub else []
        assert len(sub_h) == sum(r[1] for r in runs), kind          # what the scan of the sub-text sees
        assert [sub_h[j] for j in rs] == [rec_h[i] for i in sel], kind
    # a record that spans many cells has no point inside: one run holds it whole
    big = F.fastq_text([(b"s", b"AC"), (b"big", b"ACGTN" * 4000), (b"t", b"GG")])
    rc, _, pts = census_map(twin, big, 64, 61, 64)
    assert rc == OK and [o for o, _ in pts] == [0, 2] and pts[1][1] // 64 > 600
    rc, st, runs, rs = seek_plan(twin, [1])
    assert runs == [(0, 2, 0, pts[1][1])] and rs == [1]
    rc, rec, _, ss = mapped(twin, big, 64, 61, [1])
    assert rc == OK and rec == [(b"big", b"ACGTN" * 4000)] and ss[:2] == [3, 1]
    rc, st, runs, rs = seek_plan(twin, [2])
    assert runs == [(2, 1, pts[1][1], len(big))] and st[1] < 64


def test_planner_on_bgzf_blocks(twin, host):
    """the same plan on the text in BGZF blocks: only the blocks a run touches, each once; all of them when everything is chosen"""
    import bgzf_writer as W
    text = dict(F.well_formed())["fq_big"]
    n = len(host(text)[1])
    data = W.bgzf_compress(text, block=3000)
    table = bgzf_table(data)
    assert int(table[1].sum()) == len(text) and int(table[0].sum()) == len(data)
    rc, _, pts = census_map(twin, text, 3001, 4096, 512)
    rc, st, runs, _ = seek_plan(twin, list(range(n)), table, len(data))
    assert rc == OK and st == (1, len(text) - pts[0][1], len(data), len(table[0]))
    rc, st, runs, _ = seek_plan(twin, [pts[len(pts) // 2][0]], table, len(data))
    t0, t1 = runs[0][2], runs[0][3]
    o = np.concatenate([[0], np.cumsum(table[1])])
    touched = [b for b in range(len(table[0])) if o[b] < t1 and o[b + 1] > t0]
    assert st == (1, t1 - t0, int(table[0][touched].sum()), len(touched)) and st[2] < len(data)
    # two runs in one block: the block counts once
    sel = [pts[2][0], pts[4][0]]
    rc, st, runs, _ = seek_plan(twin, sel, table, len(data))
    touched = sorted({b for r in runs for b in range(len(table[0])) if o[b] < r[3] and o[b + 1] > r[2]})
    assert st[0] == 2 and st[3] == len(touched) and st[2] == int(table[0][touched].sum())
    assert seek_plan(twin, [0], table, len(data) + 1)[0] == INVALID          # a block table of another file


def test_refusals(twin, host):
    """a map of another text, an ordinal equal to n, an unsorted list"""
    cases = dict(F.well_formed())
    text, other = cases["fq_big"], cases["fa_big_w60_crlf"]
    n = len(host(text)[1])
    assert census_map(twin, text, 3001, 4096, 512)[0] == OK
    assert mapped(twin, other, 3001, 4096, [0])[0] == INVALID
    for sel in ([n], [0, n - 1, n], [5, 3], [0, 4, 4, 9]):
        assert mapped(twin, text, 3001, 4096, sel)[0] == INVALID, sel
        assert seek_plan(twin, sel)[0] == INVALID, sel
        assert twin.fastx_twin_windowed_count() == 0
    assert mapped(twin, text, 3001, 4096, [n - 1])[0] == OK
    # a text of the same size that is not the one the map was made of: never other records
    shifted = text[1:] + b"\n"
    rc, rec, _, _ = mapped(twin, shifted, 3001, 4096, [3])
    assert rc == UNPROVEN or rec == [host(shifted)[1][3]]
    out = (C.c_uint64 * 4)()
    assert twin.fastx_twin_census_map(b">a\nA\n", 5, 64, 64, 1, 0, C.byref(out)) == -1   # a stride has bytes


def test_abi_has_the_seek_map():
    from lrge_amd import _ffi
    L = _ffi.lib()
    hdr = open(os.path.join(ROOT, "include", "lrge_hip.h")).read()
    for s in NEW:
        assert s in _ffi.EXPORTS and hasattr(L, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    for cite in ("count_records", "twoset.rs", "ava.rs", "DESIGN section 24"):
        assert cite in hdr


def test_new_kernels_resources(tmp_path):
    """k_fx_runs copies with the helper of fx_copy_bases: no scratch, no spills, no LDS; k_fx_seek likewise"""
    import subprocess
    src = tmp_path / "k.hip"
    src.write_text('#include "%s"\n' % os.path.join(ROOT, "lrge_amd", "csrc", "k_fastx.h"))
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-o", str(tmp_path / "k.o"), str(src),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    txt = r.stderr
    for k in ("k_fx_runs", "k_fx_seek"):
        i = txt.index("Function Name: _Z%d%s" % (len(k), k))
        block = txt[i:i + 2000]
        val = lambda key: int(re.search(key + r": (\d+)", block).group(1))   # noqa: E731
        assert val(r"ScratchSize \[bytes/lane\]") == 0, k
        assert val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0, k
        assert val(r"LDS Size \[bytes/block\]") == 0, k
