"""The seek map of unaligned SAM and its mapped second pass without a GPU (lrge_amd/csrc/fx_seek.h): the host
twin makes the map of a SAM text through the point rule the device uses (a record starts at the first byte of its line), plans a
selection with the planner FASTA / FASTQ use, builds the sub-text of the runs -- whole lines, a SAM text without a header -- and
scans it through the windows.  The reference of the points is the line walk of the test itself; the reference of the records is
the host parser (lrge_hip_read_records).  The condition of the design is checked, not hoped for: over the well-formed corpus no
sub-text is unproven, and every sub-text holds exactly the planner's records."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sam_corpus as S
from test_sam_twin import OK, UNPROVEN
from test_sam_window_twin import WINDOWS
from test_sam_window_twin import host   # noqa: F401  (fixture)
from test_sam_select_twin import INVALID, bind as bind_select, census, check_kept, read_kept, selected, small_big_small, window_records
from test_sam_select_twin import twin as _select_twin   # noqa: F401  (fixture)
from test_fastx_seek_twin import bgzf_table, seek_selections

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def bind(L):
    """the prototypes of the twin's map entries (the GPU suite binds them too)"""
    bind_select(L)
    L.sam_twin_census_map.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64 * 4)]
    L.sam_twin_map_points.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.sam_twin_map_points.restype = C.c_uint64
    L.sam_twin_seek_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64 * 4)]
    L.sam_twin_plan_runs.argtypes = [C.c_void_p, C.c_uint64]
    L.sam_twin_plan_runs.restype = C.c_uint64
    L.sam_twin_plan_sel.argtypes = [C.c_void_p]
    L.sam_twin_mapped.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    return L


@pytest.fixture(scope="module")
def twin(_select_twin):
    return bind(_select_twin)


def record_starts(data):
    """the offset of the first byte of every record line, from the bytes alone: lines end at line feeds, one trailing CR is
    stripped, an empty line and one that starts with '@' carry no record"""
    starts, o = [], 0
    for line in data.split(b"\n"):
        body = line[:-1] if line.endswith(b"\r") else line
        if body and body[:1] != b"@":
            starts.append(o)
        o += len(line) + 1
    return starts


def reference_points(starts, stride):
    """[(ordinal, text offset)]: the first record start of every cell that holds one"""
    pts, cell = [], None
    for i, s in enumerate(starts):
        if s // stride != cell:
            pts.append((i, s))
            cell = s // stride
    return pts


def strides_for(data):
    return [1, 64, 257, 4096, len(data) + 1]


def census_map(L, data, window, piece, stride):
    """(verdict, counts, [(ordinal, offset)]) of the twin's census with a map"""
    out = (C.c_uint64 * 4)()
    rc = L.sam_twin_census_map(data, len(data), window, piece, stride, C.byref(out))
    if rc != OK:
        return rc, list(out), None
    k = L.sam_twin_map_points(None, None, 0)
    a, b = np.zeros(max(1, k), dtype=np.uint64), np.zeros(max(1, k), dtype=np.uint64)
    L.sam_twin_map_points(a.ctypes.data, b.ctypes.data, k)
    return rc, list(out), list(zip(a[:k].tolist(), b[:k].tolist()))


def seek_plan(L, sel, table=None, file_len=0):
    """(verdict, (runs, text bytes, file bytes, blocks), [(ord0, n_rec, t0, t1)], renumbered selection) of the last map"""
    a = np.ascontiguousarray(sel, dtype=np.uint32)
    out = (C.c_uint64 * 4)()
    cl, isz = table if table is not None else (np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32))
    rc = L.sam_twin_seek_plan(cl.ctypes.data, isz.ctypes.data, len(cl) if table is not None else 0, file_len, a.ctypes.data if a.size else None, a.size, C.byref(out))
    if rc != OK:
        return rc, None, None, None
    k = L.sam_twin_plan_runs(None, 0)
    runs = np.zeros((max(1, k), 4), dtype=np.uint64)
    L.sam_twin_plan_runs(runs.ctypes.data, k)
    re_sel = np.zeros(max(1, a.size), dtype=np.uint32)
    L.sam_twin_plan_sel(re_sel.ctypes.data)
    return rc, tuple(int(x) for x in out), [tuple(r) for r in runs[:k].tolist()], re_sel[:a.size].tolist()


def mapped(L, data, window, piece, sel):
    """(verdict, [(name, sequence)], store, select stats) of the twin's mapped pass on the last map, as `selected` reads a run"""
    a = np.ascontiguousarray(sel, dtype=np.uint32)
    rc = L.sam_twin_mapped(data, len(data), window, piece, a.ctypes.data if a.size else None, a.size)
    if rc != OK:
        assert L.sam_twin_windowed_count() == 0 and L.sam_twin_windowed_store(None) == 0
        return rc, None, None, None
    return (rc,) + read_kept(L, data)


def test_points_are_first_record_starts(twin, host):
    """every well-formed case: the points ascend strictly in ordinal and offset, every point is the first byte of a record line, the
    first of its cell, and the first point is record 0 -- whatever the window and the piece"""
    n_runs = n_many = 0
    for name, data in S.well_formed():
        rec_h = host(data)[1]
        starts = record_starts(data)
        assert len(starts) == len(rec_h), name
        bases = sum(len(s) for _, s in rec_h)
        for stride in strides_for(data):
            want = reference_points(starts, stride)
            assert not want or want[0] == (0, starts[0])
            assert all(a[0] < b[0] and a[1] < b[1] and a[1] // stride < b[1] // stride for a, b in zip(want, want[1:]))
            for window, piece in ((64, 61), (257, 1), (3001, 3001), (20000, 61), (len(data) + 1, 4096)):
                rc, out, pts = census_map(twin, data, window, piece, stride)
                assert rc == OK, (name, stride, window, piece)      # a condition, not a hope
                assert out[:3] == [len(rec_h), bases, len(data)], (name, stride, window, piece, out)
                assert pts == want, (name, stride, window, piece)
                n_runs += 1
                n_many += len(pts) > 3
    assert n_runs > 800 and n_many > 400                          # (not vacuous: many maps have several points)


def test_mapped_equals_selected(twin, host):
    """every well-formed case, stride and window: each selection through the map gives what the selecting twin gives on the whole
    text, which is the host's subset; zero unproven verdicts"""
    n_sel = n_points = n_merge = n_far = 0
    for name, data in S.well_formed():
        rec_h = host(data)[1]
        bases = sum(len(s) for _, s in rec_h)
        for stride in strides_for(data):
            for window, piece in ((64, 61), (257, 1), (3001, 3001), (20000, 20000)):
                if piece == 1 and len(data) > 20000:
                    piece = 61
                rc, out0 = census(twin, data, window, piece)
                assert rc == OK
                per_window = window_records(twin)
                rc, out, pts = census_map(twin, data, window, piece, stride)
                assert rc == OK and out == out0, (name, stride, window)                     # the map changes no count
                for kind, sel in seek_selections(len(rec_h), per_window, pts).items():
                    what = (name, stride, window, kind)
                    got = mapped(twin, data, window, piece, sel)
                    check_kept(got, rec_h, bases, sel, what)
                    if stride in (64, 4096) and window == 64:
                        assert got == selected(twin, data, window, piece, sel), what
                    n_sel += 1
                    n_points += kind == "around the points"
                    n_merge += kind == "neighbouring cells"
                    n_far += kind == "far apart"
    assert n_sel > 3000 and n_points > 300 and n_merge > 150 and n_far > 100


def plan_text_bytes(pts, sel, text_len):
    """the text bytes the runs of a selection bring, from the points alone: the cells' stretches that hold a chosen ordinal, once each"""
    ends = [o for _, o in pts[1:]] + [text_len]
    hit = {max(i for i, (o, _) in enumerate(pts) if o <= r) for r in sel}
    return sum(ends[i] - pts[i][1] for i in hit)


def test_planner_on_plain_text_and_bgzf_blocks(twin, host):
    """the plan's statistics on the plain text and on a BGZF table of 3 000-byte blocks with the empty end block: only the blocks a
    run touches, each once; lines span blocks, and a run that ends exactly where a block starts leaves that block out"""
    import bgzf_writer as W
    rng = __import__("random").Random(57)
    lines = [S.rec(b"r%03d" % i, S._seq(rng, 400 + (i % 7))) for i in range(80)]
    n = len(lines)
    for pad in range(3000):                     # pad the header until some record line starts at a multiple of 3000: found, not assumed
        data = S.sam(lines, S.HD + b"@CO\t" + b"x" * pad + b"\n")
        starts = record_starts(data)
        if any(s % 3000 == 0 for s in starts[2:-2]):
            break
    rec_h = host(data)[1]
    assert len(rec_h) == n == len(starts) and any(s % 3000 == 0 for s in starts[2:-2])
    comp = W.bgzf_compress(data, block=3000)
    table = bgzf_table(comp)
    assert int(table[1].sum()) == len(data) and int(table[0].sum()) == len(comp) and table[1][-1] == 0     # the empty end block
    o = np.concatenate([[0], np.cumsum(table[1])])
    rc, _, pts = census_map(twin, data, 3001, 3001, 64)
    assert rc == OK and pts == reference_points(starts, 64) and len(pts) == n
    # the plain text: one ordinal is one run from its point to the next; file bytes are text bytes, no blocks
    rc, st, runs, rs = seek_plan(twin, [5])
    assert rc == OK and runs == [(5, 1, starts[5], starts[6])] and rs == [0] and st == (1, starts[6] - starts[5], starts[6] - starts[5], 0)
    rc, st, runs, rs = seek_plan(twin, [5, 6, 40, n - 1])
    assert runs == [(5, 2, starts[5], starts[7]), (40, 1, starts[40], starts[41]), (n - 1, 1, starts[n - 1], len(data))] and rs == [0, 1, 2, 3]
    assert st == (3, sum(r[3] - r[2] for r in runs), sum(r[3] - r[2] for r in runs), 0)
    # everything: one run from the first record line to the end -- the header is not brought --, every block of it but none twice
    rc, st, runs, _ = seek_plan(twin, list(range(n)), table, len(comp))
    first_blk = starts[0] // 3000
    assert rc == OK and st == (1, len(data) - starts[0], int(table[0][first_blk:].sum()), len(table[0]) - first_blk)

    def touched(runs):
        return sorted({b for r in runs for b in range(len(table[0])) if table[1][b] and o[b] < r[3] and o[b + 1] > r[2]})
    # a run that ends exactly at a block start: the block behind it is not read
    whole = next(i for i in range(2, n - 2) if starts[i] % 3000 == 0)
    rc, st, runs, _ = seek_plan(twin, [whole - 1], table, len(comp))
    assert runs == [(whole - 1, 1, starts[whole - 1], starts[whole])]
    t = touched(runs)
    assert t[-1] == starts[whole] // 3000 - 1 and st == (1, starts[whole] - starts[whole - 1], int(table[0][t].sum()), len(t))
    # a line that spans blocks brings both; two runs in one block count it once
    span = next(i for i in range(n - 1) if starts[i] // 3000 != (starts[i + 1] - 1) // 3000)
    rc, st, runs, _ = seek_plan(twin, [span], table, len(comp))
    t = touched(runs)
    assert len(t) == 2 and st == (1, starts[span + 1] - starts[span], int(table[0][t].sum()), 2)
    pair = next(i for i in range(n - 3) if starts[i] // 3000 == (starts[i + 3] - 1) // 3000)
    rc, st, runs, _ = seek_plan(twin, [pair, pair + 2], table, len(comp))
    assert st[0] == 2 and st[3] == 1 and st[2] == int(table[0][touched(runs)].sum())
    # each of these through the mapped pass: the host's records
    bases = sum(len(s) for _, s in rec_h)
    for sel in ([whole - 1], [whole], [span], [pair, pair + 2], [0, n - 1], list(range(n))):
        check_kept(mapped(twin, data, 3001, 3001, sel), rec_h, bases, sel, sel)
    assert seek_plan(twin, [0], table, len(comp) + 1)[0] == INVALID             # a block table of another file


def test_a_cell_that_starts_inside_co_or_empty_lines(twin, host):
    """@CO and empty lines between the records, longer than a cell: a cell that starts inside them gets the next record line as its
    point, and they travel at the end of the run in front of it, where the scan of the sub-text skips them"""
    filler = [b"@CO\t" + b"c" * 150 + b"\n", b"\n" * 90, b"\r\n" * 40 + b"@\n", b"@CO\n\n\n@HD\tagain\n" + b"\n" * 70]
    lines = []
    for i in range(8):
        lines += [S.rec(b"r%d" % i, b"ACGT" * (1 + i % 3)), filler[i % 4]]
    data = S.sam(lines, S.HD + b"\n" * 70)
    rec_h = host(data)[1]
    starts = record_starts(data)
    assert len(rec_h) == 8 == len(starts)
    bases = sum(len(s) for _, s in rec_h)
    for stride in (16, 64):
        assert any(data[c * stride:c * stride + 1] in (b"\n", b"c", b"\r") and (c + 1) * stride <= s for s in starts for c in [s // stride - 1])    # (a cell starts in filler)
        for window, piece in ((64, 1), (257, 61), (len(data) + 1, 4096)):
            rc, out, pts = census_map(twin, data, window, piece, stride)
            assert rc == OK and pts == reference_points(starts, stride) and len(pts) == 8 and pts[0] == (0, starts[0])
            for sel in ([], [0], [3], [7], [2, 3], [0, 4, 7], list(range(8))):
                rc, st, runs, _ = seek_plan(twin, sel)
                assert rc == OK and st[1] == plan_text_bytes(pts, sel, len(data))
                assert all(data[r[2]:r[2] + 1] == b"r" and (r[3] == len(data) or data[r[3] - 1:r[3]] == b"\n") for r in runs)      # whole lines
                check_kept(mapped(twin, data, window, piece, sel), rec_h, bases, sel, (stride, window, sel))


def test_crlf_and_no_final_line_feed(twin, host):
    """CRLF lines, and a text without a final line feed: only the last run ends without one"""
    cases = dict(S.well_formed())
    for name in ("crlf", "crlf_lengths", "final_cr_after_crlf", "no_final_lf", "no_final_lf_empty_quality", "final_cr_line"):
        data = cases[name]
        rec_h = host(data)[1]
        n = len(rec_h)
        bases = sum(len(s) for _, s in rec_h)
        starts = record_starts(data)
        for window, piece in ((64, 1), (257, 61)):
            rc, out, pts = census_map(twin, data, window, piece, 64)
            assert rc == OK and pts == reference_points(starts, 64)
            for sel in ([0], [n - 1], [0, n - 1], [n // 2], list(range(n))):
                rc, st, runs, _ = seek_plan(twin, sel)
                assert all(r[3] == len(data) or data[r[3] - 1:r[3]] == b"\n" for r in runs), (name, sel)
                assert (max(sel) >= pts[-1][0]) == (runs[-1][3] == len(data))      # (the run of the last point's cell reaches the end)
                check_kept(mapped(twin, data, window, piece, sel), rec_h, bases, sel, (name, window, sel))


def test_a_record_of_many_cells_and_windows(twin, host):
    """small, 200 000 bases, small at window 64 and stride 64: no point inside the large record, and none at its start, which lies
    in the first record's cell: only [2] brings a small run"""
    data = small_big_small()
    rec_h = host(data)[1]
    starts = record_starts(data)
    assert starts[0] // 64 == starts[1] // 64                       # (a small record in front of a large one in one cell)
    rc, out, pts = census_map(twin, data, 64, 61, 64)
    assert rc == OK and pts == reference_points(starts, 64) and [p[0] for p in pts] == [0, 2]
    assert pts[-1][1] // 64 - pts[-2][1] // 64 > 3000               # (thousands of cells without a point)
    for sel in ([1], [0, 2], [0, 1, 2], [2], []):
        rc, st, runs, rs = seek_plan(twin, sel)
        assert rc == OK and st[1] == plan_text_bytes(pts, sel, len(data)), (sel, st)
        if sel == [2]:
            assert runs == [(2, 1, starts[2], len(data))] and st[1] < 64
        elif sel:
            assert st[1] > 200000
        check_kept(mapped(twin, data, 64, 61, sel), rec_h, 200005, sel, sel)
    # the corpus's long record behind three reads, at a stride that gives it a cell of its own
    data = dict(S.well_formed())["long_200k"]
    rec_h = host(data)[1]
    bases = sum(len(s) for _, s in rec_h)
    for window, stride in ((64, 64), (3001, 4096), (20000, 257)):
        rc, out, pts = census_map(twin, data, window, 3001, stride)
        assert rc == OK and out[:2] == [7, bases]
        for sel in ([3], [2, 4], [0, 6], list(range(7))):
            check_kept(mapped(twin, data, window, 3001, sel), rec_h, bases, sel, (window, stride, sel))


def test_header_that_ends_the_text(twin, host):
    """no point, no run, an empty handle"""
    for name in ("header_only", "header_no_lf", "header_three_lines"):
        hdr = dict(S.well_formed())[name]
        for window in (4, len(hdr) + 1):
            rc, out, pts = census_map(twin, hdr, window, 1, 64)
            assert rc == OK and out[:3] == [0, 0, len(hdr)] and pts == []
            assert seek_plan(twin, [])[:3] == (OK, (0, 0, 0, 0), [])
            assert mapped(twin, hdr, window, 1, []) == (OK, [], b"", [0, 0, 0, 0])
            assert mapped(twin, hdr, window, 1, [0])[0] == INVALID


def test_refusals(twin, host):
    """a map of another text, an ordinal equal to n, an unsorted list, a text of the same size with a mapped record"""
    cases = dict(S.well_formed())
    data, other = cases["plain_40"], cases["names"]
    n = len(host(data)[1])
    assert census_map(twin, data, 257, 257, 257)[0] == OK
    assert mapped(twin, other, 257, 257, [0])[0] == INVALID
    for sel in ([n], [0, n - 1, n], [5, 3], [0, 4, 4, 9]):
        assert mapped(twin, data, 257, 257, sel)[0] == INVALID, sel
        assert seek_plan(twin, sel)[0] == INVALID, sel
    assert mapped(twin, data, 257, 257, [n - 1])[0] == OK
    # the same size, but the chosen run's record is mapped now, or lost a tab: never other records
    starts = record_starts(data)
    for edit in (lambda b, s: b.__setitem__(s + len(b"read3\t"), ord("0")), lambda b, s: b.__setitem__(s + len(b"read3"), ord(" "))):
        bad = bytearray(data)
        edit(bad, starts[3])
        assert host(bytes(bad))[0] != 0
        assert mapped(twin, bytes(bad), 257, 257, [3])[0] == UNPROVEN
    out = (C.c_uint64 * 4)()
    assert twin.sam_twin_census_map(data, len(data), 64, 1, 0, C.byref(out)) == -1         # a stride has bytes
    for name, text, _ in S.unproven():
        for window in WINDOWS:
            assert census_map(twin, text, window, 61, 257)[0] == UNPROVEN, (name, window)


def test_abi_has_the_flag():
    from lrge_amd import _ffi
    assert re.search(r"#define\s+LRGE_GPU_INGEST_SELECT_SAM\s+4096\b", open(os.path.join(ROOT, "include", "lrge_hip.h")).read()) and _ffi.GPU_INGEST_SELECT_SAM == 4096
    assert re.search(r"LRGE_GPU_INGEST_SELECT_SAM: c_int = 4096;", open(os.path.join(ROOT, "integration", "liblrge_hip_shim.rs")).read())
    assert "LRGE_GPU_INGEST_SELECT_SAM" in open(os.path.join(ROOT, "include", "lrge_hip.hpp")).read()
    assert "LRGE_GPU_INGEST_SELECT_SAM" in open(os.path.join(ROOT, "tools", "lrge_hip_cli.cpp")).read()
    flags = [v for k, v in vars(_ffi).items() if k.startswith(("GPU_INGEST_", "GPU_INFLATE_")) and isinstance(v, int)]
    assert len(flags) == len(set(flags)) and all(v & (v - 1) == 0 for v in flags)         # one bit each, none shared
