"""The seek map of unaligned BAM and its mapped second pass without a GPU (lrge_amd/csrc/fx_seek.h): the
host twin makes the map of a BAM text through the point rule the device uses (a record starts at its block_size field), plans a
selection with the planner FASTA / FASTQ use, builds the sub-text of the runs -- a record stream without a header -- and scans it
through the windows.  The reference of the points is the record chain walked by the test itself; the reference of the records
is the host parser (lrge_hip_read_records).  The condition of the design is checked, not hoped for: over the well-formed corpus
no sub-text is unproven, and every sub-text holds exactly the planner's records."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import bam_corpus as B
from test_bam_twin import OK, UNPROVEN, STAT_NAMES
from test_bam_window_twin import SEGMENTS, small_big_small
from test_bam_window_twin import host   # noqa: F401  (fixture)
from test_bam_select_twin import INVALID, bind as bind_select, census, check_kept, read_kept, selected, selections, window_records
from test_bam_select_twin import twin as _select_twin   # noqa: F401  (fixture)
from test_fastx_seek_twin import bgzf_table, seek_selections

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def bind(L):
    """the prototypes of the twin's map entries (the GPU suite binds them too)"""
    bind_select(L)
    L.bam_twin_census_map.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64 * 4)]
    L.bam_twin_map_points.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.bam_twin_map_points.restype = C.c_uint64
    L.bam_twin_seek_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64 * 4)]
    L.bam_twin_plan_runs.argtypes = [C.c_void_p, C.c_uint64]
    L.bam_twin_plan_runs.restype = C.c_uint64
    L.bam_twin_plan_sel.argtypes = [C.c_void_p]
    L.bam_twin_mapped.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    return L


@pytest.fixture(scope="module")
def twin(_select_twin):
    return bind(_select_twin)


def record_starts(data):
    """(hdr_end, [the offset of every record's block_size field]) by the BAM layout, from the bytes alone"""
    assert data[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", data, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, o)
    o += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, o)
        o += 4 + l_name + 4
    hdr_end, starts = o, []
    while o < len(data):
        starts.append(o)
        o += 4 + struct.unpack_from("<i", data, o)[0]
    assert o == len(data)
    return hdr_end, starts


def reference_points(starts, stride):
    """[(ordinal, text offset)]: the first record start of every cell that holds one"""
    pts, cell = [], None
    for i, s in enumerate(starts):
        if s // stride != cell:
            pts.append((i, s))
            cell = s // stride
    return pts


def strides_for(data):
    return [1, 36, 257, 4096, len(data) + 1]


def census_map(L, data, S, window, piece, stride):
    """(verdict, counts, [(ordinal, offset)]) of the twin's census with a map"""
    out = (C.c_uint64 * 4)()
    rc = L.bam_twin_census_map(data, len(data), S, window, piece, stride, C.byref(out))
    if rc != OK:
        return rc, list(out), None
    k = L.bam_twin_map_points(None, None, 0)
    a, b = np.zeros(max(1, k), dtype=np.uint64), np.zeros(max(1, k), dtype=np.uint64)
    L.bam_twin_map_points(a.ctypes.data, b.ctypes.data, k)
    return rc, list(out), list(zip(a[:k].tolist(), b[:k].tolist()))


def seek_plan(L, sel, table=None, file_len=0):
    """(verdict, (runs, text bytes, file bytes, blocks), [(ord0, n_rec, t0, t1)], renumbered selection) of the last map"""
    a = np.ascontiguousarray(sel, dtype=np.uint32)
    out = (C.c_uint64 * 4)()
    cl, isz = table if table is not None else (np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32))
    rc = L.bam_twin_seek_plan(cl.ctypes.data, isz.ctypes.data, len(cl) if table is not None else 0, file_len, a.ctypes.data if a.size else None, a.size, C.byref(out))
    if rc != OK:
        return rc, None, None, None
    k = L.bam_twin_plan_runs(None, 0)
    runs = np.zeros((max(1, k), 4), dtype=np.uint64)
    L.bam_twin_plan_runs(runs.ctypes.data, k)
    re_sel = np.zeros(max(1, a.size), dtype=np.uint32)
    L.bam_twin_plan_sel(re_sel.ctypes.data)
    return rc, tuple(int(x) for x in out), [tuple(r) for r in runs[:k].tolist()], re_sel[:a.size].tolist()


def mapped(L, data, S, window, piece, sel):
    """(verdict, [(name, sequence)], store, select stats) of the twin's mapped pass on the last map, as `selected` reads a run"""
    a = np.ascontiguousarray(sel, dtype=np.uint32)
    rc = L.bam_twin_mapped(data, len(data), S, window, piece, a.ctypes.data if a.size else None, a.size)
    if rc != OK:
        assert L.bam_twin_windowed_count() == 0 and L.bam_twin_windowed_store(None) == 0
        return rc, None, None, None
    return (rc,) + read_kept(L, data)


def mapped_bam_stats(L):
    a = (C.c_uint64 * len(STAT_NAMES))()
    L.bam_twin_windowed_bam_stats(a)
    return dict(zip(STAT_NAMES, [int(x) for x in a]))


@pytest.mark.parametrize("S", SEGMENTS)
def test_points_are_first_record_starts(twin, host, S):
    """every well-formed case and bait: the points ascend strictly in ordinal and offset, every point is a record start of the chain,
    the first of its cell, and the first point is record 0 at hdr_end -- whatever the window and the piece"""
    n_runs = n_many = 0
    for name, data in B.well_formed():
        rec_h = host(data)[1]
        hdr_end, starts = record_starts(data)
        assert len(starts) == len(rec_h), name
        bases = sum(len(s) for _, s in rec_h)
        for stride in strides_for(data):
            want = reference_points(starts, stride)
            assert not want or want[0] == (0, hdr_end)
            assert all(a[0] < b[0] and a[1] < b[1] and a[1] // stride < b[1] // stride for a, b in zip(want, want[1:]))
            for window, piece in ((64, 61), (257, 1), (3001, 3001), (20000, 61), (len(data) + 1, 4096)):
                rc, out, pts = census_map(twin, data, S, window, piece, stride)
                assert rc == OK, (name, S, stride, window, piece)   # a condition, not a hope
                assert out[:3] == [len(rec_h), bases, len(data)], (name, S, stride, window, piece, out)
                assert pts == want, (name, S, stride, window, piece)
                n_runs += 1
                n_many += len(pts) > 3
    assert n_runs > 400 and n_many > 150                          # (not vacuous: many maps have several points)


@pytest.mark.parametrize("S", SEGMENTS)
def test_mapped_equals_selected(twin, host, S):
    """every well-formed case, stride and window: each selection through the map gives what the selecting twin gives on the whole
    text, which is the host's subset; zero unproven verdicts"""
    n_sel = n_points = n_merge = n_far = 0
    for name, data in B.well_formed():
        rec_h = host(data)[1]
        bases = sum(len(s) for _, s in rec_h)
        for stride in strides_for(data):
            for window, piece in ((64, 61), (3001, 3001), (len(data) + 1, 4096)):
                rc, out0 = census(twin, data, S, window, piece)
                assert rc == OK
                per_window = window_records(twin)
                rc, out, pts = census_map(twin, data, S, window, piece, stride)
                assert rc == OK and out == out0, (name, S, stride, window)                  # the map changes no count
                for kind, sel in seek_selections(len(rec_h), per_window, pts).items():
                    what = (name, S, stride, window, kind)
                    got = mapped(twin, data, S, window, piece, sel)
                    check_kept(got, rec_h, bases, sel, what)
                    if stride in (36, 4096) and window == 64:
                        assert got == selected(twin, data, S, window, piece, sel), what
                    n_sel += 1
                    n_points += kind == "around the points"
                    n_merge += kind == "neighbouring cells"
                    n_far += kind == "far apart"
    assert n_sel > 1500 and n_points > 100 and n_merge > 50 and n_far > 30


def test_planner_on_plain_text_and_bgzf_blocks(twin, host):
    """the plan's statistics on the plain text and on a BGZF table of 3 000-byte blocks with the empty end block: only the blocks a
    run touches, each once; records span blocks, and a run that ends exactly where a block starts leaves that block out"""
    import bgzf_writer as W
    rng = __import__("random").Random(57)
    # records of 264 bytes each behind a 36-byte header... sized so that a record start falls on a block start: found, not assumed
    recs = [B.record(b"r%03d" % i, B._seq(rng, 400 + (i % 7))) for i in range(80)]
    data = B.bam(recs)
    rec_h = host(data)[1]
    n = len(rec_h)
    hdr_end, starts = record_starts(data)
    # shift the records by padding the header text until some record starts at a multiple of 3000
    for pad in range(3000):
        hdr = B.header(b"@HD\tVN:1.6\tSO:unknown\n" + b"@CO\t" + b"x" * pad + b"\n")
        st = [len(hdr) + s - hdr_end for s in starts]
        if any(s % 3000 == 0 for s in st[2:-2]):
            break
    data = hdr + data[hdr_end:]
    hdr_end, starts = record_starts(data)
    rec_h = host(data)[1]
    assert len(rec_h) == n and any(s % 3000 == 0 for s in starts[2:-2])
    comp = W.bgzf_compress(data, block=3000)
    table = bgzf_table(comp)
    assert int(table[1].sum()) == len(data) and int(table[0].sum()) == len(comp) and table[1][-1] == 0     # the empty end block
    o = np.concatenate([[0], np.cumsum(table[1])])
    assert any(o[b] < s < o[b + 1] < s + 4 + struct.unpack_from("<i", data, s)[0] for s in starts for b in range(len(o) - 2))   # records span blocks
    rc, _, pts = census_map(twin, data, 64, 3001, 3001, 64)
    assert rc == OK and pts == reference_points(starts, 64) and len(pts) == n
    # the plain text: one ordinal is one run from its point to the next; file bytes are text bytes, no blocks
    rc, st, runs, rs = seek_plan(twin, [5])
    assert rc == OK and runs == [(5, 1, starts[5], starts[6])] and rs == [0] and st == (1, starts[6] - starts[5], starts[6] - starts[5], 0)
    rc, st, runs, rs = seek_plan(twin, [5, 6, 40, n - 1])
    assert runs == [(5, 2, starts[5], starts[7]), (40, 1, starts[40], starts[41]), (n - 1, 1, starts[n - 1], len(data))] and rs == [0, 1, 2, 3]
    assert st == (3, sum(r[3] - r[2] for r in runs), sum(r[3] - r[2] for r in runs), 0)
    # everything: one run from hdr_end to the end, every block but none twice
    rc, st, runs, _ = seek_plan(twin, list(range(n)), table, len(comp))
    assert rc == OK and st == (1, len(data) - hdr_end, len(comp), len(table[0]))

    def touched(runs):
        return sorted({b for r in runs for b in range(len(table[0])) if table[1][b] and o[b] < r[3] and o[b + 1] > r[2]})
    # a run that ends exactly at a block start: the block behind it is not read
    whole = next(i for i in range(2, n - 2) if starts[i] % 3000 == 0)
    rc, st, runs, _ = seek_plan(twin, [whole - 1], table, len(comp))
    assert runs == [(whole - 1, 1, starts[whole - 1], starts[whole])]
    t = touched(runs)
    assert t[-1] == starts[whole] // 3000 - 1 and st == (1, starts[whole] - starts[whole - 1], int(table[0][t].sum()), len(t))
    # a record that spans blocks brings both; two runs in one block count it once
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
        check_kept(mapped(twin, data, 64, 3001, 3001, sel), rec_h, bases, sel, sel)
    assert seek_plan(twin, [0], table, len(comp) + 1)[0] == INVALID             # a block table of another file


def plan_text_bytes(pts, sel, text_len):
    """the text bytes the runs of a selection bring, from the points alone: the cells' stretches that hold a chosen ordinal, once each"""
    ends = [o for _, o in pts[1:]] + [text_len]
    hit = {max(i for i, (o, _) in enumerate(pts) if o <= r) for r in sel}
    return sum(ends[i] - pts[i][1] for i in hit)


def small_big_small_in_one_cell():
    """small, 40 001 bases, small behind a header of 64 bytes: the first small record and the large one start in one cell of 64"""
    rng = __import__("random").Random(51)
    recs = [B.record(b"s", b"AC"), B.record(b"big", B._seq(rng, 40001, b"ACGTN")), B.record(b"t", b"GGA")]
    hdr = B.header(b"@HD\tVN:1.6\tSO:unknown\n@CO\t" + b"x" * 25 + b"\n")
    assert len(hdr) == 64 and len(recs[0]) < 64
    return B.bam(recs, hdr), recs


def test_a_record_of_many_cells_and_windows(twin, host):
    """small, 40 001 bases, small at window 64 and stride 64: no point inside the large record, and none at its start, which lies in
    the first record's cell: only [2] brings a small run.  With the default header the large record starts a cell of its own, and
    [0, 2] brings two small runs"""
    for (data, recs), want_pts in ((small_big_small_in_one_cell(), [0, 2]), (small_big_small(), [0, 1, 2])):
        rec_h = host(data)[1]
        hdr_end, starts = record_starts(data)
        rc, out, pts = census_map(twin, data, 64, 64, 61, 64)
        assert rc == OK and pts == reference_points(starts, 64) and [p[0] for p in pts] == want_pts
        assert pts[-1][1] // 64 - pts[-2][1] // 64 > 300            # (hundreds of cells without a point)
        for sel in ([1], [0, 2], [0, 1, 2], [2]):
            rc, st, runs, rs = seek_plan(twin, sel)
            assert rc == OK and st[1] == plan_text_bytes(pts, sel, len(data)), (sel, st)
            if sel == [2]:
                assert runs == [(2, 1, starts[2], len(data))] and st[1] < 64
            elif want_pts == [0, 2] or 1 in sel:
                assert st[1] > 20000
            check_kept(mapped(twin, data, 64, 64, 61, sel), rec_h, 40006, sel, sel)
            assert mapped_bam_stats(twin)["segments"] >= 1


def test_mapped_bam_stats_are_the_sub_texts(twin, host):
    """the counts of the record scan are summed over the windows of the sub-text: fewer segments than the whole text has"""
    data = dict(B.well_formed())["bait_quality"]
    n = len(host(data)[1])
    assert census_map(twin, data, 64, 257, 257, 257)[0] == OK
    assert selected(twin, data, 64, 257, 257, [n - 1])[0] == OK
    whole = mapped_bam_stats(twin)["segments"]
    assert mapped(twin, data, 64, 257, 257, [n - 1])[0] == OK
    assert 0 < mapped_bam_stats(twin)["segments"] < whole
    assert mapped(twin, data, 64, 257, 257, [])[:3] == (OK, [], b"") and mapped_bam_stats(twin)["segments"] == 0


def test_refusals(twin, host):
    """a map of another text, an ordinal equal to n, an unsorted list, a text of the same size with a damaged record"""
    cases = dict(B.well_formed())
    data, other = cases["bait_quality"], cases["names"]
    n = len(host(data)[1])
    assert census_map(twin, data, 64, 257, 257, 257)[0] == OK
    assert mapped(twin, other, 64, 257, 257, [0])[0] == INVALID
    for sel in ([n], [0, n - 1, n], [5, 3], [0, 4, 4, 9]):
        assert mapped(twin, data, 64, 257, 257, sel)[0] == INVALID, sel
        assert seek_plan(twin, sel)[0] == INVALID, sel
    assert mapped(twin, data, 64, 257, 257, [n - 1])[0] == OK
    # the same size, but the chosen run's record is mapped now: never other records
    hdr_end, starts = record_starts(data)
    bad = bytearray(data)
    struct.pack_into("<H", bad, starts[3] + 4 + 14, 0)             # flag: the unmapped bit cleared
    rc, rec, _, _ = mapped(twin, bytes(bad), 64, 257, 257, [3])
    assert rc == UNPROVEN
    out = (C.c_uint64 * 4)()
    assert twin.bam_twin_census_map(data, len(data), 64, 64, 1, 0, C.byref(out)) == -1     # a stride has bytes
    for name, text in B.unproven():
        assert census_map(twin, text, 64, 257, 61, 257)[0] == UNPROVEN, name


def test_abi_has_the_flag():
    from lrge_amd import _ffi
    assert re.search(r"#define\s+LRGE_GPU_INGEST_SELECT_ALN\s+1024\b", open(os.path.join(ROOT, "include", "lrge_hip.h")).read()) and _ffi.GPU_INGEST_SELECT_ALN == 1024
    assert re.search(r"LRGE_GPU_INGEST_SELECT_ALN: c_int = 1024;", open(os.path.join(ROOT, "integration", "liblrge_hip_shim.rs")).read())
    assert "LRGE_GPU_INGEST_SELECT_ALN" in open(os.path.join(ROOT, "include", "lrge_hip.hpp")).read()
    assert "LRGE_GPU_INGEST_SELECT_ALN" in open(os.path.join(ROOT, "tools", "lrge_hip_cli.cpp")).read()
    flags = [v for k, v in vars(_ffi).items() if k.startswith(("GPU_INGEST_", "GPU_INFLATE_")) and isinstance(v, int)]
    assert len(flags) == len(set(flags)) and all(v & (v - 1) == 0 for v in flags)         # one bit each, none shared


def test_k_bam_keep_resources(tmp_path):
    """no scratch, no LDS, no spill, from the compiler's own report; k_bam_store shares the copy body and stays so too"""
    import subprocess
    src = tmp_path / "k.hip"
    src.write_text('#include "%s"\n' % os.path.join(ROOT, "lrge_amd", "csrc", "k_bam.h"))
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-o", str(tmp_path / "k.o"), str(src),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    txt = r.stderr
    for k in ("k_bam_keep", "k_bam_store"):
        i = txt.index("Function Name: _Z%d%s" % (len(k), k))
        block = txt[i:i + 2000]
        val = lambda key: int(re.search(key + r": (\d+)", block).group(1))   # noqa: E731
        assert val(r"ScratchSize \[bytes/lane\]") == 0, k
        assert val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0, k
        assert val(r"LDS Size \[bytes/block\]") == 0, k
        assert val(r"Occupancy \[waves/SIMD\]") == 8, k             # (the launch counts on 8 wavefronts a SIMD)
