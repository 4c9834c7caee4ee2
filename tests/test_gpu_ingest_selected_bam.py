"""The sampled device ingest of unaligned BAM (LRGE_GPU_INGEST_SELECT_ALN beside LRGE_GPU_INGEST_BAM in lrge_hip_reads_census*,
_open_selected*, _census_map*, _open_mapped*; k_bam_keep, k_fx_seek with the BAM record start) against the host
reader, the host twin's map and plan, and the full windowed open of the same input: raw, in BGZF blocks of 3000 bytes and in a gzip
member of many deflate blocks, through windows of a few thousand bytes, at segments of 64 and 4096 bytes and strides below a
block, at a block and above the text.  The shapes are the smallest at which the kernels can go wrong: every residue of source and
destination in the packed copy, a chosen record first or last in a window or a run, odd and empty sequences side by side, a
record of hundreds of cells and windows."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import bam_corpus as B
import bgzf_writer as W
import sam_corpus as S
from test_bam_seek_twin import bind, census_map, mapped, mapped_bam_stats, plan_text_bytes, record_starts, seek_plan, small_big_small_in_one_cell
from test_bam_select_twin import census as twin_census, selected as twin_selected, selections, window_records
from test_fastx_seek_twin import bgzf_table, seek_selections
from test_gpu_ingest_seek import same_handle
from test_gpu_ingest_selected import set_knobs
from test_gpu_ingest_windowed import read_host, upload_still_works, wrap

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["big_60", "lengths", "names", "bait_quality", "long_record"]
WRAPS = ["raw", "bgzf", "gzip_blocks"]
WINDOWS = [3001, 20000]
SEGS = [64, 4096]
STRIDES = [512, 3000, 1 << 20]


def flags(extra=0, aln=True):
    from lrge_amd import _ffi
    return _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INGEST_BAM | (_ffi.GPU_INGEST_SELECT_ALN if aln else 0) | extra


def knobs_for(knobs, window, seg, stride=None):
    set_knobs(knobs, window)
    knobs.set("BAM_SEGMENT_BYTES", seg)
    if stride is not None:
        knobs.set("INGEST_SEEK_STRIDE_BYTES", stride)


@pytest.fixture(scope="module")
def twin():
    from lrge_amd import build as Bd
    return bind(C.CDLL(Bd.build_bam_twin()))


class Ref:
    """the host reader's records of one BAM text, the full windowed open of it on the device (computed once) and, by selection,
    the sketch of that open's read set"""

    def __init__(self, ctx, path, name, text):
        from lrge_amd import _ffi
        path.write_bytes(text)
        rc, rec, msg = read_host(path)
        assert rc == 0, (name, msg)
        self.ctx, self.name, self.text = ctx, name, text
        self.names, self.seqs = [n for n, _ in rec], [s for _, s in rec]
        self.lens = np.array([len(s) for s in self.seqs], dtype=np.uint32)
        self.spans = (self.lens.astype(np.int64) + 1) // 2
        self.n, self.bases = len(rec), int(self.lens.sum())
        self.full = ctx.open_reads(text, flags(_ffi.GPU_INGEST_WINDOWED | _ffi.GPU_INGEST_WINDOWED_ALN, aln=False))
        assert self.full.names == self.names and np.array_equal(self.full.lens, self.lens), name
        self._sk = {}

    def sketch(self, idx):
        key = tuple(idx)
        if key not in self._sk:
            self._sk[key] = None
            if int(self.lens[list(idx)].sum()):
                s = self.full.seqset(list(idx))
                self._sk[key] = s.sketch(0)
                s.free()
        return self._sk[key]

    def check(self, dr, sel, what, subset=True):
        k = len(sel)
        assert dr.n == k and dr.text_bytes == len(self.text), (self.name, what)
        assert dr.names == [self.names[i] for i in sel], (self.name, what)
        assert np.array_equal(dr.lens, self.lens[sel] if k else np.zeros(0, dtype=np.uint32)), (self.name, what)
        assert dr.select_stats() == (self.n, k, self.bases, int(self.lens[sel].sum()) if k else 0), (self.name, what, dr.select_stats())
        assert dr.window_stats()[1] == (int(self.spans[sel].sum()) if k else 0), (self.name, what)     # store bytes: packed
        sub = np.random.default_rng(11).permutation(k)[:max(1, k // 2)].tolist() if k and subset else []
        for kind, jdx in (("all", list(range(k))), ("shuffled subset", sub)):
            want = self.sketch([sel[j] for j in jdx]) if jdx else None
            if want is None:
                continue
            s = dr.seqset(jdx)
            assert s.n == len(jdx) and np.array_equal(s.lens, self.lens[[sel[j] for j in jdx]]), (self.name, what, kind)
            xd, yd = s.sketch(0)
            assert np.array_equal(xd, want[0]) and np.array_equal(yd, want[1]), (self.name, what, kind)
            s.free()


@pytest.fixture(scope="module")
def refs(ctx, tmp_path_factory):
    p = tmp_path_factory.mktemp("selected_bam_host") / "in.bam"
    cases = dict(B.well_formed())
    out = {name: Ref(ctx, p, name, cases[name]) for name in CASES}
    yield out
    for r in out.values():
        r.full.free()


def many_windows(text, how, window):
    """must a pass over `text` flush more than one window?  (a round of the gzip decoder brings about 40 KB of text at once)"""
    return len(text) > 2 * window and (how != "gzip_blocks" or len(text) > 65536)


def twin_points(twin, text, seg, window, stride):
    rc, out, pts = census_map(twin, text, seg, window, window, stride)
    assert rc == 0
    return out, pts


def twin_stats(twin, data, how, sel):
    """what seek_stats() must say, by the twin's plan on its last map; a container that cannot be entered brings no run"""
    if how == "gzip_blocks":
        return (0, 0, 0, 0)
    rc, st, runs, _ = seek_plan(twin, sel, bgzf_table(data) if how == "bgzf" else None, len(data))
    assert rc == 0
    return st


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("how", WRAPS)
def test_census_and_map_equal_host_and_twin(ctx, knobs, refs, twin, how, window, seg):
    """records, bases and text bytes are the host reader's and the twin's (raw input: the windows too); the windowed flags change
    nothing; a census with a map returns the same counts and the twin's points, each in the block that holds it"""
    from lrge_amd import _ffi
    for name in CASES:
        ref = refs[name]
        data = wrap(ref.text, how)
        knobs_for(knobs, window, seg, STRIDES[0])
        out = ctx.census_reads(data, flags())
        rc, tw = twin_census(twin, ref.text, seg, window, window)
        assert rc == 0 and out[:3] == (ref.n, ref.bases, len(ref.text)) == tuple(tw[:3]), (name, how, window, seg, out, tw)
        assert how != "raw" or out[3] == max(1, tw[3]), (name, window, seg, out, tw)      # (a text within one window is the last window)
        assert out[3] >= 1 and (out[3] > 1 or not many_windows(ref.text, how, window)), (name, how, window, out)
        assert ctx.census_reads(data, flags(_ffi.GPU_INGEST_WINDOWED | _ffi.GPU_INGEST_WINDOWED_ALN)) == out, (name, how, window)
        for stride in STRIDES:
            knobs_for(knobs, window, seg, stride)
            counts, m = ctx.census_map_reads(data, flags())
            what = (name, how, window, seg, stride)
            assert counts == out, what
            _, want = twin_points(twin, ref.text, seg, window, stride)
            pts = m.points()
            assert [(o, t) for o, t, _ in pts] == want and want[0] == (0, record_starts(ref.text)[0]), what
            assert m.stats() == (ref.n, len(want), stride, len(ref.text)), what
            if how == "bgzf":
                c_len, isize = bgzf_table(data)
                c_at, o_at = np.concatenate([[0], np.cumsum(c_len)]), np.concatenate([[0], np.cumsum(isize)])
                for _, t, c in pts:
                    b = int(np.searchsorted(o_at, t, side="right")) - 1
                    assert c == c_at[b] and o_at[b] <= t < o_at[b + 1], (what, t, c)
            else:
                assert all(c == 0 for _, _, c in pts), what
            m.free()


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("how", WRAPS)
def test_selected_and_mapped_equal_the_full_open(ctx, knobs, refs, twin, how, window, seg):
    """every selection of every case: names, lengths, counts and the sketch of the full open on the same indices; the mapped open
    gives the handle of the selected open and the statistics of the twin's plan; raw input: the scan counts are the twin's sums"""
    for name in CASES:
        ref = refs[name]
        data = wrap(ref.text, how)
        knobs_for(knobs, window, seg, STRIDES[0])
        rc, _ = twin_census(twin, ref.text, seg, window, window)
        assert rc == 0
        sels = selections(ref.n, window_records(twin))
        kept = {}
        for kind, sel in sels.items():
            dr = ctx.open_reads_selected(data, sel, flags())
            ref.check(dr, sel, (how, window, seg, kind))
            assert dr.seek_stats() == (0, 0, 0, 0)
            if how == "raw":
                assert twin_selected(twin, ref.text, seg, window, window, sel)[0] == 0
                assert dr.bam_stats == mapped_bam_stats(twin), (name, window, seg, kind)
            if kind == "all" and many_windows(ref.text, how, window):
                st = dr.window_stats()
                assert st[0] > 1 and st[2] >= window and st[3] > 0, (name, how, window, st)
            kept[kind] = dr
        for stride in STRIDES:
            knobs_for(knobs, window, seg, stride)
            _, m = ctx.census_map_reads(data, flags())
            _, pts = twin_points(twin, ref.text, seg, window, stride)
            more = {k: v for k, v in seek_selections(ref.n, [ref.n], pts).items() if k in ("around the points", "neighbouring cells", "far apart")}
            some = dict(sels) if stride == STRIDES[0] else {k: sels[k] for k in ("empty", "every third", "last")}
            for kind, sel in {**some, **more}.items():
                what = (name, how, window, seg, stride, kind)
                dr = ctx.open_reads_mapped(data, m, sel, flags())
                ref.check(dr, sel, what, subset=False)
                other = kept[kind] if kind in kept else ctx.open_reads_selected(data, sel, flags())
                same_handle(dr, other, what)
                assert dr.seek_stats() == twin_stats(twin, data, how, sel), (what, dr.seek_stats())
                if how == "raw":
                    assert mapped(twin, ref.text, seg, window, window, sel)[0] == 0
                    assert dr.bam_stats == mapped_bam_stats(twin), what
                if kind not in kept:
                    other.free()
                dr.free()
            m.free()
        for dr in kept.values():
            dr.free()


def sweep_records():
    """about 300 records: packed lengths walk the edges of the 16-byte groups and of a wavefront's 1 KiB step, odd and even base
    counts alternate, identifier lengths walk 1..16"""
    packed = [0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 1040, 2049]
    rng = random.Random(61)
    recs = []
    for i in range(299):
        p = packed[i % len(packed)]
        l_seq = 0 if not p else 2 * p - (i // len(packed)) % 2
        name = (b"%03dabcdefghijklm" % i)[:1 + i % 16]
        recs.append((name, B._seq(rng, l_seq, b"ACGTN")))
    return recs


def test_copy_sweep(ctx, knobs, twin, tmp_path):
    """every second record of the sweep at stride 1, so every run is one record: the source of k_bam_keep takes all four residues mod
    4 (both branches of the copy), its destination all sixteen mod 16; one window, several windows and the mapped sub-text"""
    recs = sweep_records()
    text = B.bam([B.record(n, s) for n, s in recs])
    ref = Ref(ctx, tmp_path / "sweep.bam", "sweep", text)
    sel = list(range(0, ref.n, 2))
    hdr_end, starts = record_starts(text)
    spans = ref.spans[sel]
    dst = np.concatenate([[0], np.cumsum(spans)])[:-1]
    big = spans >= 48                                               # (records that reach the 16-byte groups)
    assert {int(d) % 16 for d in dst[big]} == set(range(16))
    src_whole = np.array([starts[i] + 36 + len(recs[i][0]) + 1 for i in sel])         # in the block of one window: text offsets
    sub_at = np.concatenate([[0], np.cumsum([starts[i + 1] - starts[i] if i + 1 < ref.n else len(text) - starts[i] for i in sel])])[:-1]
    src_sub = sub_at + 36 + np.array([len(recs[i][0]) + 1 for i in sel])              # in the sub-text of a mapped open
    for src in (src_whole, src_sub):
        # the 16-byte groups start `head` bytes in: (src + head) mod 4 decides the branch
        head = (16 - dst % 16) % 16
        assert {int(x) % 4 for x in (src + head)[big]} == set(range(4)) and {int(x) % 4 for x in src[big]} == set(range(4))
    try:
        for window in (1 << 20, 20000):
            for how in ("raw", "bgzf"):
                knobs_for(knobs, window, 4096, 1)
                data = wrap(text, how)
                counts, m = ctx.census_map_reads(data, flags())
                assert counts[:3] == (ref.n, ref.bases, len(text)) and m.stats()[1] == ref.n, (how, window)
                a = ctx.open_reads_selected(data, sel, flags())
                ref.check(a, sel, (how, window, "selected"))
                b = ctx.open_reads_mapped(data, m, sel, flags())
                ref.check(b, sel, (how, window, "mapped"), subset=False)
                same_handle(a, b, (how, window))
                twin_points(twin, text, 4096, window, 1)
                st = b.seek_stats()
                assert st == twin_stats(twin, data, how, sel) and st[0] == len(sel) and st[1] < len(text), (how, window, st)
                a.free(); b.free(); m.free()
    finally:
        ref.full.free()


def test_a_record_of_many_cells_and_windows(ctx, knobs, twin, tmp_path):
    """small, 40 001 bases, small at window 64 and stride 64: chosen and not chosen; only [2] brings a small run"""
    text, _ = small_big_small_in_one_cell()
    ref = Ref(ctx, tmp_path / "sbs.bam", "small_big_small", text)
    try:
        for how in ("raw", "bgzf"):
            knobs_for(knobs, 64, 64, 64)
            data = wrap(text, how)
            counts, m = ctx.census_map_reads(data, flags())
            assert counts[:3] == (3, 40006, len(text)) and counts[3] >= 2 and [o for o, _, _ in m.points()] == [0, 2], (how, counts, m.points())
            _, pts = twin_points(twin, text, 64, 64, 64)
            for sel in ([1], [0, 2], [0, 1, 2], [2]):
                dr = ctx.open_reads_mapped(data, m, sel, flags())
                ref.check(dr, sel, (how, sel))
                st = dr.seek_stats()
                assert st == twin_stats(twin, data, how, sel) and st[1] == plan_text_bytes(pts, sel, len(text)), (how, sel, st)
                assert (st[1] < 200) == (sel == [2]), (how, sel, st)         # only the last record's run is small
                other = ctx.open_reads_selected(data, sel, flags())
                same_handle(dr, other, (how, sel))
                ws = other.window_stats()
                assert ws[0] >= 2 and ws[2] > 20000, (how, sel, ws)
                dr.free(); other.free()
            m.free()
    finally:
        ref.full.free()


def test_from_a_path(ctx, knobs, refs, twin, tmp_path):
    """the path form reads only the ranges of the plan: a sparse selection reads fewer file bytes and decodes fewer blocks than the
    file has, and gives the handle of the _mem form"""
    ref = refs["big_60"]
    knobs_for(knobs, 3001, 4096, 512)
    _, pts = twin_points(twin, ref.text, 4096, 3001, 512)
    sparse = [pts[len(pts) // 3][0], pts[-2][0]]
    for how in ("bgzf", "raw"):
        data = wrap(ref.text, how)
        p = tmp_path / ("in_%s.bam" % how)
        p.write_bytes(data)
        assert ctx.census_reads(p, flags())[:3] == (ref.n, ref.bases, len(ref.text)), how
        counts, m = ctx.census_map_reads(p, flags())
        assert counts[:3] == (ref.n, ref.bases, len(ref.text)) and [(o, t) for o, t, _ in m.points()] == pts, how
        n_blocks = len(bgzf_table(data)[0]) if how == "bgzf" else 0
        for kind, sel in (("sparse", sparse), ("every third", list(range(0, ref.n, 3))), ("all", list(range(ref.n))), ("empty", [])):
            dr = ctx.open_reads_mapped(p, m, sel, flags())
            ref.check(dr, sel, (how, kind), subset=False)
            st = dr.seek_stats()
            assert st == twin_stats(twin, data, how, sel), (how, kind, st)
            mem = ctx.open_reads_mapped(data, m, sel, flags())
            same_handle(dr, mem, (how, kind))
            assert mem.seek_stats() == st, (how, kind)
            sel_p = ctx.open_reads_selected(p, sel, flags())
            same_handle(dr, sel_p, (how, kind, "selected from the path"))
            if kind == "sparse":
                assert st[0] == 2 and 0 < st[1] < len(ref.text) // 4 and 0 < st[2] < len(data) // 4 and (how == "raw" or 0 < st[3] < n_blocks // 4), (how, st)
            dr.free(); mem.free(); sel_p.free()
        m.free()


def test_budget(ctx, knobs, refs):
    """INGEST_MAX_BYTES bounds the chosen packed bytes plus the block: one byte below all packed bytes, every second read fits and
    all do not, in both opens"""
    from lrge_amd import _ffi
    ref = refs["big_60"]
    knobs_for(knobs, 3001, 4096, 512)
    knobs.set("INGEST_MAX_BYTES", int(ref.spans.sum()) - 1)
    for how in ("raw", "bgzf"):
        data = wrap(ref.text, how)
        counts, m = ctx.census_map_reads(data, flags())
        assert counts[:2] == (ref.n, ref.bases), how
        sel = list(range(0, ref.n, 2))
        for dr in (ctx.open_reads_selected(data, sel, flags()), ctx.open_reads_mapped(data, m, sel, flags())):
            ref.check(dr, sel, (how, "every second, below the cap"), subset=False)
            dr.free()
        for call in (lambda: ctx.open_reads_selected(data, list(range(ref.n)), flags()), lambda: ctx.open_reads_mapped(data, m, list(range(ref.n)), flags())):
            with pytest.raises(_ffi.UnprovenInput) as ei:
                call()
            assert "bases and window above INGEST_MAX_BYTES" in str(ei.value), how
            upload_still_works(ctx)
        m.free()


def test_header_that_ends_the_text(ctx, knobs):
    """an empty census, an empty map and empty handles"""
    knobs_for(knobs, 3001, 64, 512)
    for hdr in (B.header(), B.header(refs=[(b"chr1", 1000)])):
        for how in ("raw", "bgzf"):
            data = wrap(hdr, how)
            assert ctx.census_reads(data, flags())[:3] == (0, 0, len(hdr))
            counts, m = ctx.census_map_reads(data, flags())
            assert counts[:3] == (0, 0, len(hdr)) and m.stats()[:2] == (0, 0)
            for dr in (ctx.open_reads_selected(data, [], flags()), ctx.open_reads_mapped(data, m, [], flags())):
                assert dr.n == 0 and dr.names == [] and dr.select_stats() == (0, 0, 0, 0) and dr.bam_stats["segments"] == 0
                dr.free()
            m.free()


def test_refusals(ctx, knobs, refs):
    """the new flag without LRGE_GPU_INGEST_BAM; SAM with it; a mapped record in the third window, a damaged record and 1-3 trailing
    bytes: unproven, no handle; bad selections; a map of another input; a BAM map used without the flags"""
    from lrge_amd import _ffi
    ref = refs["big_60"]
    only = "selected ingest takes FASTA / FASTQ only"
    inflate = _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP
    sam = S.toy_sam([n.split()[0] for n in ref.names[:12]], ref.seqs[:12])
    knobs_for(knobs, 3001, 64, 512)
    for how in WRAPS:
        for data, fl in ((wrap(ref.text, how), inflate | _ffi.GPU_INGEST_SELECT_ALN), (wrap(ref.text, how), flags(aln=False)),
                         (wrap(sam, how), flags(_ffi.GPU_INGEST_SAM)), (wrap(sam, how), flags(_ffi.GPU_INGEST_SAM | _ffi.GPU_INGEST_WINDOWED | _ffi.GPU_INGEST_WINDOWED_ALN))):
            for call in (lambda d, f: ctx.census_reads(d, f), lambda d, f: ctx.census_map_reads(d, f), lambda d, f: ctx.open_reads_selected(d, [0, 1], f)):
                with pytest.raises(_ffi.UnprovenInput) as ei:
                    call(data, fl)
                assert ei.value.code == _ffi.ERR_UNPROVEN and only in str(ei.value), (how, fl)
    upload_still_works(ctx)
    # a mapped record in the third window after two clean ones, a record with a bad block size, 1-3 trailing bytes
    rng = random.Random(53)
    recs = [B.record(b"m%d" % i, B._seq(rng, 30)) for i in range(12)]
    k = next(i for i in range(12) if len(B.header()) + sum(len(r) for r in recs[:i]) > 2 * 200)
    bad = [B.bam(recs[:k] + [B.record(b"mapped", B._seq(rng, 30), flag=0)] + recs[k:]), B.bam(recs[:k]) + (31).to_bytes(4, "little") + bytes(31) + b"".join(recs[k:])]
    bad += [B.bam(recs) + bytes(t) for t in (1, 2, 3)]
    knobs_for(knobs, 200, 64, 64)
    good = B.bam(recs)
    assert ctx.census_reads(good, flags())[3] >= 3
    _, m_good = ctx.census_map_reads(good, flags())
    for text in bad:
        for how in ("raw", "bgzf"):
            data = wrap(text, how)
            for call in (lambda: ctx.census_reads(data, flags()), lambda: ctx.census_map_reads(data, flags()), lambda: ctx.open_reads_selected(data, [0, 1], flags()),
                         lambda: ctx.open_reads_selected(data, [], flags())):
                with pytest.raises(_ffi.UnprovenInput) as ei:
                    call()
                assert ei.value.code == _ffi.ERR_UNPROVEN and "not proven on the device" in str(ei.value), (how, str(ei.value))
            upload_still_works(ctx)
    # a text of the map's size whose chosen run holds a mapped record now: the map does not fit, never other records
    hdr_end, starts = record_starts(good)
    dented = bytearray(good)
    dented[starts[k] + 4 + 14:starts[k] + 4 + 16] = b"\0\0"
    with pytest.raises(_ffi.UnprovenInput) as ei:
        ctx.open_reads_mapped(bytes(dented), m_good, [k], flags())
    assert "the map does not fit the input" in str(ei.value)
    upload_still_works(ctx)
    m_good.free()
    # bad selections keep their wording; a map of another input; a BAM map without the flags
    knobs_for(knobs, 3001, 64, 512)
    other = refs["bait_quality"]
    for how in ("raw", "bgzf"):
        data = wrap(ref.text, how)
        _, m = ctx.census_map_reads(data, flags())
        for sel in ([5, 3], [0, 4, 4, 9]):
            for call in (lambda: ctx.open_reads_selected(data, sel, flags()), lambda: ctx.open_reads_mapped(data, m, sel, flags())):
                with pytest.raises(_ffi.LrgeHipError) as ei:
                    call()
                assert ei.value.code == _ffi.ERR_INVALID and "strictly ascending" in str(ei.value), (how, sel)
        for sel in ([ref.n], [0, ref.n - 1, ref.n + 7]):
            for call in (lambda: ctx.open_reads_selected(data, sel, flags()), lambda: ctx.open_reads_mapped(data, m, sel, flags())):
                with pytest.raises(_ffi.LrgeHipError) as ei:
                    call()
                assert ei.value.code == _ffi.ERR_INVALID and "ordinal %d of %d records" % (sel[-1], ref.n) in str(ei.value), (how, sel)
        for wrong in (wrap(other.text, how), wrap(ref.text, "bgzf" if how == "raw" else "raw"), data[:-1], b""):
            with pytest.raises(_ffi.LrgeHipError) as ei:
                ctx.open_reads_mapped(wrong, m, [0], flags())
            assert ei.value.code == _ffi.ERR_INVALID and "the map is of another input" in str(ei.value), how
        for fl in (flags(aln=False), inflate | _ffi.GPU_INGEST_SELECT_ALN, inflate):
            with pytest.raises(_ffi.UnprovenInput) as ei:
                ctx.open_reads_mapped(data, m, [0], fl)
            assert ei.value.code == _ffi.ERR_UNPROVEN and only in str(ei.value), (how, fl)
        upload_still_works(ctx)
        dr = ctx.open_reads_mapped(data, m, [ref.n - 1], flags())
        assert dr.names == [ref.names[-1]]
        dr.free(); m.free()


@pytest.mark.parametrize("args", [["-T", "300", "-Q", "100"], ["-n", "200"]])
def test_cli_sampled_ubam_equals_device_ingest(tmp_path, args):
    """the golden toy reads as a BGZF uBAM: lrge-hip --gpu-ingest, with --gpu-sample and with --gpu-seek too print the same estimate,
    and each says which route ran"""
    from lrge_amd import build as Bd, readio
    names, seqs = readio.load(os.path.join(HERE, "golden", "toy_reads.fa.gz"))
    src = tmp_path / "toy.bam"
    src.write_bytes(W.bgzf_compress(W.bam_bytes(names, seqs)))
    cmd = [Bd.CLI_PATH, str(src)] + args + ["-s", "6", "-f"]
    runs = [subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300) for extra in (["--gpu-ingest"], ["--gpu-ingest", "--gpu-sample"], ["--gpu-ingest", "--gpu-sample", "--gpu-seek"])]
    assert all(r.returncode == 0 for r in runs), [r.stderr for r in runs]
    assert runs[0].stdout == runs[1].stdout == runs[2].stdout and runs[0].stdout.strip(), [r.stdout for r in runs]
    assert "gpu-ingest: device\n" in runs[0].stderr and "gpu-ingest: device (sampled)\n" in runs[1].stderr and "gpu-ingest: device (sampled, seek)\n" in runs[2].stderr, [r.stderr for r in runs]
    warn = lambda s: [ln for ln in s.splitlines() if ln.startswith("[WARN]")]   # noqa: E731
    assert warn(runs[0].stderr) == warn(runs[1].stderr) == warn(runs[2].stderr)
