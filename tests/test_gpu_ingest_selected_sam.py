"""The sampled device ingest of unaligned SAM (LRGE_GPU_INGEST_SELECT_SAM beside LRGE_GPU_INGEST_SAM in lrge_hip_reads_census*,
_open_selected*, _census_map*, _open_mapped*; the SAM windows in the keep modes, k_fx_bases behind k_sam_records, k_fx_keep, k_fx_seek
with the SAM record start) against the host reader, the host twin's map and plan, and the full windowed open of
the same input: raw, in BGZF blocks of 3000 bytes and in a gzip member of many deflate blocks, through windows of a few thousand
bytes, at strides below a block, at a block and above the text.  The shapes are the smallest at which the path can go wrong:
sequence lengths on every side of a 16-byte group and of a 1 KiB step, '*' and empty fields, CRLF, a chosen record first or last
in a window or a run, a record of hundreds of cells and windows."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import bgzf_writer as W
import sam_corpus as S
from test_bam_select_twin import selections
from test_fastx_seek_twin import bgzf_table, seek_selections
from test_gpu_bam import toy_reads
from test_gpu_ingest_seek import same_handle
from test_gpu_ingest_selected import set_knobs
from test_gpu_ingest_windowed import read_host, upload_still_works, wrap
from test_sam_seek_twin import bind, census_map, mapped, plan_text_bytes, record_starts, seek_plan
from test_sam_select_twin import census as twin_census, small_big_small, window_records

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["plain_40", "lengths", "names", "crlf", "long_200k"]
WRAPS = ["raw", "bgzf", "gzip_blocks"]
WINDOWS = [3001, 20000]
STRIDES = [512, 3000, 1 << 20]


def flags(extra=0, sel=True, sam=True):
    from lrge_amd import _ffi
    return _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | (_ffi.GPU_INGEST_SAM if sam else 0) | (_ffi.GPU_INGEST_SELECT_SAM if sel else 0) | extra


def knobs_for(knobs, window, stride=None):
    set_knobs(knobs, window)
    if stride is not None:
        knobs.set("INGEST_SEEK_STRIDE_BYTES", stride)


@pytest.fixture(scope="module")
def twin():
    from lrge_amd import build as Bd
    return bind(C.CDLL(Bd.build_sam_twin()))


class Ref:
    """the host reader's records of one SAM text, the full windowed open of it on the device (computed once) and, by selection,
    the sketch of that open's read set"""

    def __init__(self, ctx, path, name, text):
        from lrge_amd import _ffi
        path.write_bytes(text)
        rc, rec, msg = read_host(path)
        assert rc == 0, (name, msg)
        self.ctx, self.name, self.text = ctx, name, text
        self.names, self.seqs = [n for n, _ in rec], [s for _, s in rec]
        self.lens = np.array([len(s) for s in self.seqs], dtype=np.uint32)
        self.n, self.bases = len(rec), int(self.lens.sum())
        self.full = ctx.open_reads(text, flags(_ffi.GPU_INGEST_WINDOWED | _ffi.GPU_INGEST_WINDOWED_ALN, sel=False))
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
        kept = int(self.lens[sel].sum()) if k else 0
        assert dr.n == k and dr.text_bytes == len(self.text), (self.name, what)
        assert dr.names == [self.names[i] for i in sel], (self.name, what)
        assert np.array_equal(dr.lens, self.lens[sel] if k else np.zeros(0, dtype=np.uint32)), (self.name, what)
        assert dr.select_stats() == (self.n, k, self.bases, kept), (self.name, what, dr.select_stats())
        assert dr.window_stats()[1] == kept, (self.name, what)     # store bytes: the chosen bases and nothing else
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
    p = tmp_path_factory.mktemp("selected_sam_host") / "in.sam"
    cases = dict(S.well_formed())
    out = {name: Ref(ctx, p, name, cases[name]) for name in CASES}
    yield out
    for r in out.values():
        r.full.free()


def many_windows(text, how, window):
    """must a pass over `text` flush more than one window?  (a round of the gzip decoder brings about 40 KB of text at once)"""
    return len(text) > 2 * window and (how != "gzip_blocks" or len(text) > 65536)


def twin_points(twin, text, window, stride):
    rc, out, pts = census_map(twin, text, window, window, stride)
    assert rc == 0
    return out, pts


def twin_stats(twin, data, how, sel):
    """what seek_stats() must say, by the twin's plan on its last map; a container that cannot be entered brings no run"""
    if how == "gzip_blocks":
        return (0, 0, 0, 0)
    rc, st, runs, _ = seek_plan(twin, sel, bgzf_table(data) if how == "bgzf" else None, len(data))
    assert rc == 0
    return st


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("how", WRAPS)
def test_census_and_map_equal_host_and_twin(ctx, knobs, refs, twin, how, window):
    """records, bases and text bytes are the host reader's and the twin's (raw input: the windows too); the windowed flags change
    nothing; a census with a map returns the same counts and the twin's points, each in the block that holds it"""
    from lrge_amd import _ffi
    for name in CASES:
        ref = refs[name]
        data = wrap(ref.text, how)
        knobs_for(knobs, window, STRIDES[0])
        out = ctx.census_reads(data, flags())
        rc, tw = twin_census(twin, ref.text, window, window)
        assert rc == 0 and out[:3] == (ref.n, ref.bases, len(ref.text)) == tuple(tw[:3]), (name, how, window, out, tw)
        assert how != "raw" or out[3] == max(1, tw[3]), (name, window, out, tw)      # (a text within one window is the last window)
        assert out[3] >= 1 and (out[3] > 1 or not many_windows(ref.text, how, window)), (name, how, window, out)
        assert ctx.census_reads(data, flags(_ffi.GPU_INGEST_WINDOWED | _ffi.GPU_INGEST_WINDOWED_ALN)) == out, (name, how, window)
        for stride in STRIDES:
            knobs_for(knobs, window, stride)
            counts, m = ctx.census_map_reads(data, flags())
            what = (name, how, window, stride)
            assert counts == out, what
            _, want = twin_points(twin, ref.text, window, stride)
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


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("how", WRAPS)
def test_selected_and_mapped_equal_the_full_open(ctx, knobs, refs, twin, how, window):
    """every selection of every case: names, lengths, counts, store bytes and the sketch of the full open on the same indices; the
    mapped open gives the handle of the selected open and the statistics of the twin's plan"""
    for name in CASES:
        ref = refs[name]
        data = wrap(ref.text, how)
        knobs_for(knobs, window, STRIDES[0])
        rc, _ = twin_census(twin, ref.text, window, window)
        assert rc == 0
        sels = selections(ref.n, window_records(twin))
        kept = {}
        for kind, sel in sels.items():
            dr = ctx.open_reads_selected(data, sel, flags())
            ref.check(dr, sel, (how, window, kind))
            assert dr.seek_stats() == (0, 0, 0, 0)
            if kind == "all" and many_windows(ref.text, how, window):
                st = dr.window_stats()
                assert st[0] > 1 and st[2] >= window and st[3] > 0, (name, how, window, st)
            kept[kind] = dr
        for stride in STRIDES:
            knobs_for(knobs, window, stride)
            _, m = ctx.census_map_reads(data, flags())
            _, pts = twin_points(twin, ref.text, window, stride)
            more = {k: v for k, v in seek_selections(ref.n, [ref.n], pts).items() if k in ("around the points", "neighbouring cells", "far apart")}
            some = dict(sels) if stride == STRIDES[0] else {k: sels[k] for k in ("empty", "every third", "last")}
            for kind, sel in {**some, **more}.items():
                what = (name, how, window, stride, kind)
                dr = ctx.open_reads_mapped(data, m, sel, flags())
                ref.check(dr, sel, what, subset=False)
                other = kept[kind] if kind in kept else ctx.open_reads_selected(data, sel, flags())
                same_handle(dr, other, what)
                assert dr.seek_stats() == twin_stats(twin, data, how, sel), (what, dr.seek_stats())
                if how == "raw":
                    assert mapped(twin, ref.text, window, window, sel)[0] == 0
                if kind not in kept:
                    other.free()
                dr.free()
            m.free()
        for dr in kept.values():
            dr.free()


def test_co_and_empty_lines_and_no_final_line_feed(ctx, knobs, twin, tmp_path):
    """a stride of 16: cells start inside @CO and empty lines, whose bytes travel at the end of the run in front; a text without a
    final line feed ends its last run without one"""
    cases = dict(S.well_formed())
    for name in ("co_and_empty_lines", "no_final_lf", "no_final_lf_empty_quality", "final_cr_after_crlf", "star_star_sequence"):
        text = cases[name]
        ref = Ref(ctx, tmp_path / (name + ".sam"), name, text)
        try:
            for how in ("raw", "bgzf"):
                for window, stride in ((64, 16), (3001, 64)):
                    knobs_for(knobs, window, stride)
                    data = wrap(text, how)
                    counts, m = ctx.census_map_reads(data, flags())
                    _, pts = twin_points(twin, text, window, stride)
                    assert counts[:3] == (ref.n, ref.bases, len(text)) and [(o, t) for o, t, _ in m.points()] == pts, (name, how, window)
                    for sel in ([], [0], [ref.n - 1], [0, ref.n - 1], list(range(ref.n)), list(range(1, ref.n, 2))):
                        a = ctx.open_reads_selected(data, sel, flags())
                        ref.check(a, sel, (how, window, sel), subset=False)
                        b = ctx.open_reads_mapped(data, m, sel, flags())
                        ref.check(b, sel, (how, window, sel, "mapped"), subset=False)
                        same_handle(a, b, (name, how, window, sel))
                        assert b.seek_stats() == twin_stats(twin, data, how, sel), (name, how, window, sel)
                        a.free(); b.free()
                    m.free()
        finally:
            ref.full.free()


def test_a_record_of_many_cells_and_windows(ctx, knobs, twin, tmp_path):
    """small, 200 000 bases, small at window 64 and stride 64: chosen and not chosen; only [2] brings a small run"""
    text = small_big_small()
    ref = Ref(ctx, tmp_path / "sbs.sam", "small_big_small", text)
    try:
        for how in ("raw", "bgzf"):
            knobs_for(knobs, 64, 64)
            data = wrap(text, how)
            counts, m = ctx.census_map_reads(data, flags())
            assert counts[:3] == (3, 200005, len(text)) and counts[3] >= 2 and [o for o, _, _ in m.points()] == [0, 2], (how, counts, m.points())
            _, pts = twin_points(twin, text, 64, 64)
            for sel in ([1], [0, 2], [2]):
                dr = ctx.open_reads_mapped(data, m, sel, flags())
                ref.check(dr, sel, (how, sel))
                st = dr.seek_stats()
                assert st == twin_stats(twin, data, how, sel) and st[1] == plan_text_bytes(pts, sel, len(text)), (how, sel, st)
                assert (st[1] < 200) == (sel == [2]), (how, sel, st)         # only the last record's run is small
                other = ctx.open_reads_selected(data, sel, flags())
                same_handle(dr, other, (how, sel))
                ws = other.window_stats()
                assert ws[0] >= 2 and ws[2] > 200000, (how, sel, ws)
                dr.free(); other.free()
            m.free()
    finally:
        ref.full.free()


def test_from_a_path(ctx, knobs, refs, twin, tmp_path):
    """the path form reads only the ranges of the plan: a sparse selection reads fewer file bytes and decodes fewer blocks than the
    file has, and gives the handle of the _mem form"""
    ref = refs["lengths"]
    knobs_for(knobs, 3001, 512)
    _, pts = twin_points(twin, ref.text, 3001, 512)
    sparse = [pts[len(pts) // 3][0], pts[-2][0]]
    for how in ("bgzf", "raw"):
        data = wrap(ref.text, how)
        p = tmp_path / ("in_%s.sam" % how)
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
                # (two runs of one record line each, a line of at most 2.1 KB: at most two blocks of 3000 text bytes a run)
                assert st[0] == 2 and 0 < st[1] < len(ref.text) // 4 and 0 < st[2] < len(data) // 2 and (how == "raw" or 0 < st[3] <= 4 < n_blocks // 4), (how, st)
            dr.free(); mem.free(); sel_p.free()
        m.free()


def test_budget(ctx, knobs, refs):
    """INGEST_MAX_BYTES bounds the chosen bases plus the block: one byte below all bases, every second read fits and all do not,
    in both opens -- the full windowed open of this text is refused at that cap"""
    from lrge_amd import _ffi
    ref = refs["lengths"]
    knobs_for(knobs, 3001, 512)
    knobs.set("INGEST_MAX_BYTES", ref.bases - 1)
    for how in ("raw", "bgzf"):
        data = wrap(ref.text, how)
        counts, m = ctx.census_map_reads(data, flags())
        assert counts[:2] == (ref.n, ref.bases), how
        sel = list(range(0, ref.n, 2))
        for dr in (ctx.open_reads_selected(data, sel, flags()), ctx.open_reads_mapped(data, m, sel, flags())):
            ref.check(dr, sel, (how, "every second, below the cap"), subset=False)
            dr.free()
        for call in (lambda: ctx.open_reads_selected(data, list(range(ref.n)), flags()), lambda: ctx.open_reads_mapped(data, m, list(range(ref.n)), flags()),
                     lambda: ctx.open_reads(data, flags(_ffi.GPU_INGEST_WINDOWED | _ffi.GPU_INGEST_WINDOWED_ALN))):
            with pytest.raises(_ffi.UnprovenInput) as ei:
                call()
            assert "bases and window above INGEST_MAX_BYTES" in str(ei.value), how
            upload_still_works(ctx)
        m.free()


def test_header_that_ends_the_text(ctx, knobs):
    """an empty census, an empty map and empty handles"""
    knobs_for(knobs, 3001, 512)
    cases = dict(S.well_formed())
    for hdr in (cases["header_only"], cases["header_no_lf"], cases["header_three_lines"]):
        for how in ("raw", "bgzf"):
            data = wrap(hdr, how)
            assert ctx.census_reads(data, flags())[:3] == (0, 0, len(hdr))
            counts, m = ctx.census_map_reads(data, flags())
            assert counts[:3] == (0, 0, len(hdr)) and m.stats()[:2] == (0, 0)
            for dr in (ctx.open_reads_selected(data, [], flags()), ctx.open_reads_mapped(data, m, [], flags())):
                assert dr.n == 0 and dr.names == [] and dr.select_stats() == (0, 0, 0, 0)
                dr.free()
            m.free()


def test_refusals(ctx, knobs, refs):
    """the new flag without LRGE_GPU_INGEST_SAM, and LRGE_GPU_INGEST_SAM without it; a mapped record in the third window, a line
    with fewer than ten tabs and a bad flag: unproven, no handle; the unproven corpus; bad selections; a map of another input; a SAM
    map used without the flags"""
    from lrge_amd import _ffi
    ref = refs["plain_40"]
    only = "selected ingest takes FASTA / FASTQ only"
    knobs_for(knobs, 3001, 512)
    for how in WRAPS:
        data = wrap(ref.text, how)
        for fl in (flags(sam=False), flags(sel=False), flags(_ffi.GPU_INGEST_WINDOWED | _ffi.GPU_INGEST_WINDOWED_ALN, sel=False),
                   flags(_ffi.GPU_INGEST_BAM | _ffi.GPU_INGEST_SELECT_ALN, sel=False)):
            for call in (lambda d, f: ctx.census_reads(d, f), lambda d, f: ctx.census_map_reads(d, f), lambda d, f: ctx.open_reads_selected(d, [0, 1], f)):
                with pytest.raises(_ffi.UnprovenInput) as ei:
                    call(data, fl)
                assert ei.value.code == _ffi.ERR_UNPROVEN and only in str(ei.value), (how, fl)
    upload_still_works(ctx)
    # a bad line in the third window after two clean ones
    rng = random.Random(53)
    lines = [S.rec(b"m%d" % i, S._seq(rng, 30)) for i in range(12)]
    k = next(i for i in range(12) if len(S.HD) + sum(len(r) for r in lines[:i]) > 2 * 200)
    nine = b"\t".join([b"nine", b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0", b"ACGT"]) + b"\n"
    bad = [S.sam(lines[:k] + [line] + lines[k:]) for line in (S.rec(b"mapped", S._seq(rng, 30), flag=b"0"), nine, S.rec(b"fx", b"ACGT", flag=b"4x"))]
    knobs_for(knobs, 200, 64)
    good = S.sam(lines)
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
    starts = record_starts(good)
    dented = bytearray(good)
    at = starts[k] + len(b"m%d\t" % k)
    assert dented[at:at + 2] == b"4\t"
    dented[at] = ord("0")
    with pytest.raises(_ffi.UnprovenInput) as ei:
        ctx.open_reads_mapped(bytes(dented), m_good, [k], flags())
    assert "the map does not fit the input" in str(ei.value)
    upload_still_works(ctx)
    m_good.free()
    # what the scan leaves to the host stays unproven at either window (the two texts without the magic are not SAM to the sniff and
    # never reach this scan)
    for name, text, _ in S.unproven():
        if not name.startswith("starts_with_"):
            assert text[:3] == b"@HD"
        else:
            continue
        for window in (200, 3001):
            knobs_for(knobs, window, 64)
            for call in (lambda: ctx.census_reads(text, flags()), lambda: ctx.open_reads_selected(text, [0], flags())):
                with pytest.raises(_ffi.UnprovenInput) as ei:
                    call()
                assert ei.value.code == _ffi.ERR_UNPROVEN, (name, window)
    upload_still_works(ctx)
    # bad selections keep their wording; a map of another input; a SAM map without the flags
    knobs_for(knobs, 3001, 512)
    other = refs["names"]
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
        for fl in (flags(sel=False), flags(sam=False), _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP):
            with pytest.raises(_ffi.UnprovenInput) as ei:
                ctx.open_reads_mapped(data, m, [0], fl)
            assert ei.value.code == _ffi.ERR_UNPROVEN and only in str(ei.value), (how, fl)
        upload_still_works(ctx)
        dr = ctx.open_reads_mapped(data, m, [ref.n - 1], flags())
        assert dr.names == [ref.names[-1]]
        dr.free(); m.free()


@pytest.mark.parametrize("args", [["-T", "300", "-Q", "100"], ["-n", "200"]])
@pytest.mark.parametrize("bgzip", [False, True])
def test_cli_sampled_sam_equals_device_ingest(tmp_path, args, bgzip):
    """the golden toy reads as SAM text and as bgzipped SAM: lrge-hip --gpu-ingest, with --gpu-sample and with --gpu-seek too print
    the same estimate, and each says which route ran"""
    from lrge_amd import build as Bd
    names, seqs = toy_reads()
    text = S.toy_sam(names, seqs)
    src = tmp_path / ("toy.sam.gz" if bgzip else "toy.sam")
    src.write_bytes(W.bgzf_compress(text) if bgzip else text)
    cmd = [Bd.CLI_PATH, str(src)] + args + ["-s", "6", "-f"]
    runs = [subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300) for extra in (["--gpu-ingest"], ["--gpu-ingest", "--gpu-sample"], ["--gpu-ingest", "--gpu-sample", "--gpu-seek"])]
    assert all(r.returncode == 0 for r in runs), [r.stderr for r in runs]
    assert runs[0].stdout == runs[1].stdout == runs[2].stdout and runs[0].stdout.strip(), [r.stdout for r in runs]
    assert "gpu-ingest: device\n" in runs[0].stderr and "gpu-ingest: device (sampled)\n" in runs[1].stderr and "gpu-ingest: device (sampled, seek)\n" in runs[2].stderr, [r.stderr for r in runs]
    warn = lambda s: [ln for ln in s.splitlines() if ln.startswith("[WARN]")]   # noqa: E731
    assert warn(runs[0].stderr) == warn(runs[1].stderr) == warn(runs[2].stderr)
