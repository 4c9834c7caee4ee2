"""The seek map and the mapped second pass on the device (lrge_hip_reads_census_map*, lrge_hip_reads_open_mapped*; k_fx_seek,
k_fx_runs) against the host twin's map and plan and against the handle of the selected open on the same
input: raw and in BGZF blocks of 3000 bytes, through windows of a few thousand bytes, at strides below a record, around a
block and above the text.  The shapes are the smallest at which the kernels can go wrong: runs that start and end at every
residue, a chosen record first or last in a run, runs that share a BGZF block, a record of hundreds of cells."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bam_corpus as B
import fastx_corpus as F
import sam_corpus as S
import zstd_corpus as Z
from test_fastx_seek_twin import bgzf_table, bind, census_map, seek_plan, seek_selections
from test_gpu_ingest_selected import CASES, Ref, flags, set_knobs, window_records
from test_gpu_ingest_windowed import upload_still_works, wrap

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WRAPS = ["raw", "bgzf"]
WINDOWS = [3001, 20000]
STRIDES = [512, 3000, 70000, 1 << 20]


@pytest.fixture(scope="module")
def twin():
    from lrge_amd import build as Bd
    return bind(C.CDLL(Bd.build_fastx_twin()))


@pytest.fixture(scope="module")
def refs(ctx, tmp_path_factory):
    p = tmp_path_factory.mktemp("seek_host") / "in.txt"
    cases = dict(F.well_formed())
    return {name: Ref(ctx, p, name, cases[name]) for name in CASES}


def knobs_for(knobs, window, stride):
    set_knobs(knobs, window)
    knobs.set("INGEST_SEEK_STRIDE_BYTES", stride)


def twin_map(twin, text, window, stride):
    rc, out, pts = census_map(twin, text, window, window, stride, tile=4096)
    assert rc == 0
    return pts


def twin_stats(twin, data, how, sel):
    """what seek_stats() must say, by the twin's plan on its last map"""
    rc, st, runs, _ = seek_plan(twin, sel, bgzf_table(data) if how == "bgzf" else None, len(data))
    assert rc == 0
    return st


def same_handle(a, b, what):
    assert a.names == b.names and np.array_equal(a.lens, b.lens) and a.text_bytes == b.text_bytes, what
    assert a.select_stats() == b.select_stats() and a.window_stats()[1] == b.window_stats()[1], (what, a.select_stats(), b.select_stats())


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("how", WRAPS)
def test_map_equals_the_twin(ctx, knobs, refs, twin, how, window):
    """the counts are the plain census's, the points the twin's, the block of every point the one that holds its offset; a census
    without a map returns what it returned"""
    for stride in STRIDES:
        knobs_for(knobs, window, stride)
        for name in CASES:
            ref = refs[name]
            data = wrap(ref.text, how)
            plain = ctx.census_reads(data, flags())
            counts, m = ctx.census_map_reads(data, flags())
            what = (name, how, window, stride)
            assert counts == plain and counts[:3] == (ref.n, ref.bases, len(ref.text)), what
            want = twin_map(twin, ref.text, window, stride)
            pts = m.points()
            assert [(o, t) for o, t, _ in pts] == want, what
            assert m.stats() == (ref.n, len(want), stride, len(ref.text)), what
            if how == "bgzf":
                c_len, isize = bgzf_table(data)
                c_at, o_at = np.concatenate([[0], np.cumsum(c_len)]), np.concatenate([[0], np.cumsum(isize)])
                for _, t, c in pts:
                    b = int(np.searchsorted(o_at, t, side="right")) - 1
                    assert c == c_at[b] and o_at[b] <= t < o_at[b + 1], (what, t, c)
            else:
                assert all(c == 0 for _, _, c in pts), what
            assert ctx.census_reads(data, flags()) == plain, what
            m.free()


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("how", WRAPS)
def test_mapped_open_equals_the_selected_open(ctx, knobs, refs, twin, how, window, stride):
    """every selection of every case: the handle of the selected open on the same input, the host's records and sketches, and the
    statistics of the twin's plan"""
    knobs_for(knobs, window, stride)
    for name in CASES:
        ref = refs[name]
        data = wrap(ref.text, how)
        _, m = ctx.census_map_reads(data, flags())
        pts = twin_map(twin, ref.text, window, stride)
        sels = dict(ref.sel[window])
        sels.update({k: v for k, v in seek_selections(ref.n, [ref.n], pts).items() if k in ("around the points", "neighbouring cells", "far apart")})
        for kind, sel in sels.items():
            what = (name, how, window, stride, kind)
            dr = ctx.open_reads_mapped(data, m, sel, flags())
            ref.check(dr, sel, what)
            other = ctx.open_reads_selected(data, sel, flags())
            same_handle(dr, other, what)
            assert other.seek_stats() == (0, 0, 0, 0), what
            assert dr.seek_stats() == twin_stats(twin, data, how, sel), (what, dr.seek_stats())
            dr.free(); other.free()
        m.free()


def test_alignment_sweep(ctx, knobs, twin, tmp_path):
    """record lengths that walk 1..40 at stride 1: every record is a point, every second one a run of its own, so the runs start
    and end at every residue mod 16 in the staging and in the block"""
    recs = [(b"r%d" % i, (b"ACGTTGCA" * 6)[i % 7:i % 7 + 1 + i % 40]) for i in range(240)]
    text = F.fasta_text(recs, None)
    ref = Ref(ctx, tmp_path / "in.fa", "walk", text, windows=[3001])
    knobs_for(knobs, 3001, 1)
    sel = list(range(0, ref.n, 2))
    for how in WRAPS:
        data = wrap(text, how)
        counts, m = ctx.census_map_reads(data, flags())
        assert counts[0] == ref.n and m.stats()[1] == ref.n, how
        twin_map(twin, text, 3001, 1)
        dr = ctx.open_reads_mapped(data, m, sel, flags())
        ref.check(dr, sel, (how, "every second"))
        st = dr.seek_stats()
        assert st == twin_stats(twin, data, how, sel) and st[0] == len(sel) and st[1] < len(text), (how, st)
        assert {r0 % 16 for r0 in np.cumsum([0] + [len(n) + len(s) + 3 for n, s in recs])[sel].tolist()} == set(range(16))
        dr.free(); m.free()


def test_many_runs_in_one_batch(ctx, knobs):
    """10 MB of text within one window, every third record chosen at stride 4096: 923 runs and 1692 tiles of 4 KiB in one launch
    of k_fx_runs, a wavefront each, against the selected open of the same input"""
    rng = np.random.default_rng(17)
    recs = [(b"m%d" % i, bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.integers(500, 3000))))) for i in range(3000)]
    text = F.fastq_text(recs)
    assert len(text) > 9 << 20
    knobs_for(knobs, 64 << 20, 4096)
    knobs.unset("INFLATE_CHUNK_BYTES")
    sel = list(range(0, len(recs), 3))
    for how in WRAPS:
        data = wrap(text, how)
        counts, m = ctx.census_map_reads(data, flags())
        assert counts[0] == len(recs), how
        dr = ctx.open_reads_mapped(data, m, sel, flags())
        other = ctx.open_reads_selected(data, sel, flags())
        same_handle(dr, other, how)
        assert dr.names == [recs[i][0] for i in sel] and dr.seek_stats()[:2] == (923, 4923007), (how, dr.seek_stats())
        idx = list(range(0, len(sel), 7))
        a, b = dr.seqset(idx), other.seqset(idx)
        (xa, ya), (xb, yb) = a.sketch(0), b.sketch(0)
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb), how
        a.free(); b.free(); dr.free(); other.free(); m.free()


def test_the_record_of_many_cells_and_windows(ctx, knobs, twin, tmp_path):
    """a small record in front of one that spans hundreds of cells and windows of 64 bytes: chosen, and not chosen"""
    big = (b"ACGTN" * 8000)
    recs = [(b"s", b"AC"), (b"big", big), (b"t", b"GG")]
    for k, text in enumerate((F.fastq_text(recs), F.fasta_text(recs, 60))):
        ref = Ref(ctx, tmp_path / ("in%d.txt" % k), "small_then_big_%d" % k, text, windows=[64])
        for how in WRAPS:
            knobs_for(knobs, 64, 64)
            data = wrap(text, how)
            counts, m = ctx.census_map_reads(data, flags())
            assert counts[:3] == (3, ref.bases, len(text)) and [o for o, _, _ in m.points()] == [0, 2], (how, counts, m.points())
            twin_map(twin, text, 64, 64)
            for sel in ([1], [0, 2], [0, 1, 2], [2]):
                dr = ctx.open_reads_mapped(data, m, sel, flags())
                ref.check(dr, sel, (how, sel))
                st = dr.seek_stats()
                assert st == twin_stats(twin, data, how, sel), (how, sel, st)
                assert (st[1] < 200) == (sel == [2]), (how, sel, st)         # only the last record's run is small
                dr.free()
            m.free()


def test_from_a_path(ctx, knobs, refs, twin, tmp_path):
    """the path form reads only the ranges of the plan; a sparse selection at stride 512 brings less than the text and the file"""
    from lrge_amd import _ffi
    ref = refs["fq_big"]
    knobs_for(knobs, 3001, 512)
    pts = twin_map(twin, ref.text, 3001, 512)
    sparse = [pts[len(pts) // 3][0], pts[-2][0]]
    for how in ("bgzf", "raw"):
        data = wrap(ref.text, how)
        p = tmp_path / ("in_%s.fq" % how)
        p.write_bytes(data)
        counts, m = ctx.census_map_reads(p, flags())
        assert counts[:3] == (ref.n, ref.bases, len(ref.text)), how
        assert [(o, t) for o, t, _ in m.points()] == pts, how
        for fl in (flags(), flags(_ffi.GPU_INGEST_WINDOWED)):
            for kind, sel in (("sparse", sparse), ("every third", ref.sel[3001]["every third"]), ("all", list(range(ref.n))), ("empty", [])):
                dr = ctx.open_reads_mapped(p, m, sel, fl)
                ref.check(dr, sel, (how, kind))
                st = dr.seek_stats()
                assert st == twin_stats(twin, data, how, sel), (how, kind, st)
                mem = ctx.open_reads_mapped(data, m, sel, fl)
                same_handle(dr, mem, (how, kind))
                assert mem.seek_stats() == st, (how, kind)
                if kind == "sparse":
                    assert st[0] == 2 and 0 < st[1] < len(ref.text) // 4 and 0 < st[2] < len(data) // 4, (how, st)
                dr.free(); mem.free()
        m.free()


def test_containers_that_cannot_be_entered(ctx, knobs, refs):
    """gzip and bzip2: the mapped open is the selected open, and says that it brought no run"""
    knobs_for(knobs, 3001, 512)
    ref = refs["fq_big"]
    for how in ("gzip_blocks", "bzip2"):
        data = wrap(ref.text, how)
        counts, m = ctx.census_map_reads(data, flags())
        assert counts == ctx.census_reads(data, flags()) and m.stats()[0] == ref.n, how
        for kind in ("every third", "last", "empty"):
            sel = ref.sel[3001][kind]
            dr = ctx.open_reads_mapped(data, m, sel, flags())
            ref.check(dr, sel, (how, kind))
            other = ctx.open_reads_selected(data, sel, flags())
            same_handle(dr, other, (how, kind))
            assert dr.seek_stats() == (0, 0, 0, 0), how
            dr.free(); other.free()
        m.free()


def test_budget(ctx, knobs, refs):
    """INGEST_MAX_BYTES bounds the chosen bases plus the block: one byte below all the bases, every second read fits and all do not"""
    from lrge_amd import _ffi
    ref = refs["fq_big"]
    knobs_for(knobs, 3001, 512)
    knobs.set("INGEST_MAX_BYTES", ref.bases - 1)
    for how in WRAPS:
        data = wrap(ref.text, how)
        counts, m = ctx.census_map_reads(data, flags())
        assert counts[:2] == (ref.n, ref.bases), how
        sel = list(range(0, ref.n, 2))
        dr = ctx.open_reads_mapped(data, m, sel, flags())
        ref.check(dr, sel, (how, "every second, below the cap"))
        dr.free()
        with pytest.raises(_ffi.UnprovenInput) as ei:
            ctx.open_reads_mapped(data, m, list(range(ref.n)), flags())
        assert "bases and window above INGEST_MAX_BYTES" in str(ei.value), how
        upload_still_works(ctx)
        m.free()


def test_refusals(ctx, knobs, refs):
    """BAM, SAM and Zstandard input with the census's texts; a map of another input, or of the same text in the other container;
    selections that are not ascending or reach the map's records"""
    from lrge_amd import _ffi
    reads = B.big_reads()[:12]
    bam = B.bam([B.record(n.split()[0], s) for n, s in reads])
    sam = S.toy_sam([n.split()[0] for n, _ in reads], [s for _, s in reads])
    every = _ffi.GPU_INGEST_BAM | _ffi.GPU_INGEST_SAM | _ffi.GPU_INGEST_WINDOWED | _ffi.GPU_INGEST_WINDOWED_ALN
    for window in (64, 1 << 20):
        knobs_for(knobs, window, 512)
        for data in (bam, sam):
            for how in ("raw", "bgzf", "gzip_blocks"):
                for fl in (flags(), flags(every)):
                    with pytest.raises(_ffi.UnprovenInput) as ei:
                        ctx.census_map_reads(wrap(data, how), fl)
                    assert ei.value.code == _ffi.ERR_UNPROVEN and "selected ingest takes FASTA / FASTQ only" in str(ei.value), (how, window)
        upload_still_works(ctx)
    ref, other = refs["fq_big"], refs["fa_big_w60_crlf"]
    zst = Z.compress(ref.text)
    with pytest.raises(_ffi.UnprovenInput) as ei:
        ctx.census_map_reads(zst, flags(_ffi.GPU_INFLATE_ZSTD))
    assert "selected ingest takes FASTA / FASTQ only, not Zstandard input" in str(ei.value)
    upload_still_works(ctx)
    knobs_for(knobs, 3001, 512)
    maps = {how: ctx.census_map_reads(wrap(ref.text, how), flags())[1] for how in WRAPS}
    with pytest.raises(_ffi.UnprovenInput) as ei:
        ctx.open_reads_mapped(zst, maps["raw"], [0], flags(_ffi.GPU_INFLATE_ZSTD))
    assert "not Zstandard input" in str(ei.value)
    for how in WRAPS:
        for data in (wrap(other.text, how), wrap(ref.text, "bgzf" if how == "raw" else "raw"), wrap(ref.text, how)[:-1], b""):
            with pytest.raises(_ffi.LrgeHipError) as ei:
                ctx.open_reads_mapped(data, maps[how], [0], flags())
            assert ei.value.code == _ffi.ERR_INVALID and "the map is of another input" in str(ei.value), how
    upload_still_works(ctx)
    for how in WRAPS:
        data = wrap(ref.text, how)
        for sel in ([5, 3], [0, 4, 4, 9]):
            with pytest.raises(_ffi.LrgeHipError) as ei:
                ctx.open_reads_mapped(data, maps[how], sel, flags())
            assert ei.value.code == _ffi.ERR_INVALID and "strictly ascending" in str(ei.value), (how, sel)
        for sel in ([ref.n], [0, ref.n - 1, ref.n + 7]):
            with pytest.raises(_ffi.LrgeHipError) as ei:
                ctx.open_reads_mapped(data, maps[how], sel, flags())
            assert ei.value.code == _ffi.ERR_INVALID and "ordinal %d of %d records" % (sel[-1], ref.n) in str(ei.value), (how, sel)
        upload_still_works(ctx)
        dr = ctx.open_reads_mapped(data, maps[how], [ref.n - 1], flags())
        assert dr.names == [ref.names[-1]]
        dr.free()
    # a text of the map's size that is not the map's: never other records than its own
    shifted = ref.text[1:] + b"\n"
    try:
        dr = ctx.open_reads_mapped(shifted, maps["raw"], [3], flags())
        assert dr.names == [ref.names[3]]
        dr.free()
    except _ffi.UnprovenInput as e:
        assert "the map does not fit the input" in str(e)
    upload_still_works(ctx)
    for m in maps.values():
        m.free()


@pytest.mark.parametrize("args", [["-T", "300", "-Q", "100"], ["-n", "200"]])
def test_cli_seek_equals_device_ingest(tmp_path, args):
    """lrge-hip --gpu-ingest --gpu-sample --gpu-seek prints the estimate of --gpu-ingest alone, and says which route ran"""
    from lrge_amd import build as Bd
    src = tmp_path / "toy_reads.fa.gz"
    shutil.copy(os.path.join(HERE, "golden", "toy_reads.fa.gz"), src)
    cmd = [Bd.CLI_PATH, str(src)] + args + ["-s", "6", "-f"]
    a = subprocess.run(cmd + ["--gpu-ingest"], capture_output=True, text=True, timeout=300)
    b = subprocess.run(cmd + ["--gpu-ingest", "--gpu-sample", "--gpu-seek"], capture_output=True, text=True, timeout=300)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == b.stdout and a.stdout.strip(), (a.stdout, b.stdout)
    assert "gpu-ingest: device (sampled, seek)" in b.stderr and "gpu-ingest: device\n" in a.stderr, (a.stderr, b.stderr)
    warn = lambda s: [ln for ln in s.splitlines() if ln.startswith("[WARN]")]   # noqa: E731
    assert warn(a.stderr) == warn(b.stderr)


def test_cli_seek_requires_sample(tmp_path):
    from lrge_amd import build as Bd
    src = tmp_path / "toy_reads.fa.gz"
    shutil.copy(os.path.join(HERE, "golden", "toy_reads.fa.gz"), src)
    r = subprocess.run([Bd.CLI_PATH, str(src), "--gpu-ingest", "--gpu-seek"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "error: the argument '--gpu-seek' requires '--gpu-sample'" in r.stderr, r.stderr
    c = subprocess.run([Bd.CLI_PATH, str(src), "-n", "200", "-s", "6", "--gpu-ingest", "--gpu-sample"], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0 and "gpu-ingest: device (sampled)\n" in c.stderr, c.stderr
