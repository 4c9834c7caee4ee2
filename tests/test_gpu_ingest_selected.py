"""The device ingest of a sample (lrge_hip_reads_census*, lrge_hip_reads_open_selected*; k_fx_bases, k_fx_pick, k_fx_keep; DESIGN
section 23) against the host reader: a count pass that keeps nothing, then a pass that keeps only the chosen reads -- raw, in
BGZF, in a gzip member of many deflate blocks and in bzip2, through windows of a few thousand bytes and through one window.  The
shapes are the smallest at which the kernels can go wrong: a chosen record first or last in a window, windows with nothing
chosen, empty sequences, multi-line CRLF FASTA through the compaction body, unaligned destinations in the store."""
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
from conftest import to_arrays
from test_gpu_ingest_windowed import read_host, upload_still_works, wrap

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["fq_big", "fa_big_w60_crlf", "fq_empty_seqs", "fq_size_4096"]
WRAPS = ["raw", "bgzf", "gzip_blocks", "bzip2"]
WINDOWS = [3001, 20000]


def flags(extra=0):
    from lrge_amd import _ffi
    return _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INFLATE_BZIP2 | extra


def set_knobs(knobs, window):
    knobs.set("INGEST_WINDOW_BYTES", window)
    knobs.set("INFLATE_CHUNK_BYTES", 20000)
    knobs.set("GZIP_CHUNK_BYTES", 512)
    knobs.set("GZIP_ROUND_BYTES", 8192)
    knobs.set("GZIP_SLOT_RATIO", 64)
    knobs.set("BZIP2_ROUND_BLOCKS", 2)


def window_records(text, window):
    """the records of every window of the twin's run with pieces of a window, as raw input arrives on the device"""
    from lrge_amd import build as Bd
    L = C.CDLL(Bd.build_fastx_twin())
    L.fastx_twin_census.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64 * 4)]
    L.fastx_twin_windowed_cuts.argtypes = [C.c_void_p, C.c_uint64]
    L.fastx_twin_windowed_cuts.restype = C.c_uint64
    out = (C.c_uint64 * 4)()
    assert L.fastx_twin_census(text, len(text), 4096, window, window, C.byref(out)) == 0
    k = L.fastx_twin_windowed_cuts(None, 0)
    a = np.zeros(max(1, k), dtype=np.uint64)
    L.fastx_twin_windowed_cuts(a.ctypes.data, k)
    return a[:k].tolist()


def selections(n, per_window):
    """the selections of tests/test_fastx_select_twin.py"""
    rng = np.random.default_rng(5)
    sels = {"empty": [], "first": [0], "last": [n - 1], "all": list(range(n)), "every third": list(range(0, n, 3)),
            "random half": sorted(rng.permutation(n)[:n // 2].tolist())}
    edges, r0 = set(), 0
    for m in per_window:
        if m:
            edges |= {r0, r0 + m - 1}
        r0 += m
    sels["around the cuts"] = sorted(edges)
    return sels


class Ref:
    """the host reader's records of one text; per window its selections, and the sketches of a host upload of each selection and of
    a shuffled half of it under both presets, computed once"""

    def __init__(self, ctx, path, name, text, windows=WINDOWS):
        path.write_bytes(text)
        rc, rec, msg = read_host(path)
        assert rc == 0, (name, msg)
        self.ctx, self.name, self.text = ctx, name, text
        self.names, self.seqs = [n for n, _ in rec], [s for _, s in rec]
        self.lens = np.array([len(s) for s in self.seqs], dtype=np.uint32)
        self.n, self.bases = len(rec), int(self.lens.sum())
        self.sel = {w: selections(self.n, window_records(text, w)) for w in windows}
        self._sk = {}

    def sketches(self, idx):
        key = tuple(idx)
        if key not in self._sk:
            seqs = [self.seqs[i] for i in idx]
            self._sk[key] = None
            if sum(len(s) for s in seqs):
                H = self.ctx.upload(*to_arrays(seqs))
                self._sk[key] = [H.sketch(preset) for preset in (0, 1)]
                H.free()
        return self._sk[key]

    def check(self, dr, sel, what):
        k = len(sel)
        assert dr.n == k and dr.text_bytes == len(self.text), (self.name, what)
        assert dr.names == [self.names[i] for i in sel], (self.name, what)
        assert np.array_equal(dr.lens, self.lens[sel] if k else np.zeros(0, dtype=np.uint32)), (self.name, what)
        assert dr.select_stats() == (self.n, k, self.bases, int(self.lens[sel].sum()) if k else 0), (self.name, what, dr.select_stats())
        assert dr.window_stats()[1] == (int(self.lens[sel].sum()) if k else 0), (self.name, what)
        sub = np.random.default_rng(11).permutation(k)[:max(1, k // 2)].tolist() if k else []
        for kind, jdx in (("all", list(range(k))), ("shuffled subset", sub)):
            if not jdx:
                continue
            s = dr.seqset(jdx)
            assert s.n == len(jdx) and np.array_equal(s.lens, self.lens[[sel[j] for j in jdx]]), (self.name, what, kind)
            for preset, (xh, yh) in enumerate(self.sketches([sel[j] for j in jdx]) or []):
                xd, yd = s.sketch(preset)
                assert np.array_equal(xd, xh) and np.array_equal(yd, yh), (self.name, what, kind, preset)
            s.free()


@pytest.fixture(scope="module")
def refs(ctx, tmp_path_factory):
    p = tmp_path_factory.mktemp("selected_host") / "in.txt"
    cases = dict(F.well_formed())
    return {name: Ref(ctx, p, name, cases[name]) for name in CASES}


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("how", WRAPS)
def test_census_equals_the_host(ctx, knobs, refs, how, window):
    """records, bases and text bytes are the host reader's; text above two windows went through more than one; the windowed flag
    changes nothing"""
    from lrge_amd import _ffi
    set_knobs(knobs, window)
    for name in CASES:
        ref = refs[name]
        out = ctx.census_reads(wrap(ref.text, how), flags())
        assert out[:3] == (ref.n, ref.bases, len(ref.text)), (name, how, window, out)
        assert out[3] >= 1 and (out[3] > 1 or len(ref.text) <= 2 * window), (name, how, window, out)
        assert ctx.census_reads(wrap(ref.text, how), flags(_ffi.GPU_INGEST_WINDOWED)) == out, (name, how, window)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("how", WRAPS)
def test_selected_open_equals_the_host_subset(ctx, knobs, refs, how, window):
    """every selection of every case: identifiers, lengths, the counts, and the sketches of the kept reads under both presets"""
    set_knobs(knobs, window)
    for name in CASES:
        ref = refs[name]
        data = wrap(ref.text, how)
        for kind, sel in ref.sel[window].items():
            dr = ctx.open_reads_selected(data, sel, flags())
            ref.check(dr, sel, (how, window, kind))
            if kind == "all" and len(ref.text) > 2 * window:
                st = dr.window_stats()
                assert st[0] > 1 and st[2] >= window and st[3] > 0, (name, how, window, st)
            dr.free()


def test_from_a_path_and_under_the_windowed_flag(ctx, knobs, refs, tmp_path):
    from lrge_amd import _ffi
    set_knobs(knobs, 3001)
    ref = refs["fq_big"]
    p = tmp_path / "in.fq.gz"
    p.write_bytes(wrap(ref.text, "bgzf"))
    assert ctx.census_reads(p, flags())[:3] == (ref.n, ref.bases, len(ref.text))
    sel = ref.sel[3001]["every third"]
    for fl in (flags(), flags(_ffi.GPU_INGEST_WINDOWED)):
        dr = ctx.open_reads_selected(p, sel, fl)
        ref.check(dr, sel, "path")
        dr.free()


@pytest.mark.parametrize("window", WINDOWS)
def test_equals_the_existing_route(ctx, knobs, refs, window):
    """open_reads(...).seqset(idx) and open_reads_selected(sorted(idx)) renumbered give the same sketches"""
    from lrge_amd import _ffi
    set_knobs(knobs, window)
    for name in CASES:
        ref = refs[name]
        idx = np.random.default_rng(3).permutation(ref.n)[:max(1, ref.n // 3)].tolist()
        asc = sorted(idx)
        for how in WRAPS:
            data = wrap(ref.text, how)
            a = ctx.open_reads(data, flags(_ffi.GPU_INGEST_WINDOWED))
            b = ctx.open_reads_selected(data, asc, flags())
            sa, sb = a.seqset(idx), b.seqset([asc.index(i) for i in idx])
            assert np.array_equal(sa.lens, sb.lens), (name, how)
            if int(sa.lens.sum()):
                for preset in (0, 1):
                    (xa, ya), (xb, yb) = sa.sketch(preset), sb.sketch(preset)
                    assert np.array_equal(xa, xb) and np.array_equal(ya, yb), (name, how, preset)
            sa.free(); sb.free(); a.free(); b.free()


def test_the_record_of_many_windows(ctx, knobs, tmp_path):
    """a small record in front of one that spans hundreds of windows of 64 bytes: the big record chosen, and not chosen"""
    big = (b"ACGTN" * 8000)
    recs = [(b"s", b"AC"), (b"big", big), (b"t", b"GG")]
    for k, text in enumerate((F.fastq_text(recs), F.fasta_text(recs, 60))):
        ref = Ref(ctx, tmp_path / ("in%d.txt" % k), "small_then_big_%d" % k, text, windows=[64])
        for how in ("raw", "bgzf"):
            set_knobs(knobs, 64)
            data = wrap(text, how)
            out = ctx.census_reads(data, flags())
            assert out[:3] == (3, ref.bases, len(text)) and out[3] >= 2, (how, out)
            for sel in ([1], [0, 2], [0, 1, 2], [2]):
                dr = ctx.open_reads_selected(data, sel, flags())
                ref.check(dr, sel, (how, sel))
                st = dr.window_stats()
                assert st[0] >= 2 and st[2] > len(big), (how, sel, st)
                dr.free()


def test_budget(ctx, knobs, refs):
    """INGEST_MAX_BYTES bounds the chosen bases plus the block: one byte below all the bases, every second read fits and all do not"""
    from lrge_amd import _ffi
    ref = refs["fq_big"]
    set_knobs(knobs, 3001)
    knobs.set("INGEST_MAX_BYTES", ref.bases - 1)
    for how in ("raw", "bgzf"):
        data = wrap(ref.text, how)
        assert ctx.census_reads(data, flags())[:2] == (ref.n, ref.bases), how
        sel = list(range(0, ref.n, 2))
        dr = ctx.open_reads_selected(data, sel, flags())
        ref.check(dr, sel, (how, "every second, below the cap"))
        dr.free()
        with pytest.raises(_ffi.UnprovenInput) as ei:
            ctx.open_reads_selected(data, list(range(ref.n)), flags())
        assert "bases and window above INGEST_MAX_BYTES" in str(ei.value), how
        upload_still_works(ctx)


def test_refusals(ctx, knobs, refs):
    """BAM, SAM and Zstandard input, whatever the flags; selections that are not ascending or reach past the records"""
    from lrge_amd import _ffi
    reads = B.big_reads()[:12]
    bam = B.bam([B.record(n.split()[0], s) for n, s in reads])
    sam = S.toy_sam([n.split()[0] for n, _ in reads], [s for _, s in reads])
    every = _ffi.GPU_INGEST_BAM | _ffi.GPU_INGEST_SAM | _ffi.GPU_INGEST_WINDOWED | _ffi.GPU_INGEST_WINDOWED_ALN
    for window in (64, 1 << 20):
        set_knobs(knobs, window)
        for data in (bam, sam):
            for how in ("raw", "bgzf", "gzip_blocks"):
                for fl in (flags(), flags(every)):
                    for call in (lambda d, f: ctx.census_reads(d, f), lambda d, f: ctx.open_reads_selected(d, [0, 1], f)):
                        with pytest.raises(_ffi.UnprovenInput) as ei:
                            call(wrap(data, how), fl)
                        assert ei.value.code == _ffi.ERR_UNPROVEN and "selected ingest takes FASTA / FASTQ only" in str(ei.value), (how, window)
        upload_still_works(ctx)
    ref = refs["fq_big"]
    zst = Z.compress(ref.text)
    for call in (lambda f: ctx.census_reads(zst, f), lambda f: ctx.open_reads_selected(zst, [0], f)):
        with pytest.raises(_ffi.UnprovenInput) as ei:
            call(flags(_ffi.GPU_INFLATE_ZSTD))
        assert "selected ingest takes FASTA / FASTQ only, not Zstandard input" in str(ei.value)
    upload_still_works(ctx)
    set_knobs(knobs, 3001)
    for how in ("raw", "bgzf"):
        data = wrap(ref.text, how)
        for sel in ([5, 3], [0, 4, 4, 9]):
            with pytest.raises(_ffi.LrgeHipError) as ei:
                ctx.open_reads_selected(data, sel, flags())
            assert ei.value.code == _ffi.ERR_INVALID and "strictly ascending" in str(ei.value), (how, sel)
        for sel in ([ref.n], [0, ref.n - 1, ref.n + 7]):
            with pytest.raises(_ffi.LrgeHipError) as ei:
                ctx.open_reads_selected(data, sel, flags())
            assert ei.value.code == _ffi.ERR_INVALID and "ordinal %d of %d records" % (sel[-1], ref.n) in str(ei.value), (how, sel)
        upload_still_works(ctx)
    dr = ctx.open_reads_selected(ref.text, [ref.n - 1], flags())
    assert dr.names == [ref.names[-1]]
    dr.free()


@pytest.mark.parametrize("args", [["-T", "300", "-Q", "100"], ["-n", "200"]])
def test_cli_sampled_equals_device_ingest(tmp_path, args):
    """lrge-hip --gpu-ingest --gpu-sample prints the estimate of --gpu-ingest alone, and says which route ran"""
    from lrge_amd import build as Bd
    src = tmp_path / "toy_reads.fa.gz"
    shutil.copy(os.path.join(HERE, "golden", "toy_reads.fa.gz"), src)
    cmd = [Bd.CLI_PATH, str(src)] + args + ["-s", "6", "-f"]
    a = subprocess.run(cmd + ["--gpu-ingest"], capture_output=True, text=True, timeout=300)
    b = subprocess.run(cmd + ["--gpu-ingest", "--gpu-sample"], capture_output=True, text=True, timeout=300)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == b.stdout and a.stdout.strip(), (a.stdout, b.stdout)
    assert "gpu-ingest: device (sampled)" in b.stderr and "gpu-ingest: device\n" in a.stderr, (a.stderr, b.stderr)
    warn = lambda s: [ln for ln in s.splitlines() if ln.startswith("[WARN]")]   # noqa: E731
    assert warn(a.stderr) == warn(b.stderr)
