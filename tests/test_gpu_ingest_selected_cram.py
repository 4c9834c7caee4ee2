"""The sampled device ingest of unaligned CRAM (LRGE_GPU_INGEST_SELECT_CRAM beside LRGE_GPU_INGEST_CRAM in lrge_hip_reads_census*,
_open_selected*, _census_map*, _open_mapped*; k_rans_decode into a scratch of a round's size, k_fx_runs for the chosen reads; DESIGN
section 27) held to the host twin field for field -- counts, names, lengths, cram_stats, select_stats, seek_stats -- and to the full
CRAM open of the same file by the sketch of the read set on the same indices.  The files are the walker's corpus: 7 records a
slice, a read of length 0, '*' names, every BA codec the device takes, every block a round and all blocks in one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cram_corpus as K
import cram_writer as CW
from test_cram_select_twin import CENSUS, CENSUS_MAP, MAPPED, SELECTED, bind, kept, map_points, sampled, selections, stats, walk
from test_cram_twin import STAT_KEYS, load_twin
from test_gpu_ingest import upload_still_works

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ONLY = "selected ingest takes FASTA / FASTQ only"


def flags(sel=True, cram=True):
    from lrge_amd import _ffi
    return _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | (_ffi.GPU_INGEST_CRAM if cram else 0) | (_ffi.GPU_INGEST_SELECT_CRAM if sel else 0)


@pytest.fixture(scope="module")
def twin():
    from lrge_amd import build as B
    return bind(load_twin(B.build_cram_twin()))


def check_handle(twin, dr, data, sel, what, full=None, mapped=False):
    """the handle against the twin's last call on the same file and selection, field for field"""
    want = kept(twin, sel)
    st_t, seek_t, mem = stats(twin)
    n, bases = twin.cram_twin_walk_recs(None, None, 0), sum(walk(twin)[3])
    assert dr.n == len(sel) and dr.names == [nm for nm, _ in want], what
    assert np.array_equal(dr.lens, np.array([len(s) for _, s in want], dtype=np.uint32)), what
    assert dr.text_bytes == bases and dr.select_stats() == (n, len(sel), bases, mem["store"]), (what, dr.select_stats())
    ws = dr.window_stats()
    assert ws[0] == 0 and ws[1] == mem["store"] == sum(len(s) for _, s in want), (what, ws)      # the store holds the chosen bases only
    st = dr.cram_stats()
    assert [st[k] for k in STAT_KEYS] == [st_t[k] for k in STAT_KEYS], (what, st, st_t)
    assert dr.seek_stats() == (seek_t if mapped else (0, 0, 0, 0)), (what, dr.seek_stats(), seek_t)
    if full is not None and sum(len(s) for _, s in want):
        a, b = dr.seqset(list(range(len(sel)))), full.seqset(list(sel))
        (xa, ya), (xb, yb) = a.sketch(0), b.sketch(0)
        assert np.array_equal(a.lens, b.lens) and np.array_equal(xa, xb) and np.array_equal(ya, yb), what
        a.free(); b.free()


@pytest.mark.parametrize("round_bytes", [0, 1])
def test_four_calls_equal_the_twin_and_the_full_open(ctx, knobs, twin, tmp_path, round_bytes):
    """every file of the corpus from memory, a few from a path too: census, census with a map, every selection selected and mapped"""
    knobs.set("CRAM_MIN_BLOCKS", 0)
    if round_bytes:
        knobs.set("CRAM_ROUND_BYTES", 1)                                 # every block a round of its own
    else:
        knobs.unset("CRAM_ROUND_BYTES")
    for i, (name, data) in enumerate(K.file_cases()):
        srcs = [data]
        if i % 5 == 0:
            p = tmp_path / (name + ".cram")
            p.write_bytes(data)
            srcs.append(str(p))
        rc, out = sampled(twin, CENSUS, data, round_bytes=round_bytes)
        assert rc == 0
        slices = walk(twin)[0]
        full = ctx.open_reads(data, flags(sel=False))
        rec = list(zip(full.names, [b"x" * int(n) for n in full.lens]))       # (names and lengths: what `selections` looks at)
        for src in srcs:
            what = (name, round_bytes, src is data)
            assert ctx.census_reads(src, flags()) == tuple(out) == (full.n, full.text_bytes, full.text_bytes, 0), what
            assert sampled(twin, CENSUS_MAP, data, round_bytes=round_bytes)[0] == 0
            head, pts = map_points(twin)
            counts, m = ctx.census_map_reads(src, flags())
            assert counts == tuple(out) and m.stats() == (head[0], head[1], 0, head[3]), (what, m.stats(), head)
            assert m.points() == [(o, off, c_off) for o, off, c_off, _ in pts], what
            for kind, sel in selections(rec, slices).items():
                assert sampled(twin, SELECTED, data, sel, round_bytes=round_bytes)[0] == 0
                dr = ctx.open_reads_selected(src, sel, flags())
                check_handle(twin, dr, data, sel, what + (kind,), full if src is data else None)
                dr.free()
                assert sampled(twin, MAPPED, data, sel, round_bytes=round_bytes)[0] == 0
                dr = ctx.open_reads_mapped(src, m, sel, flags())
                check_handle(twin, dr, data, sel, what + (kind, "mapped"), full if src is data else None, mapped=True)
                dr.free()
            m.free()
        full.free()
    upload_still_works(ctx)


def test_budget(ctx, knobs, twin):
    """ba_rans1 with INGEST_MAX_BYTES at the file's bases: the full open is refused there (tests/test_gpu_cram.py), the selected and
    the mapped open of two reads succeed -- chosen bases plus the largest round fit, by the twin's own figures -- and a cap below
    chosen bases plus the largest single block gives the over-cap text"""
    from lrge_amd import _ffi
    knobs.set("CRAM_MIN_BLOCKS", 0)
    data = K.by_name("ba_rans1")
    full = ctx.open_reads(data, flags(sel=False))
    bases, sel = full.text_bytes, [2, 17]
    assert sampled(twin, CENSUS_MAP, data)[0] == 0
    slices, lens, comp, raw = walk(twin)
    pad = lambda c: (c + 3) & ~3   # noqa: E731
    knobs.set("INGEST_MAX_BYTES", bases)
    with pytest.raises(_ffi.UnprovenInput) as ei:
        ctx.open_reads(data, flags(sel=False))
    assert "reads_open: bases and one round above INGEST_MAX_BYTES (%d)" % bases in str(ei.value)
    counts, m = ctx.census_map_reads(data, flags())
    assert counts == (full.n, bases, bases, 0)
    for what in (SELECTED, MAPPED):
        assert sampled(twin, what, data, sel, cap=bases)[0] == 0
        _, _, mem = stats(twin)
        assert mem["store"] + mem["scratch"] + max(pad(c) for c in comp) <= bases, mem       # chosen bases plus the largest round fit
        dr = ctx.open_reads_selected(data, sel, flags()) if what == SELECTED else ctx.open_reads_mapped(data, m, sel, flags())
        check_handle(twin, dr, data, sel, ("budget", what), full, mapped=what == MAPPED)
        dr.free()
        touched = {slices[i] for i in sel} if what == MAPPED else range(len(comp))
        cap = mem["store"] + max(pad(comp[s]) + raw[s] for s in touched)
        knobs.set("INGEST_MAX_BYTES", cap)
        (ctx.open_reads_selected(data, sel, flags()) if what == SELECTED else ctx.open_reads_mapped(data, m, sel, flags())).free()
        knobs.set("INGEST_MAX_BYTES", cap - 1)
        with pytest.raises(_ffi.UnprovenInput) as ei:
            ctx.open_reads_selected(data, sel, flags()) if what == SELECTED else ctx.open_reads_mapped(data, m, sel, flags())
        assert "chosen bases and one round of CRAM blocks above INGEST_MAX_BYTES (%d)" % (cap - 1) in str(ei.value), str(ei.value)
        knobs.set("INGEST_MAX_BYTES", bases)
    m.free(); full.free()
    upload_still_works(ctx)


def test_refusals(ctx, knobs, twin):
    """without LRGE_GPU_INGEST_SELECT_CRAM the four calls refuse a CRAM exactly as before; CRAM_MIN_BLOCKS 5 and the default refuse
    all four with the full open's text; the refused files by their reason; a refused head only in a touched block; a map of another
    file; bad selections"""
    from lrge_amd import _ffi
    data, other = K.by_name("ba_rans1"), K.by_name("ba_rans0")
    knobs.set("CRAM_MIN_BLOCKS", 0)
    counts, m = ctx.census_map_reads(data, flags())
    n = counts[0]
    calls = (lambda d, f: ctx.census_reads(d, f), lambda d, f: ctx.census_map_reads(d, f), lambda d, f: ctx.open_reads_selected(d, [0, 1], f),
             lambda d, f: ctx.open_reads_mapped(d, m, [0, 1], f))
    for fl in (flags(sel=False), flags(cram=False), _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP,
               flags(sel=False) | _ffi.GPU_INGEST_BAM | _ffi.GPU_INGEST_SAM | _ffi.GPU_INGEST_SELECT_ALN | _ffi.GPU_INGEST_SELECT_SAM | _ffi.GPU_INGEST_WINDOWED):
        for call in calls:
            with pytest.raises(_ffi.UnprovenInput) as ei:
                call(data, fl)
            assert ei.value.code == _ffi.ERR_UNPROVEN and ONLY in str(ei.value), (fl, str(ei.value))
    upload_still_works(ctx)
    for min_blocks in (5, None):                                         # None: the default, 32 (the file has 4)
        if min_blocks:
            knobs.set("CRAM_MIN_BLOCKS", min_blocks)
        else:
            knobs.unset("CRAM_MIN_BLOCKS")
        for call in calls:
            with pytest.raises(_ffi.UnprovenInput) as ei:
                call(data, flags())
            assert "reads_open: not proven on the device (fewer BA blocks than CRAM_MIN_BLOCKS)" in str(ei.value), str(ei.value)
    knobs.set("CRAM_MIN_BLOCKS", 0)
    for name, bad, reason in K.refused_files():
        for call in calls[:2] + (lambda d, f: ctx.open_reads_selected(d, [0], f),):      # (short_table holds one record)
            with pytest.raises(_ffi.UnprovenInput) as ei:
                call(bad, flags())
            if reason is None:                                           # behind_gzip: the decompressed text is not entered -- the sampled calls' sniff refuses it by name
                assert ei.value.code == _ffi.ERR_UNPROVEN and ONLY in str(ei.value), (name, str(ei.value))
            else:
                assert "reads_open: not proven on the device (" in str(ei.value) and reason in str(ei.value), (name, str(ei.value))
    upload_still_works(ctx)
    # a gzip BA block in the second slice only (tests/test_cram_select_twin.py): the mapped open meets it only when it touches slice 1
    R = K.reads(14, 3, 1, 200)
    good = CW.write_cram(R, method="gzip", records_per_slice=7, method_for={"BA": "rans0"})
    blk = next(b for b in (CW.block("rans0", 4, cid, b"".join(s for _, s in R[7:])) for cid in range(64)) if good.count(b) == 1)
    at = good.index(blk)
    bad = good[:at] + bytes([CW.METHODS["gzip"]]) + good[at + 1:]
    for call in calls[:3]:
        with pytest.raises(_ffi.UnprovenInput) as ei:
            call(bad, flags())
        assert "a BA block in gzip" in str(ei.value)
    _, m2 = ctx.census_map_reads(good, flags())
    assert sampled(twin, CENSUS_MAP, good)[0] == 0 and sampled(twin, MAPPED, bad, [0, 3])[0] == 0
    dr = ctx.open_reads_mapped(bad, m2, [0, 3], flags())
    check_handle(twin, dr, bad, [0, 3], "the bad block is not touched", mapped=True)
    dr.free()
    with pytest.raises(_ffi.UnprovenInput) as ei:
        ctx.open_reads_mapped(bad, m2, [0, 9], flags())
    assert "a BA block in gzip" in str(ei.value)
    upload_still_works(ctx)
    # a map of another file, a map of another kind, a CRAM map on other input
    for wrong in (other, data + b"\0"):
        with pytest.raises(_ffi.LrgeHipError) as ei:
            ctx.open_reads_mapped(wrong, m, [0], flags())
        assert ei.value.code == _ffi.ERR_INVALID and "the map is of another input" in str(ei.value)
    with pytest.raises(_ffi.LrgeHipError) as ei:
        ctx.open_reads_mapped(good, m, [0], flags())
    assert ei.value.code == _ffi.ERR_INVALID and "the map is of another input" in str(ei.value)
    fq = b"@r\nACGT\n+\nIIII\n"
    _, mfq = ctx.census_map_reads(fq, flags())
    # (the last: Zstandard that the sampled calls refuse by name under its flag -- a CRAM map on it is of another input first)
    for src, mp, fl in ((data, mfq, flags()), (fq, m, flags()), (b"\x28\xb5\x2f\xfd" + fq, m, flags() | _ffi.GPU_INFLATE_ZSTD)):
        with pytest.raises(_ffi.LrgeHipError) as ei:
            ctx.open_reads_mapped(src, mp, [0], fl)
        assert ei.value.code == _ffi.ERR_INVALID and "the map is of another input" in str(ei.value)
    mfq.free(); m2.free()
    # bad selections keep their wording
    for sel in ([5, 3], [0, 4, 4, 9]):
        for call in (lambda: ctx.open_reads_selected(data, sel, flags()), lambda: ctx.open_reads_mapped(data, m, sel, flags())):
            with pytest.raises(_ffi.LrgeHipError) as ei:
                call()
            assert ei.value.code == _ffi.ERR_INVALID and "strictly ascending" in str(ei.value), sel
    for sel in ([n], [0, n - 1, n + 7]):
        for call in (lambda: ctx.open_reads_selected(data, sel, flags()), lambda: ctx.open_reads_mapped(data, m, sel, flags())):
            with pytest.raises(_ffi.LrgeHipError) as ei:
                call()
            assert ei.value.code == _ffi.ERR_INVALID and "ordinal %d of %d records" % (sel[-1], n) in str(ei.value), sel
    dr = ctx.open_reads_mapped(data, m, [n - 1], flags())
    assert dr.n == 1
    dr.free(); m.free()
    upload_still_works(ctx)


def test_cli_sampled_cram_equals_device_ingest(tmp_path):
    """a file of one record a slice, 32 slices and more: lrge-hip --gpu-ingest --gpu-cram, with --gpu-sample and with --gpu-seek too
    print the same estimate, and each says which route ran"""
    from lrge_amd import build as B, readio
    tn, ts = readio.load(os.path.join(GOLDEN, "toy_reads.fa.gz"))
    recs, total = [], 0
    for n, s in zip(tn, ts):
        if total + len(s) > 200_000:
            break
        recs.append((n if isinstance(n, bytes) else n.encode(), s if isinstance(s, bytes) else bytes(s)))
        total += len(s)
    assert len(recs) >= 32                                               # (the default of CRAM_MIN_BLOCKS is 32 blocks: the CLI sets no options)
    p = tmp_path / "toy.cram"
    p.write_bytes(CW.write_cram(recs, method="gzip", records_per_slice=1, slices_per_container=8, method_for={"BA": "rans1"}))
    cmd = [B.CLI_PATH, str(p), "-T", "10", "-Q", "5", "-s", "1", "-f", "--gpu-ingest", "--gpu-cram"]
    runs = [subprocess.run(cmd + extra, capture_output=True, text=True, timeout=120) for extra in ([], ["--gpu-sample"], ["--gpu-sample", "--gpu-seek"])]
    assert all(r.returncode == 0 for r in runs), [r.stderr for r in runs]
    assert runs[0].stdout == runs[1].stdout == runs[2].stdout and runs[0].stdout.strip(), [r.stdout for r in runs]
    assert "gpu-ingest: device\n" in runs[0].stderr and "gpu-ingest: device (sampled)\n" in runs[1].stderr and "gpu-ingest: device (sampled, seek)\n" in runs[2].stderr, [r.stderr for r in runs]
    # without --gpu-cram the sampled route does not take the file: the host reads it, as before
    d = subprocess.run([a for a in cmd if a != "--gpu-cram"] + ["--gpu-sample"], capture_output=True, text=True, timeout=120)
    assert d.returncode == 0 and d.stdout == runs[0].stdout and "gpu-ingest: host" in d.stderr, d.stderr
