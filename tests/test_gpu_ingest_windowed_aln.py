"""Windowed device ingest of unaligned BAM and SAM (LRGE_GPU_INGEST_WINDOWED_ALN beside LRGE_GPU_INGEST_WINDOWED and the format's
flag; bam_round.h's tail mode, k_bam_spans, k_bam_store): text that passes through HBM in windows while only
the bases stay -- BAM's packed -- against the host reader, raw, in BGZF, in gzip and in bzip2, at windows of a few hundred and a
few thousand bytes; INGEST_MAX_BYTES below the text; the counts against the host twin's; the carried tail; the inputs the device
leaves to the host; the CLI."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import bam_corpus as B
import sam_corpus as S
from test_bam_twin import STAT_NAMES, load_twin as load_bam_twin
from test_gpu_ingest_windowed import Ref, read_host, upload_still_works, wrap
from test_sam_twin import load_twin as load_sam_twin

pytestmark = pytest.mark.gpu
WRAPS = ["raw", "bgzf", "gzip_blocks", "multi", "bzip2"]
WINDOWS = [257, 3001, 20000]
SEGMENTS = [64, 4096]
# one item is nearly all of the text: a block that has doubled past it may reach the end of the input before it is flushed
NO_WINDOW_EXPECTED = {"header_refs_100k"}


def flags(extra=0):
    from lrge_amd import _ffi
    return (_ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INFLATE_BZIP2 | _ffi.GPU_INGEST_BAM | _ffi.GPU_INGEST_SAM | _ffi.GPU_INGEST_WINDOWED |
            _ffi.GPU_INGEST_WINDOWED_ALN) & ~extra


def decoder_knobs(knobs):
    knobs.set("INFLATE_CHUNK_BYTES", 20000)
    knobs.set("GZIP_CHUNK_BYTES", 512)
    knobs.set("GZIP_ROUND_BYTES", 8192)
    knobs.set("GZIP_SLOT_RATIO", 64)
    knobs.set("BZIP2_ROUND_BLOCKS", 2)


def big12():
    reads = B.big_reads()[:12]
    names, seqs = [n.split()[0] for n, _ in reads], [s for _, s in reads]
    return B.bam([B.record(n, s) for n, s in zip(names, seqs)]), S.toy_sam(names, seqs)


def all_cases():
    """(kind, name, text): the two corpora and the twelve big reads in either format"""
    bam12, sam12 = big12()
    return [("bam", n, d) for n, d in B.well_formed() + [("big_12", bam12)]] + [("sam", n, d) for n, d in S.well_formed() + [("big_12", sam12)]]


@pytest.fixture(scope="module")
def refs(ctx, tmp_path_factory):
    """the host reader's records and sketches of every case with a record, computed once; None for a case without one"""
    p = tmp_path_factory.mktemp("windowed_aln_host") / "in.bin"
    out = {}
    for kind, name, text in all_cases():
        p.write_bytes(text)
        rc, rec, msg = read_host(p)
        assert rc == 0, (kind, name, msg)
        out[(kind, name)] = Ref(ctx, p, kind + ":" + name, text) if rec else None
    return out


@pytest.fixture(scope="module")
def twins():
    LB, LS = load_bam_twin(), load_sam_twin()
    LB.bam_twin_windowed.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]
    LB.bam_twin_windowed_stats.argtypes = [C.POINTER(C.c_uint64 * 5)]
    LB.bam_twin_windowed_bam_stats.argtypes = [C.c_void_p]
    LS.sam_twin_windowed.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64]
    LS.sam_twin_windowed_stats.argtypes = [C.POINTER(C.c_uint64 * 4)]
    return LB, LS


def twin_counts(twins, kind, text, S_, window):
    """(window_stats, summed BamStats or None) of the twin's run with pieces of a window's size, as raw input is appended"""
    LB, LS = twins
    if kind == "bam":
        assert LB.bam_twin_windowed(text, len(text), S_, window, window) == 0
        st, a = (C.c_uint64 * 5)(), (C.c_uint64 * len(STAT_NAMES))()
        LB.bam_twin_windowed_stats(C.byref(st))
        LB.bam_twin_windowed_bam_stats(a)
        return tuple(int(x) for x in st[:4]), dict(zip(STAT_NAMES, [int(x) for x in a]))
    assert LS.sam_twin_windowed(text, len(text), window, window) == 0
    st = (C.c_uint64 * 4)()
    LS.sam_twin_windowed_stats(C.byref(st))
    return tuple(int(x) for x in st), None


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("how", WRAPS)
def test_corpus_against_the_host(ctx, knobs, refs, twins, how, window):
    """Every case of both corpora through windows of `window` bytes, BAM at both segment sizes: the host's names, lengths and
    sketches.  Raw input arrives in pieces of a window's size, so there the window counts and the summed counts of the BAM scan
    are the twin's, field for field."""
    knobs.set("INGEST_WINDOW_BYTES", window)
    decoder_knobs(knobs)
    n_windowed = 0
    for kind, name, text in all_cases():
        ref = refs[(kind, name)]
        for S_ in SEGMENTS if kind == "bam" else [0]:
            if S_:
                knobs.set("BAM_SEGMENT_BYTES", S_)
            dr = ctx.open_reads(wrap(text, how), flags())
            what = (kind, name, how, window, S_)
            if ref is None:
                assert dr.n == 0 and dr.text_bytes == len(text), what
            else:
                ref.check(dr, what)
            st = dr.window_stats()
            n_windowed += st[0] > 1
            if st[0]:
                spans = int(((ref.lens.astype(np.uint64) + 1) // 2).sum()) if kind == "bam" else int(ref.lens.sum())
                assert st[1] == spans and st[2] <= len(text), (what, st)
            if len(text) < window:                                       # (text of exactly a window may or may not be flushed)
                assert st == (0, 0, 0, 0), (what, st)
            if len(text) > 2 * max(window, 3000) and name not in NO_WINDOW_EXPECTED:
                assert st[0] >= 1, (what, st)
            if how == "raw" and len(text) != window:
                st_t, bam_t = twin_counts(twins, kind, text, S_, window)
                assert st == st_t, (what, st, st_t)
                if kind == "bam" and ref is not None:
                    assert dr.bam_stats == bam_t, (what, dr.bam_stats, bam_t)
            dr.free()
    # (not vacuous.  Raw and BGZF input arrives in pieces of a window or a 3000-byte block; a round of the gzip and bzip2 decoders
    # delivers most of the small cases whole, which is one window, so only the large cases count there)
    assert n_windowed > (40 if window < 20000 and how in ("raw", "bgzf") else 4)


def quality_bam():
    rng = random.Random(61)
    reads = B.big_reads()
    return B.bam([B.record(n.split()[0], s, qual=bytes(rng.randrange(2, 42) for _ in s)) for n, s in reads]), reads


@pytest.mark.parametrize("kind", ["bam", "sam"])
def test_text_above_the_cap(ctx, knobs, tmp_path, kind):
    """INGEST_MAX_BYTES one byte below the text: resident the file is refused, as test_bam_and_sam_stay_resident pins; under the
    new flag it passes through in windows, and the store is below half the text for BAM (4 bits a base against a byte of
    sequence and a byte of quality) and below the text for SAM"""
    from lrge_amd import _ffi
    if kind == "bam":
        text, reads = quality_bam()
    else:
        reads = B.big_reads()
        text = S.toy_sam([n.split()[0] for n, _ in reads], [s for _, s in reads])
    ref = Ref(ctx, tmp_path / "in.bin", kind + "_big", text)
    knobs.set("INFLATE_CHUNK_BYTES", 20000)
    knobs.set("INGEST_MAX_BYTES", len(text) - 1)
    for how in ("raw", "bgzf"):
        for window in (3001, 20000):
            knobs.set("INGEST_WINDOW_BYTES", window)
            dr = ctx.open_reads(wrap(text, how), flags())
            ref.check(dr, (kind, how, window, "below the cap"))
            st = dr.window_stats()
            assert st[0] >= 2 and st[3] > 0, (how, window, st)
            assert st[1] < len(text) // 2 if kind == "bam" else st[1] < len(text), (how, window, st, len(text))
            dr.free()
            with pytest.raises(_ffi.UnprovenInput):
                ctx.open_reads(wrap(text, how), flags(_ffi.GPU_INGEST_WINDOWED_ALN))
            upload_still_works(ctx)
    # the flag alone does nothing: without the format's own flag the text is not taken at all
    with pytest.raises(_ffi.UnprovenInput):
        ctx.open_reads(text, flags(_ffi.GPU_INGEST_BAM | _ffi.GPU_INGEST_SAM))


def test_small_record_in_front_of_a_large_one(ctx, knobs, tmp_path):
    """a cut a few bytes into the block with a tail far longer behind it: the tail is carried through a second block"""
    rng = random.Random(62)
    big = B._seq(rng, 40001, b"ACGTN")
    items = [(b"s", b"AC"), (b"big", big), (b"t", b"GGA")]
    for kind, text, rec_bytes in (("bam", B.bam([B.record(n, s) for n, s in items]), len(B.record(b"big", big))),
                                  ("sam", S.sam([S.rec(n, s) for n, s in items]), len(S.rec(b"big", big)))):
        ref = Ref(ctx, tmp_path / ("in.%s" % kind), "small_then_big_" + kind, text)
        knobs.set("INFLATE_CHUNK_BYTES", 20000)
        for how, window in (("raw", 64), ("raw", 3001), ("bgzf", 64)):
            knobs.set("INGEST_WINDOW_BYTES", window)
            dr = ctx.open_reads(wrap(text, how), flags())
            ref.check(dr, (kind, how, window))
            st = dr.window_stats()
            assert st[0] >= 2 and st[2] > rec_bytes, (kind, how, window, st)
            dr.free()


def test_unproven_lists(ctx, knobs, tmp_path):
    """the inputs the resident scans leave to the host, through windows of 64 bytes: unproven, or the host's records; a refused
    call leaves the context usable"""
    from lrge_amd import _ffi
    knobs.set("INGEST_WINDOW_BYTES", 64)
    knobs.set("BAM_SEGMENT_BYTES", 64)
    decoder_knobs(knobs)
    p = tmp_path / "in.bin"
    n_refused = 0
    for name, text in B.unproven() + [(n, d) for n, d, _ in S.unproven()]:
        p.write_bytes(text)
        rc_h, rec_h, _ = read_host(p)
        for how in ("raw", "bgzf", "gzip_blocks"):
            try:
                dr = ctx.open_reads(wrap(text, how), flags())
            except _ffi.UnprovenInput as e:
                assert e.code == _ffi.ERR_UNPROVEN, (name, how)
                n_refused += 1
                continue
            assert rc_h == 0 and dr.names == [n for n, _ in rec_h] and dr.lens.tolist() == [len(s) for _, s in rec_h], (name, how)
            dr.free()
    assert n_refused >= 3 * (len(B.unproven()) + 10)
    upload_still_works(ctx)


def test_cli_gpu_ingest_windows_a_bam(tmp_path):
    """--gpu-ingest passes the flag: a BAM above a small INGEST_WINDOW_BYTES takes the device route through windows, and the
    estimate is the host route's"""
    from lrge_amd import build as Bd
    from test_gpu_bam import toy_reads
    import bgzf_writer as W
    names, seqs = toy_reads()
    toy = tmp_path / "toy.bam"
    toy.write_bytes(W.bgzf_compress(W.bam_bytes(names, seqs)))
    env = dict(os.environ, LRGE_HIP_INGEST_WINDOW_BYTES="65536", LRGE_HIP_VERBOSE="1")
    args = [Bd.CLI_PATH, str(toy), "-T", "10", "-Q", "5", "-s", "6", "-f"]
    a = subprocess.run(args, capture_output=True, text=True, timeout=300, env=env)
    b = subprocess.run(args + ["--gpu-ingest"], capture_output=True, text=True, timeout=300, env=env)
    assert a.returncode == b.returncode == 0, (a.stderr, b.stderr)
    assert "gpu-ingest: device" in b.stderr and "gpu-ingest" not in a.stderr, b.stderr
    line = [ln for ln in b.stderr.splitlines() if "reads_open:" in ln and " windows, " in ln]
    assert line and int(line[0].split(" text bytes in ")[1].split(" windows")[0]) >= 2, b.stderr
    assert a.stdout == b.stdout and a.stdout.strip(), (a.stdout, b.stdout)
