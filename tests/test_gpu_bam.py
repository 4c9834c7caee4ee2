"""Read sets built on the device from unaligned BAM (k_bam_* kernels, LRGE_GPU_INGEST_BAM): the corpus of tests/bam_corpus.py raw,
in BGZF and in plain gzip at several segment sizes against the host reader, with the counts of the scan against the host twin's;
records crossing BGZF chunks and gzip rounds; the inputs the device leaves to the host; the toy reads; the CLI with and without
--gpu-ingest."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import bam_corpus as B
import bgzf_writer as W
import gzip_corpus as G
from conftest import to_arrays, write_unaligned_bam
from test_bam_twin import load_twin, twin_stats

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_char), C.c_uint64, C.POINTER(C.c_char), C.c_uint64)
WRAPS = ["raw", "bgzf", "gzip"]


def flags():
    from lrge_amd import _ffi
    return _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INGEST_BAM


def read_host(path):
    from lrge_amd import _ffi
    L = _ffi.lib()
    out = []
    cb = CB(lambda u, n, nl, b, bl: out.append((C.string_at(n, nl), C.string_at(b, bl))))
    err = C.create_string_buffer(512)
    L.lrge_hip_read_records.argtypes = [C.c_char_p, CB, C.c_void_p, C.c_char_p, C.c_uint64]
    rc = L.lrge_hip_read_records(os.fsencode(str(path)), cb, None, err, 512)
    return rc, out, err.value.decode()


def wrap(data, how):
    return data if how == "raw" else W.bgzf_compress(data, block=3000) if how == "bgzf" else G.gz(data)


@pytest.fixture(scope="module")
def host_corpus(tmp_path_factory):
    """the host reader's records of every well-formed case, computed once"""
    d = tmp_path_factory.mktemp("bam_host")
    out = {}
    for name, data in B.well_formed():
        p = d / "in.bam"
        p.write_bytes(data)
        rc, rec, msg = read_host(p)
        assert rc == 0, (name, msg)
        out[name] = rec
    return out


@pytest.fixture(scope="module")
def twin():
    return load_twin()


def check_seqset(ctx, dr, seqs, idx, what):
    S = dr.seqset(idx)
    sel = [seqs[i] for i in idx]
    assert S.n == len(idx) and np.array_equal(S.lens, np.array([len(s) for s in sel], dtype=np.uint32)), what
    if sum(len(s) for s in sel):
        H = ctx.upload(*to_arrays(sel))
        for preset in (0, 1):
            xd, yd = S.sketch(preset)
            xh, yh = H.sketch(preset)
            assert np.array_equal(xd, xh) and np.array_equal(yd, yh), (what, preset)
        H.free()
    S.free()


def check_against_host(ctx, name, data, wrapped, rec_h, rng, stats=None):
    dr = ctx.open_reads(wrapped, flags())
    assert dr.n == len(rec_h) and dr.text_bytes == len(data), name
    assert dr.names == [n for n, _ in rec_h], name
    assert np.array_equal(dr.lens, np.array([len(s) for _, s in rec_h], dtype=np.uint32)), name
    if stats is not None:
        assert dr.bam_stats == stats, name
    seqs = [s for _, s in rec_h]
    if dr.n:
        n = dr.n
        check_seqset(ctx, dr, seqs, list(range(n)), (name, "all"))
        check_seqset(ctx, dr, seqs, rng.permutation(n)[:max(1, n // 2)].tolist(), (name, "shuffled half"))
        check_seqset(ctx, dr, seqs, rng.integers(0, n, size=n + 3).tolist(), (name, "repeats"))
    dr.free()
    return len(rec_h)


@pytest.mark.parametrize("S", [64, 257, 4096])
@pytest.mark.parametrize("how", WRAPS)
def test_corpus_on_the_device(ctx, knobs, twin, host_corpus, how, S):
    knobs.set("BAM_SEGMENT_BYTES", S)
    rng = np.random.default_rng(7)
    n = 0
    for name, data in B.well_formed():
        assert twin.bam_twin_parse(data, len(data), S) == 0, name
        n += check_against_host(ctx, "%s/%s/%d" % (name, how, S), data, wrap(data, how), host_corpus[name], rng, twin_stats(twin))
    assert n > 3200


def test_segment_size_is_clamped(ctx, knobs, twin):
    data = dict(B.well_formed())["plain_40"]
    assert twin.bam_twin_parse(data, len(data), 64) == 0
    knobs.set("BAM_SEGMENT_BYTES", 1)
    dr = ctx.open_reads(data, flags())
    assert dr.n == 40 and dr.bam_stats == twin_stats(twin)
    dr.free()


def test_records_cross_chunks_and_rounds(ctx, knobs, host_corpus):
    """many BGZF chunks and many gzip rounds: records straddle every internal boundary of the decoders"""
    knobs.set("INFLATE_CHUNK_BYTES", 20000)
    knobs.set("GZIP_CHUNK_BYTES", 512)
    knobs.set("GZIP_ROUND_BYTES", 8192)
    knobs.set("GZIP_SLOT_RATIO", 64)
    knobs.set("BAM_SEGMENT_BYTES", 4096)
    rng = np.random.default_rng(8)
    cases = dict(B.well_formed())
    for name in ("big_60", "short_3000", "long_record"):
        data = cases[name]
        assert len(data) > 30000
        for how in ("bgzf", "gzip"):
            check_against_host(ctx, name + "/" + how, data, wrap(data, how), host_corpus[name], rng)


def upload_still_works(ctx):
    S = ctx.upload(*to_arrays([b"ACGTACGTACGTTTGACCA" * 20, b"GGGTTTACACACGT" * 11]))
    x, _ = S.sketch(0)
    assert x.size > 0
    S.free()


def test_unproven_inputs(ctx):
    from lrge_amd import _ffi
    for name, data in B.unproven():
        for how in WRAPS:
            with pytest.raises(_ffi.UnprovenInput) as ei:
                ctx.open_reads(wrap(data, how), flags())
            assert ei.value.code == _ffi.ERR_UNPROVEN, (name, how)
            upload_still_works(ctx)
    # without the new flag BAM stays unproven, as before
    data = dict(B.well_formed())["plain_40"]
    for how in WRAPS:
        with pytest.raises(_ffi.UnprovenInput):
            ctx.open_reads(wrap(data, how))
        with pytest.raises(_ffi.UnprovenInput):
            ctx.open_reads(wrap(data, how), _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP)
    upload_still_works(ctx)


def test_stats_only_for_bam(ctx):
    from lrge_amd import _ffi
    dr = ctx.open_reads(b">a\nACGT\n", flags())
    assert dr.n == 1
    with pytest.raises(_ffi.LrgeHipError) as ei:
        dr.bam_stats
    assert ei.value.code == _ffi.ERR_INVALID
    dr.free()
    dr = ctx.open_reads(B.header(), flags())          # an empty BAM: no records, as on the host
    assert dr.n == 0 and dr.names == [] and dr.bam_stats["segments"] == 0
    S = dr.seqset([])
    assert S.n == 0
    S.free(); dr.free()


def toy_reads():
    txt = gzip.open(os.path.join(GOLDEN, "toy_reads.fa.gz")).read().split(b">")[1:]
    names = [r.split(b"\n", 1)[0].split()[0] for r in txt]
    seqs = [r.split(b"\n", 1)[1].replace(b"\n", b"") for r in txt]
    return names, seqs


def test_toy_reads(ctx, knobs, tmp_path):
    knobs.set("BAM_SEGMENT_BYTES", 65536)
    names, seqs = toy_reads()
    data = W.bam_bytes(names, seqs)
    p = tmp_path / "toy.raw.bam"
    p.write_bytes(data)
    rc, rec_h, msg = read_host(p)
    assert rc == 0 and len(rec_h) == 500, msg
    dr = ctx.open_reads(W.bgzf_compress(data), flags())
    assert dr.n == 500 and dr.names == [n for n, _ in rec_h]
    assert np.array_equal(dr.lens, np.array([len(s) for _, s in rec_h], dtype=np.uint32))
    assert dr.bam_stats["segments"] == -(-(len(data) - len(B.header())) // 65536) > 1
    idx = np.random.default_rng(11).choice(500, 100, replace=False).tolist()
    check_seqset(ctx, dr, [s for _, s in rec_h], idx, "toy")
    dr.free()


# ---- end to end ----
def run_cli(args):
    from lrge_amd import build as Bd
    a = subprocess.run([Bd.CLI_PATH] + args, capture_output=True, text=True, timeout=300)
    b = subprocess.run([Bd.CLI_PATH] + args + ["--gpu-ingest"], capture_output=True, text=True, timeout=300)
    path_line = lambda s: [ln for ln in s.splitlines() if "gpu-ingest" not in ln]   # noqa: E731
    assert a.returncode == b.returncode, (a.stderr, b.stderr)
    assert a.stdout == b.stdout, (a.stdout, b.stdout)
    assert path_line(a.stderr) == path_line(b.stderr)
    return a, b


def test_cli_gpu_ingest(tmp_path):
    names, seqs = toy_reads()
    toy = str(tmp_path / "toy.bam")
    write_unaligned_bam(toy, names, seqs)
    for strat in (["-T", "10", "-Q", "5"], ["-n", "40"]):
        a, b = run_cli([toy] + strat + ["-s", "6", "-f"])
        assert "gpu-ingest: device" in b.stderr, b.stderr
        assert "gpu-ingest" not in a.stderr
    # a BAM with a mapped record: the same failure and message both ways, by the host route
    bad = tmp_path / "mapped.bam"
    bad.write_bytes(W.bgzf_compress(dict(B.unproven())["mapped_middle"]))
    a, b = run_cli([str(bad), "-T", "10", "-Q", "5", "-s", "6", "-f"])
    assert a.returncode != 0 and "Mapped records are not supported" in a.stderr
    assert "gpu-ingest: host" in b.stderr
