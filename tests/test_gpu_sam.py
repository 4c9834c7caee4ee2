"""Read sets built on the device from unaligned SAM text (k_sam_mark, k_sam_records, LRGE_GPU_INGEST_SAM): the corpus of
tests/sam_corpus.py raw, in BGZF and in plain gzip against the host reader; lines crossing BGZF chunks and gzip rounds; the inputs
the device leaves to the host; SAM without the flag; the toy reads; the CLI with and without --gpu-ingest."""
import gzip
import os

import numpy as np
import pytest

import bgzf_writer as W
import gzip_corpus as G
import sam_corpus as S
from test_gpu_bam import check_seqset, read_host, run_cli, toy_reads, upload_still_works

pytestmark = pytest.mark.gpu
WRAPS = ["raw", "bgzf", "gzip"]


def flags():
    from lrge_amd import _ffi
    return _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INGEST_SAM


def wrap(data, how):
    return data if how == "raw" else W.bgzf_compress(data, block=3000) if how == "bgzf" else G.gz(data)


@pytest.fixture(scope="module")
def host_corpus(tmp_path_factory):
    """the host reader's records of every well-formed case, computed once"""
    d = tmp_path_factory.mktemp("sam_host")
    out = {}
    for name, data in S.well_formed():
        p = d / "in.sam"
        p.write_bytes(data)
        rc, rec, msg = read_host(p)
        assert rc == 0, (name, msg)
        out[name] = rec
    return out


def check_against_host(ctx, name, data, wrapped, rec_h, rng, fl=None):
    dr = ctx.open_reads(wrapped, flags() if fl is None else fl)
    assert dr.n == len(rec_h) and dr.text_bytes == len(data), name
    assert dr.names == [n for n, _ in rec_h], name
    assert np.array_equal(dr.lens, np.array([len(s) for _, s in rec_h], dtype=np.uint32)), name
    seqs = [s for _, s in rec_h]
    if dr.n:
        n = dr.n
        check_seqset(ctx, dr, seqs, list(range(n)), (name, "all"))
        check_seqset(ctx, dr, seqs, rng.permutation(n)[:max(1, n // 2)].tolist(), (name, "shuffled half"))
        check_seqset(ctx, dr, seqs, rng.integers(0, n, size=n + 3).tolist(), (name, "repeats"))
    dr.free()
    return len(rec_h)


@pytest.mark.parametrize("how", WRAPS)
def test_corpus_on_the_device(ctx, host_corpus, how):
    rng = np.random.default_rng(7)
    n = 0
    for name, data in S.well_formed():
        n += check_against_host(ctx, "%s/%s" % (name, how), data, wrap(data, how), host_corpus[name], rng)
    assert n > 3200


def test_all_flags_together(ctx, host_corpus):
    """the BAM bit beside the SAM bit changes nothing for SAM text"""
    from lrge_amd import _ffi
    data = dict(S.well_formed())["plain_40"]
    check_against_host(ctx, "plain_40/all flags", data, data, host_corpus["plain_40"], np.random.default_rng(9), flags() | _ffi.GPU_INGEST_BAM)


def test_lines_cross_chunks_and_rounds(ctx, knobs, host_corpus):
    """many BGZF chunks and many gzip rounds: lines straddle every internal boundary of the decoders"""
    knobs.set("INFLATE_CHUNK_BYTES", 20000)
    knobs.set("GZIP_CHUNK_BYTES", 512)
    knobs.set("GZIP_ROUND_BYTES", 8192)
    knobs.set("GZIP_SLOT_RATIO", 64)
    rng = np.random.default_rng(8)
    cases = dict(S.well_formed())
    for name in ("short_3000", "long_200k"):
        data = cases[name]
        assert len(data) > 30000
        for how in ("bgzf", "gzip"):
            check_against_host(ctx, name + "/" + how, data, wrap(data, how), host_corpus[name], rng)


def test_unproven_inputs(ctx):
    from lrge_amd import _ffi
    for name, data, _ in S.unproven():
        for how in WRAPS:
            with pytest.raises(_ffi.UnprovenInput) as ei:
                ctx.open_reads(wrap(data, how), flags())
            assert ei.value.code == _ffi.ERR_UNPROVEN, (name, how)
            upload_still_works(ctx)


def test_sam_without_the_flag_is_unproven(ctx):
    """without the new bit well-formed SAM stays unproven, as before the bit existed"""
    from lrge_amd import _ffi
    cases = dict(S.well_formed())
    for name in ("plain_40", "header_only", "magic_sq", "magic_rg"):
        for how in WRAPS:
            for fl in (_ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP, _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INGEST_BAM):
                with pytest.raises(_ffi.UnprovenInput) as ei:
                    ctx.open_reads(wrap(cases[name], how), fl)
                assert ei.value.code == _ffi.ERR_UNPROVEN, (name, how, fl)
    with pytest.raises(_ffi.UnprovenInput):
        ctx.open_reads(cases["plain_40"])
    upload_still_works(ctx)


def test_header_only_and_no_bam_stats(ctx):
    from lrge_amd import _ffi
    for data in (S.HD, b"@HD", b"@SQ\n\n\n"):
        dr = ctx.open_reads(data, flags())              # no record, as on the host
        assert dr.n == 0 and dr.names == [] and dr.text_bytes == len(data)
        with pytest.raises(_ffi.LrgeHipError) as ei:
            dr.bam_stats
        assert ei.value.code == _ffi.ERR_INVALID
        Q = dr.seqset([])
        assert Q.n == 0
        Q.free(); dr.free()
    dr = ctx.open_reads(dict(S.well_formed())["magic_hd"], flags())
    assert dr.n == 1
    with pytest.raises(_ffi.LrgeHipError) as ei:
        dr.bam_stats
    assert ei.value.code == _ffi.ERR_INVALID
    dr.free()


def test_toy_reads(ctx, tmp_path):
    names, seqs = toy_reads()
    data = S.toy_sam(names, seqs)
    p = tmp_path / "toy.sam"
    p.write_bytes(data)
    rc, rec_h, msg = read_host(p)
    assert rc == 0 and len(rec_h) == 500 and [s for _, s in rec_h] == seqs, msg
    dr = ctx.open_reads(W.bgzf_compress(data), flags())
    assert dr.n == 500 and dr.names == [n for n, _ in rec_h] and dr.text_bytes == len(data)
    assert np.array_equal(dr.lens, np.array([len(s) for _, s in rec_h], dtype=np.uint32))
    idx = np.random.default_rng(11).choice(500, 100, replace=False).tolist()
    check_seqset(ctx, dr, seqs, idx, "toy")
    dr.free()


# ---- end to end ----
def test_cli_gpu_ingest(tmp_path):
    names, seqs = toy_reads()
    toy = tmp_path / "toy.sam"
    toy.write_bytes(S.toy_sam(names, seqs))
    for strat in (["-T", "10", "-Q", "5"], ["-n", "40"]):
        a, b = run_cli([str(toy)] + strat + ["-s", "6", "-f"])
        assert a.returncode == 0 and a.stdout.strip(), a.stderr
        assert "gpu-ingest: device" in b.stderr, b.stderr
        assert "gpu-ingest" not in a.stderr
    # a SAM with a mapped record: the same failure and message both ways, by the host route
    lines = [S.rec(n, s, flag=b"0" if i == 250 else b"4") for i, (n, s) in enumerate(zip(names, seqs))]
    bad = tmp_path / "mapped.sam"
    bad.write_bytes(S.sam(lines))
    a, b = run_cli([str(bad), "-T", "10", "-Q", "5", "-s", "6", "-f"])
    assert a.returncode != 0 and "Mapped records are not supported" in a.stderr
    assert "gpu-ingest: host" in b.stderr


def test_cli_gpu_ingest_compressed(tmp_path):
    """.sam.gz and bgzip SAM: the device route, and the estimate of the plain file's host route"""
    names, seqs = toy_reads()
    data = S.toy_sam(names, seqs)
    gz = tmp_path / "toy.sam.gz"
    with gzip.open(gz, "wb") as fh:
        fh.write(data)
    bg = tmp_path / "toy.bgzf.sam.gz"
    bg.write_bytes(W.bgzf_compress(data))
    out = set()
    for p in (gz, bg):
        a, b = run_cli([str(p), "-T", "10", "-Q", "5", "-s", "6", "-f"])
        assert a.returncode == 0 and "gpu-ingest: device" in b.stderr, b.stderr
        out.add(b.stdout)
    assert len(out) == 1
