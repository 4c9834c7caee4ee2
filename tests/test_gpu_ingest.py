"""Read sets built on the device from FASTA / FASTQ text (k_fx_* kernels, lrge_hip_reads_*): the corpus of tests/fastx_corpus.py
raw, in BGZF, in one gzip member and in several, against the host reader; records crossing BGZF chunks and gzip rounds; the
inputs the device leaves to the host; a 1.2 GB FASTQ; the memory cap; the CLI with and without --gpu-ingest."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import bgzf_writer as W
import fastx_corpus as F
import gzip_corpus as G
from conftest import to_arrays

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_char), C.c_uint64, C.POINTER(C.c_char), C.c_uint64)


def read_host(path):
    from lrge_amd import _ffi
    L = _ffi.lib()
    out = []
    cb = CB(lambda u, n, nl, b, bl: out.append((C.string_at(n, nl), C.string_at(b, bl))))
    err = C.create_string_buffer(512)
    L.lrge_hip_read_records.argtypes = [C.c_char_p, CB, C.c_void_p, C.c_char_p, C.c_uint64]
    rc = L.lrge_hip_read_records(os.fsencode(str(path)), cb, None, err, 512)
    return rc, out, err.value.decode()


def wrappings(text):
    third = max(1, len(text) // 3)
    return {"raw": text, "bgzf": W.bgzf_compress(text, block=3000), "gzip": G.gz(text),
            "multi": b"".join(G.gz(text[i:i + third], 1 + k % 9) for k, i in enumerate(range(0, max(1, len(text)), third)))}


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


def check_against_host(ctx, tmp_path, name, text, data, rng, sketches=True):
    p = tmp_path / "in.bin"
    p.write_bytes(text)
    rc_h, rec_h, msg = read_host(p)
    assert rc_h == 0, (name, msg)
    dr = ctx.open_reads(data)
    assert dr.n == len(rec_h) and dr.text_bytes == len(text), name
    assert dr.names == [n for n, _ in rec_h], name
    assert np.array_equal(dr.lens, np.array([len(s) for _, s in rec_h], dtype=np.uint32)), name
    seqs = [s for _, s in rec_h]
    if sketches and dr.n:
        n = dr.n
        check_seqset(ctx, dr, seqs, list(range(n)), (name, "all"))
        check_seqset(ctx, dr, seqs, rng.permutation(n)[:max(1, n // 2)].tolist(), (name, "shuffled subset"))
        check_seqset(ctx, dr, seqs, rng.integers(0, n, size=n + 3).tolist(), (name, "repeats"))
    dr.free()
    return len(rec_h)


@pytest.mark.parametrize("wrap", ["raw", "bgzf", "gzip", "multi"])
def test_corpus_on_the_device(ctx, tmp_path, wrap):
    rng = np.random.default_rng(7)
    n = 0
    for name, text in F.well_formed():
        n += check_against_host(ctx, tmp_path, name + "/" + wrap, text, wrappings(text)[wrap], rng)
    assert n > 500


def test_flags_choose_the_decoders(ctx):
    from lrge_amd import _ffi
    text = dict(F.well_formed())["fq_lf_nl"]
    w = wrappings(text)
    for wrap, flags, ok in (("raw", 0, True), ("bgzf", 0, False), ("gzip", 0, False), ("bgzf", 1, True), ("gzip", 1, False), ("bgzf", 2, False),
                            ("gzip", 2, True), ("multi", 3, True)):
        if ok:
            dr = ctx.open_reads(w[wrap], flags)
            assert dr.n == 40
            dr.free()
        else:
            with pytest.raises(_ffi.UnprovenInput):
                ctx.open_reads(w[wrap], flags)
    import bz2
    with pytest.raises(_ffi.UnprovenInput):
        ctx.open_reads(bz2.compress(text))


def test_index_out_of_range_is_invalid(ctx):
    from lrge_amd import _ffi
    dr = ctx.open_reads(dict(F.well_formed())["fa_lf_nl"], 0)
    with pytest.raises(_ffi.LrgeHipError) as ei:
        dr.seqset([0, dr.n])
    assert ei.value.code == _ffi.ERR_INVALID
    S = dr.seqset([])
    assert S.n == 0
    S.free(); dr.free()


def test_records_cross_chunks_and_rounds(ctx, tmp_path, knobs):
    """many BGZF chunks and many gzip rounds: records and lines straddle every internal boundary"""
    knobs.set("INFLATE_CHUNK_BYTES", 20000)
    knobs.set("GZIP_CHUNK_BYTES", 512)
    knobs.set("GZIP_ROUND_BYTES", 8192)
    knobs.set("GZIP_SLOT_RATIO", 64)
    rng = np.random.default_rng(8)
    cases = dict(F.well_formed())
    for name in ("fq_big", "fa_big_w60_crlf", "fa_big_one_line"):
        text = cases[name]
        assert len(text) > 60000
        for wrap in ("bgzf", "gzip", "multi"):
            check_against_host(ctx, tmp_path, name + "/" + wrap, text, wrappings(text)[wrap], rng)


def test_chunks_start_unaligned_in_the_text(ctx, tmp_path, knobs):
    """one block of 2999 bytes per chunk: the chunks start at every residue mod 4 of the text, which the resident block takes
    with the output pointer rounded down to a word (3000-byte and 65280-byte blocks never leave a word boundary)"""
    knobs.set("INFLATE_CHUNK_BYTES", 1)
    text = dict(F.well_formed())["fq_big"][:30000]
    text = text[:text.rindex(b"\n@big") + 1]
    assert len(text) > 8 * 2999
    data = W.bgzf_compress(text, block=2999)
    assert check_against_host(ctx, tmp_path, "fq_big/bgzf2999", text, data, np.random.default_rng(11)) > 0
    assert ctx.bgzf_inflate(data) == text


def upload_still_works(ctx):
    S = ctx.upload(*to_arrays([b"ACGTACGTACGTTTGACCA" * 20, b"GGGTTTACACACGT" * 11]))
    x, _ = S.sketch(0)
    assert x.size > 0
    S.free()


def test_unproven_inputs(ctx):
    from lrge_amd import _ffi
    for name, text in F.unproven():
        for wrap, data in wrappings(text).items():
            with pytest.raises(_ffi.UnprovenInput) as ei:
                ctx.open_reads(data)
            assert ei.value.code == _ffi.ERR_UNPROVEN, (name, wrap)
            upload_still_works(ctx)
    # damaged compressed data is unproven too (the host path reports it): a BGZF block with a flipped payload bit, trailing bytes
    text = dict(F.well_formed())["fq_big"]
    bg = bytearray(W.bgzf_compress(text, block=3000))
    bg[len(bg) // 2] ^= 0x10
    for data in (bytes(bg), G.gz(text) + b"trailing bytes"):
        with pytest.raises(_ffi.UnprovenInput):
            ctx.open_reads(data)
        upload_still_works(ctx)


def test_large_fastq(ctx):
    """the 1.2 GB construction of test_gpu_bgzf.py::test_more_than_1gb, cut on a record boundary so that the repeats are whole records"""
    rng = np.random.default_rng(5)
    seqs = [rng.choice(np.frombuffer(b"ACGT", np.uint8), 1000).tobytes() for _ in range(8000)]
    names = [b"r%d" % i for i in range(len(seqs))]
    fq = W.fastq_bytes(names, seqs)[:16 << 20]
    fq = fq[:fq.rindex(b"\n@r") + 1]
    per = fq.count(b"\n+\n")
    assert fq.count(b"\n") == 4 * per
    one = W.bgzf_compress(fq, eof=False, level=1)
    reps = 72
    dr = ctx.open_reads(one * reps + W.EOF_BLOCK)
    assert dr.text_bytes == reps * len(fq) > 1 << 30
    assert dr.n == reps * per and int(dr.lens.astype(np.uint64).sum()) == reps * per * 1000
    idx = np.random.default_rng(9).choice(dr.n, 1000, replace=False)
    assert [dr.names[i] for i in idx[:50]] == [names[i % per] for i in idx[:50]]
    S = dr.seqset(idx)
    H = ctx.upload(*to_arrays([seqs[i % per] for i in idx]))
    for preset in (0, 1):
        xd, yd = S.sketch(preset)
        xh, yh = H.sketch(preset)
        assert np.array_equal(xd, xh) and np.array_equal(yd, yh), preset
    S.free(); H.free(); dr.free()


def test_memory_cap(ctx, knobs):
    from lrge_amd import _ffi
    text = dict(F.well_formed())["fq_big"]
    knobs.set("INGEST_MAX_BYTES", len(text) - 1)
    for wrap, data in wrappings(text).items():
        with pytest.raises(_ffi.UnprovenInput):
            ctx.open_reads(data)
    knobs.set("INGEST_MAX_BYTES", len(text))
    for wrap, data in wrappings(text).items():
        dr = ctx.open_reads(data)
        assert dr.n == 60
        dr.free()


# ---- end to end ----
def run_cli(args):
    from lrge_amd import build as B
    a = subprocess.run([B.CLI_PATH] + args, capture_output=True, text=True, timeout=300)
    b = subprocess.run([B.CLI_PATH] + args + ["--gpu-ingest"], capture_output=True, text=True, timeout=300)
    path_line = lambda s: [ln for ln in s.splitlines() if "gpu-ingest" not in ln]   # noqa: E731
    assert a.returncode == b.returncode, (a.stderr, b.stderr)
    assert a.stdout == b.stdout, (a.stdout, b.stdout)
    assert path_line(a.stderr) == path_line(b.stderr)
    return a, b


def test_cli_gpu_ingest(tmp_path):
    from lrge_amd import synth
    _, q, t = synth.make_config("tiny_twoset")
    names, seqs = list(t.names) + list(q.names), t.seqs() + q.seqs()
    fq = W.fastq_bytes(names, seqs)
    files = {"toy": os.path.join(GOLDEN, "toy_reads.fa.gz"), "bgzf": str(tmp_path / "s.bgzf.fq.gz"), "gzip": str(tmp_path / "s.fq.gz")}
    open(files["bgzf"], "wb").write(W.bgzf_compress(fq))
    open(files["gzip"], "wb").write(gzip.compress(fq))
    estimates = {"-T": 0, "-n": 0}
    for name, p in files.items():
        for strat in (["-T", "10", "-Q", "5"], ["-n", "40"]):
            a, b = run_cli([p] + strat + ["-s", "6", "-f"])          # (identical whether or not this sample yields an estimate)
            estimates[strat[0]] += a.returncode == 0 and bool(a.stdout.strip())
            assert "gpu-ingest: device" in b.stderr, (name, b.stderr)
    assert estimates["-T"] >= 1 and estimates["-n"] >= 1, estimates   # both strategies were compared on real estimates
    # an unproven file -- FASTQ with an empty line between records -- goes the host way without a word
    k = fq.index(b"\n@", len(fq) // 2) + 1
    bad = tmp_path / "gap.fq"
    bad.write_bytes(fq[:k] + b"\n" + fq[k:])
    a, b = run_cli([str(bad), "-T", "10", "-Q", "5", "-s", "6", "-f"])
    assert a.returncode == 0 and a.stdout.strip() and "gpu-ingest: host" in b.stderr
