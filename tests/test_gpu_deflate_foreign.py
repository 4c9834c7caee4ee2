"""The device decoders (k_inflate; k_gz_find / k_gz_decode / k_gz_window / k_gz_resolve; the ingest on top of both) on the
streams of tests/deflate_corpus.py: legal deflate that zlib's encoder never writes, and streams zlib's inflate rejects.  zlib
decides the bytes and accept / reject; a rejected stream ends in ERR_PARSE (UnprovenInput for the ingest) and leaves the
context usable.  TOO_MANY is accepted for the cases of deflate_corpus.DENSE only."""
import random

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

import bgzf_writer as W
import deflate_corpus as K
from test_gpu_ingest import check_against_host, upload_still_works

pytestmark = pytest.mark.gpu


def test_bgzf_cases(ctx):
    from lrge_amd import _ffi
    cases = K.bgzf_cases()
    assert sum(e is None for _, _, e in cases) >= 25 and sum(e is not None for _, _, e in cases) >= 40
    for name, block, exp in cases:
        if exp is None:
            with pytest.raises(_ffi.LrgeHipError) as ei:
                ctx.bgzf_inflate(block + W.EOF_BLOCK)
            assert ei.value.code == _ffi.ERR_PARSE, name
        else:
            assert ctx.bgzf_inflate(block + W.EOF_BLOCK) == exp, name
    # the blocks of different cases in one file: statuses are per block
    good = [(b, e) for _, b, e in cases if e is not None]
    assert ctx.bgzf_inflate(b"".join(b for b, _ in good) + W.EOF_BLOCK) == b"".join(e for _, e in good)
    for k, (name, block, exp) in enumerate(cases):
        if exp is None:
            head = b"".join(b for b, _ in good[:k % len(good)])
            with pytest.raises(_ffi.LrgeHipError) as ei:
                ctx.bgzf_inflate(head + block + b"".join(b for b, _ in good[:3]) + W.EOF_BLOCK)
            assert ei.value.code == _ffi.ERR_PARSE and ("file offset %d:" % len(head)) in str(ei.value), name
    for name, data, off in K.bgzf_reach_files():
        with pytest.raises(_ffi.LrgeHipError) as ei:
            ctx.bgzf_inflate(data)
        assert ei.value.code == _ffi.ERR_PARSE and ("file offset %d:" % off) in str(ei.value), name
    upload_still_works(ctx)


def check_gzip_cases(ctx):
    from lrge_amd import _ffi
    n_rejected = 0
    for name, data, exp in K.gzip_cases():
        if exp is None:
            with pytest.raises(_ffi.LrgeHipError) as ei:
                ctx.gzip_inflate(data)
            assert ei.value.code == _ffi.ERR_PARSE, name
            upload_still_works(ctx)
            n_rejected += 1
            continue
        try:
            out = ctx.gzip_inflate(data)
        except _ffi.LrgeHipError as e:
            assert e.code == _ffi.ERR_TOO_MANY and name in K.DENSE, (name, str(e))
            continue
        assert out == exp, name
    assert n_rejected >= 30


def test_gzip_cases_default(ctx):
    check_gzip_cases(ctx)


def test_gzip_cases_tiny_chunks_and_rounds(ctx, knobs):
    knobs.set("GZIP_CHUNK_BYTES", 512)
    knobs.set("GZIP_ROUND_BYTES", 8192)
    knobs.set("GZIP_SLOT_RATIO", 64)
    check_gzip_cases(ctx)
    out, stats = ctx.gzip_inflate(dict((n, d) for n, d, _ in K.gzip_cases())["provenance_chains_of_distance_32768"], stats=True)
    assert stats["speculative_starts"] > 100 and stats["chunks"] > 200, stats


def test_open_reads_writer_fastq(ctx, tmp_path, knobs):
    from lrge_amd import _ffi
    rng = np.random.default_rng(3)
    for tiny in (False, True):
        if tiny:
            knobs.set("GZIP_CHUNK_BYTES", 512)
            knobs.set("GZIP_ROUND_BYTES", 8192)
            knobs.set("GZIP_SLOT_RATIO", 64)
        for name, (data, fq) in K.fastq_files().items():
            assert check_against_host(ctx, tmp_path, name, fq, data, rng) == 160
        with pytest.raises(_ffi.UnprovenInput):
            ctx.open_reads(K.fastq_rejected())
        upload_still_works(ctx)


@settings(derandomize=True, max_examples=60, deadline=None, database=None)
@given(st.integers(0, 2 ** 32 - 1), st.sampled_from([20, 300, 2000]))
def test_property_streams(ctx, seed, max_tokens):
    raw, plain, _ = K.random_stream(random.Random(seed), max_tokens)
    assert K.zlib_raw(raw) == plain
    if K.bgzf_fits(K.Case("p", raw, plain, plain)):
        block = W.bgzf_block(plain, comp=raw)
        assert ctx.bgzf_inflate(block + block + W.EOF_BLOCK) == plain + plain
    gz = K.member(raw, plain)
    assert ctx.gzip_inflate(gz + gz) == plain + plain               # (defaults: a slot of 4 Mi symbols, far above any example)
    if K.max_piece_output(gz, 512) <= 64 * 512:
        try:
            for k, v in (("GZIP_CHUNK_BYTES", 512), ("GZIP_ROUND_BYTES", 8192), ("GZIP_SLOT_RATIO", 64)):
                ctx.set_option(k, str(v))
            assert ctx.gzip_inflate(gz + gz) == plain + plain
        finally:
            for k in ("GZIP_CHUNK_BYTES", "GZIP_ROUND_BYTES", "GZIP_SLOT_RATIO"):
                ctx.set_option(k, None)
