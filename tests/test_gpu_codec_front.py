"""What the four round decoders (gzip, bzip2, Zstandard, xz) share in front of their kernels, held for each of them: a C sink
that stops the call (LRGE_ERR_IO, its own message, one sink call, a context that goes on working), the stage line of the
*_TIMING options on stderr, the times that are measured without an option, and the record reader's hook.

The hook: test_gpu_gzip.py, test_gpu_bzip2.py, test_gpu_zstd.py and test_gpu_xz.py each hold an accepted file (used_device 1, the
host's records) and a file the device refuses with its flag set (used_device 0, the host's records or message).  What none of
them holds is a refusal that is no parse error: gzip's LRGE_ERR_TOO_MANY must take the host path as well (the case at the foot).

Every input is a few KB but bzip2's, whose smallest multi-block case is bzip2_corpus.three_blocks() (250 KB)."""
import ctypes as C
import gzip
import re

import pytest

import bzip2_corpus as BZ
import xz_writer as XW
import zstd_corpus as ZS

pytestmark = pytest.mark.gpu

STAGE_LINE = {
    "bzip2": r"bzip2 stages ms: find ([\d.]+) entropy ([\d.]+) scatter ([\d.]+) walk ([\d.]+) rle_crc ([\d.]+)",                         # tools/bzip2_bench.py
    "zstd": r"zstd stages ms: heads ([\d.]+) literals ([\d.]+) sequences ([\d.]+) execute ([\d.]+) resolve ([\d.]+) checksum ([\d.]+)",   # tools/zstd_bench.py
    "xz": r"\[lrge_hip\] xz stages ms: walk [\d.]+ upload [\d.]+ decode [\d.]+ check [\d.]+",
}
_INPUTS = {}


def codec_input(codec):
    """(compressed bytes, plain text, options under which the decode takes two rounds); made once"""
    if codec not in _INPUTS:
        if codec == "gzip":
            text = BZ.fastq(4000, 71)
            _INPUTS[codec] = (gzip.compress(text), text, {})
        elif codec == "bzip2":
            _, comp, text = BZ.three_blocks()
            _INPUTS[codec] = (comp, text, {"BZIP2_ROUND_BLOCKS": 2})
        elif codec == "zstd":                               # two frames of one block, each with its content checksum
            a, b = BZ.fastq(3000, 72), BZ.fastq(2500, 73)
            comp = ZS.compress(a) + ZS.compress(b)
            assert ZS.walk(comp)["per_frame"] == [1, 1] and ZS.walk(comp)["checksums"] == 2
            _INPUTS[codec] = (comp, a + b, {"ZSTD_ROUND_BLOCKS": 1})
        else:                                               # one stream of two blocks
            text = BZ.fastq(4000, 74)
            _INPUTS[codec] = (XW.xz_of(text, 2000, XW.CHECK_CRC32), text, {"XZ_MIN_BLOCKS": 1, "XZ_ROUND_BLOCKS": 1})
    return _INPUTS[codec]


def decode(ctx, codec, comp):
    """the ordinary wrapper: (bytes, stats)"""
    if codec == "gzip":
        return ctx.gzip_inflate(comp, stats=True)
    return getattr(ctx, codec + "_inflate")(comp)


@pytest.mark.parametrize("codec", ["gzip", "bzip2", "zstd", "xz"])
def test_a_sink_that_stops(ctx, knobs, codec):
    from lrge_amd import _ffi
    comp, text, opts = codec_input(codec)
    for name, value in opts.items():
        knobs.set(name, value)
    calls = []

    def sink(_user, _p, n):
        calls.append(n)
        return 1
    cb = _ffi.GZIP_SINK(sink)
    rc = getattr(ctx._lib, "lrge_hip_%s_inflate" % codec)(ctx.h, comp, len(comp), cb, None, None)
    msg = ctx._lib.lrge_hip_last_error(ctx.h).decode()
    assert rc == _ffi.ERR_IO and msg == "%s inflate: the sink stopped the call" % codec, (rc, msg)
    assert len(calls) == 1 and 0 < calls[0] <= len(text), calls
    out, st = decode(ctx, codec, comp)                      # the context survived, and the input does take two rounds
    assert out == text, st
    if codec != "gzip":
        assert st["rounds"] == 2 and calls[0] < len(text), (st, calls)


@pytest.mark.parametrize("codec", ["bzip2", "zstd", "xz"])
def test_stage_line(ctx, knobs, capfd, codec):
    comp, text, opts = codec_input(codec)
    for name, value in opts.items():
        knobs.set(name, value)
    capfd.readouterr()
    out, _ = decode(ctx, codec, comp)
    err = capfd.readouterr().err
    assert out == text and "stages ms" not in err, err       # without the option: no such line
    knobs.set(codec.upper() + "_TIMING", 1)
    out, _ = decode(ctx, codec, comp)
    err = capfd.readouterr().err
    assert out == text
    assert len([ln for ln in err.splitlines() if re.search(STAGE_LINE[codec], ln)]) == 1 and err.count("stages ms") == 1, err


def test_times_measured_without_an_option(ctx, knobs):
    comp, text, _ = codec_input("zstd")
    out, st = ctx.zstd_inflate(comp)
    assert out == text and st["checksums_checked"] >= 1 and isinstance(st["checksum_us"], int), st
    comp, text, opts = codec_input("xz")
    for name, value in opts.items():
        knobs.set(name, value)
    out, st = ctx.xz_inflate(comp)
    assert out == text and all(isinstance(st[k], int) for k in ("check_us", "decode_us", "walk_us")), st      # (a clock may round to 0)


def test_hook_takes_the_host_path_on_too_many(ctx, knobs, tmp_path):
    """gzip the device gives up on with LRGE_ERR_TOO_MANY (a chunk beyond its slot, as test_gpu_gzip.test_overflow_retry_and_too_many
    sets it up): the reader's hook hands the file to the host, whose records come back with used_device 0"""
    from lrge_amd import _ffi
    from test_gpu_gzip import read_gpu_ex, read_host
    knobs.set("GZIP_CHUNK_BYTES", 512)
    knobs.set("GZIP_SLOT_RATIO", 1)
    k = 200_000
    comp = gzip.compress(b"@long\n" + b"A" * k + b"\n+\n" + b"I" * k + b"\n", 9)
    with pytest.raises(_ffi.LrgeHipError) as ei:
        ctx.gzip_inflate(comp)
    assert ei.value.code == _ffi.ERR_TOO_MANY
    p = tmp_path / "long.fq.gz"
    p.write_bytes(comp)
    rc_h, rec_h, msg_h = read_host(p)
    rc_g, rec_g, _, used = read_gpu_ex(ctx, p, 3)
    assert rc_h == 0 and rec_h == [(b"long", b"A" * k)], msg_h
    assert (rc_g, used) == (0, 0) and rec_g == rec_h
