"""xz decompressed on the device (k_xz_decode / k_xz_check): byte-equal to liblzma and to the host twin over the corpus of
tests/xz_corpus.py and the streams of tests/xz_writer.py, the twin's stats field for field at both round and launch settings, read
sets opened from xz text kept in HBM (resident and through windows) against the host reader, what is not accepted, the check
option, the fall-back of the record reader, the CLI.  The largest text is 600 KB."""
import os
import subprocess

import numpy as np
import pytest

import bgzf_writer as W
import xz_corpus as X
import xz_writer as XW
from test_gpu_ingest import check_seqset, read_host, upload_still_works
from test_xz_twin import STAT_KEYS, load_twin, not_accepted_cases, run as run_twin

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def xtwin():
    from lrge_amd import build as B
    return load_twin(B.build_xz_twin())


def inflate_flags():
    from lrge_amd import _ffi
    return _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INFLATE_XZ


def gpu_cases():
    """the corpus and the writer's streams with texts of at most 600 KB"""
    return [c for c in X.cases() + XW.cases(big=False) if len(c[2]) <= 600_000]


@pytest.mark.parametrize("round_blocks,launch_bytes", [(0, 0), (2, 1)])
def test_streams_and_stats_equal_liblzma_and_the_twin(ctx, knobs, xtwin, round_blocks, launch_bytes):
    knobs.set("XZ_MIN_BLOCKS", 0)
    if round_blocks:
        knobs.set("XZ_ROUND_BLOCKS", round_blocks)
        knobs.set("XZ_LAUNCH_BYTES", launch_bytes)
    cases = gpu_cases()
    assert len(cases) >= 30 and {"one_block_300k", "controls_mid_block", "slot_classes", "three_streams_padded", "incompressible_stretches"} <= {c[0] for c in cases}
    for name, comp, plain in cases:
        out, st = ctx.xz_inflate(comp)
        rc, out_t, st_t, _ = run_twin(xtwin, comp, round_blocks, launch_bytes)
        assert rc == 0 and out_t == plain, name
        assert out == plain, (name, st)
        assert [st[k] for k in STAT_KEYS] == [st_t[k] for k in STAT_KEYS], (name, st, st_t)
    _, st = ctx.xz_inflate(X.by_name("one_block_300k")[1])
    assert st["blocks"] == 1 and st["launches"] == (st["chunks"] if launch_bytes else 1) and st["chunks"] >= 3, st
    _, st = ctx.xz_inflate(X.by_name("fastq_p6")[1])
    assert st["blocks"] == 4 and st["rounds"] == (2 if round_blocks else 1) and st["checks_checked"] == 4, st


def fastq_files():
    """(tag, xz bytes, text): multi-block, multi-stream with padding, one block of three chunks"""
    fq = X.fastq(300_000, 62)
    cut1, cut2 = fq.index(b"\n@read", 100_000) + 1, fq.index(b"\n@read", 200_000) + 1
    multi = XW.xz_of(fq, 70_000, XW.CHECK_CRC64)
    streams = (XW.xz_of(fq[:cut1], 40_000, XW.CHECK_CRC32) + b"\0" * 8 + XW.xz_of(fq[cut1:cut2], 100_000, XW.CHECK_NONE, sizes=False) + XW.stream([]) +
               XW.xz_of(fq[cut2:], 30_000, XW.CHECK_CRC64, preset=1) + b"\0" * 4)
    one = XW.xz_of(fq, len(fq), XW.CHECK_CRC32, preset=1)
    assert X.walk(multi)["blocks"] == 5 and X.walk(streams)["streams"] == 4 and X.walk(one)["per_block"][0] >= 3
    return [("five_blocks", multi, fq), ("four_streams_padded", streams, fq), ("one_block_three_chunks", one, fq)]


def test_open_reads_from_xz(ctx, tmp_path, knobs):
    from lrge_amd import _ffi
    knobs.set("XZ_MIN_BLOCKS", 1)
    files = fastq_files()
    for tag, comp, plain in files:
        p = tmp_path / (tag + ".fq.xz")
        p.write_bytes(comp)
        rc_h, rec_h, msg = read_host(p)
        assert rc_h == 0 and len(rec_h) > 100, msg
        seqs = [s for _, s in rec_h]
        for round_blocks, launch_bytes in ((0, 0), (2, 1)):
            if round_blocks:
                knobs.set("XZ_ROUND_BLOCKS", round_blocks)
                knobs.set("XZ_LAUNCH_BYTES", launch_bytes)
            else:
                knobs.unset("XZ_ROUND_BLOCKS")
                knobs.unset("XZ_LAUNCH_BYTES")
            for src in (comp, str(p)):
                dr = ctx.open_reads(src, inflate_flags())
                assert dr.n == len(rec_h) and dr.text_bytes == len(plain) and dr.window_stats()[0] == 0
                assert dr.names == [n for n, _ in rec_h]
                assert np.array_equal(dr.lens, np.array([len(s) for s in seqs], dtype=np.uint32))
                check_seqset(ctx, dr, seqs, list(range(dr.n)), (tag, round_blocks))
                dr.free()
    one = files[0][1]
    every_other = (_ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INFLATE_BZIP2 | _ffi.GPU_INFLATE_ZSTD | _ffi.GPU_INGEST_BAM | _ffi.GPU_INGEST_SAM |
                   _ffi.GPU_INGEST_WINDOWED | _ffi.GPU_INGEST_WINDOWED_ALN)
    for flags in (_ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP, every_other):        # without the flag: as before
        with pytest.raises(_ffi.UnprovenInput) as ei:
            ctx.open_reads(one, flags)
        assert "reads_open: bzip2, zstd and xz input is decompressed on the host" in str(ei.value)
    damaged = one[:5000] + bytes([one[5000] ^ 0x10]) + one[5001:]
    with pytest.raises(_ffi.UnprovenInput) as ei:                                    # with it, a damaged file: the new text
        ctx.open_reads(damaged, inflate_flags())
    assert "reads_open: xz data not accepted by the device (" in str(ei.value) and "near file offset" in str(ei.value)
    upload_still_works(ctx)


def test_windowed_xz(ctx, knobs):
    """with LRGE_GPU_INGEST_WINDOWED every finished round passes through the windows: the same reads, more than one window, and
    INGEST_MAX_BYTES below the text is enough (only the bases stay)"""
    from lrge_amd import _ffi
    knobs.set("XZ_MIN_BLOCKS", 1)
    knobs.set("INGEST_WINDOW_BYTES", 50_000)
    for tag, comp, fq in fastq_files():
        ref = ctx.open_reads(comp, inflate_flags())
        for round_blocks in (0, 1):
            if round_blocks:
                knobs.set("XZ_ROUND_BLOCKS", round_blocks)
            else:
                knobs.unset("XZ_ROUND_BLOCKS")
            dr = ctx.open_reads(comp, inflate_flags() | _ffi.GPU_INGEST_WINDOWED)
            # a finished round is flushed at once: rounds of one block give a window per block, the default round one window
            many = round_blocks == 1 and tag != "one_block_three_chunks"
            assert (dr.window_stats()[0] > 1 if many else dr.window_stats()[0] == 1) and dr.text_bytes == len(fq), (tag, dr.window_stats())
            assert dr.names == ref.names and np.array_equal(dr.lens, ref.lens), tag
            idx = list(range(0, dr.n, 7))
            a, b = dr.seqset(idx), ref.seqset(idx)
            xa, ya = a.sketch(0)
            xb, yb = b.sketch(0)
            assert np.array_equal(xa, xb) and np.array_equal(ya, yb), tag
            a.free()
            b.free()
            dr.free()
        ref.free()
    knobs.unset("XZ_ROUND_BLOCKS")
    tag, comp, fq = fastq_files()[0]
    # the cap's edges, as for the other decoders: a round's text must fit, resident or not
    for flags in (inflate_flags(), inflate_flags() | _ffi.GPU_INGEST_WINDOWED):
        knobs.set("INGEST_MAX_BYTES", len(fq) - 1)
        with pytest.raises(_ffi.UnprovenInput) as ei:
            ctx.open_reads(comp, flags)
        assert "reads_open: text above INGEST_MAX_BYTES (%d)" % (len(fq) - 1) in str(ei.value)
    knobs.set("INGEST_MAX_BYTES", len(fq))
    ctx.open_reads(comp, inflate_flags()).free()
    # by rounds of one block the windows carry the text through a cap below it: only the bases stay
    knobs.set("XZ_ROUND_BLOCKS", 1)
    knobs.set("INGEST_MAX_BYTES", len(fq) - 1)
    dr = ctx.open_reads(comp, inflate_flags() | _ffi.GPU_INGEST_WINDOWED)
    assert dr.window_stats()[0] > 1
    dr.free()
    knobs.set("INGEST_MAX_BYTES", 60_000)                                          # below one block's text
    with pytest.raises(_ffi.UnprovenInput) as ei:
        ctx.open_reads(comp, inflate_flags() | _ffi.GPU_INGEST_WINDOWED)
    assert "reads_open: text above INGEST_MAX_BYTES (60000)" in str(ei.value)
    upload_still_works(ctx)


def test_not_accepted(ctx, knobs):
    from lrge_amd import _ffi
    knobs.set("XZ_MIN_BLOCKS", 0)
    for name, data, status, at, host in not_accepted_cases():
        with pytest.raises(_ffi.LrgeHipError) as ei:
            ctx.xz_inflate(data)
        assert ei.value.code == _ffi.ERR_PARSE and "xz data at file offset" in str(ei.value), (name, str(ei.value))
        if isinstance(at, tuple):
            at = X.walk(data)["chunk_at"][at[1]][0]
        if at is not None:
            assert "file offset %d:" % at in str(ei.value), (name, at, str(ei.value))
        if name in ("wrong_check", "delta_filter", "truncated_in_a_block", "distance_beyond_the_block", "range_coder_one_byte_long"):
            with pytest.raises(_ffi.UnprovenInput) as ei:
                ctx.open_reads(data, inflate_flags())
            assert "reads_open: xz data not accepted by the device (" in str(ei.value) and "near file offset" in str(ei.value), (name, str(ei.value))
        upload_still_works(ctx)
    three = XW.by_name("three_blocks_crc32_sizes")[1]
    for min_blocks in (4, None):                                                   # None: the default, 64 blocks (BASELINE section 13)
        if min_blocks:
            knobs.set("XZ_MIN_BLOCKS", min_blocks)
        else:
            knobs.unset("XZ_MIN_BLOCKS")
        with pytest.raises(_ffi.LrgeHipError) as ei:
            ctx.xz_inflate(three)
        assert ei.value.code == _ffi.ERR_PARSE and "file offset 0: fewer blocks than XZ_MIN_BLOCKS" in str(ei.value)
        with pytest.raises(_ffi.UnprovenInput) as ei:
            ctx.open_reads(three, inflate_flags())
        assert "reads_open: xz data not accepted by the device (fewer blocks than XZ_MIN_BLOCKS near file offset 0)" in str(ei.value)
    text = XW._noise(6400, 40)
    out, st = ctx.xz_inflate(XW.xz_of(text, 100))                                  # 64 blocks: the default takes them
    assert out == text and st["blocks"] == 64
    upload_still_works(ctx)


def test_check_option(ctx, knobs):
    from lrge_amd import _ffi
    knobs.set("XZ_MIN_BLOCKS", 1)
    _, comp, plain = XW.by_name("three_blocks_crc64_sizes")
    at = X.walk(comp)["check_at"][2]
    flipped = comp[:at] + bytes([comp[at] ^ 1]) + comp[at + 1:]
    with pytest.raises(_ffi.LrgeHipError) as ei:
        ctx.xz_inflate(flipped)
    assert "file offset %d: block check mismatch" % at in str(ei.value)
    knobs.set("XZ_CHECK", 0)
    out, st = ctx.xz_inflate(flipped)
    assert out == plain and st["checks_checked"] == 0 and st["check_us"] == 0
    knobs.set("XZ_CHECK", 1)
    out, st = ctx.xz_inflate(comp)
    assert out == plain and st["checks_checked"] == 3


def test_records_fall_back_to_the_host(ctx, tmp_path, knobs):
    """lrge_hip_read_records_gpu_ex with the flag: the device's records on an accepted file, the host's records or message otherwise"""
    from lrge_amd import _ffi
    from test_gpu_gzip import read_gpu_ex
    knobs.set("XZ_MIN_BLOCKS", 1)
    comp = fastq_files()[1][1]
    ck = X.walk(comp)["check_at"][0]
    cases = {"ok": comp, "trailing": comp + b"junk", "truncated": comp[:len(comp) // 2], "wrong_check": comp[:ck] + bytes([comp[ck] ^ 1]) + comp[ck + 1:]}
    for name, data in cases.items():
        p = tmp_path / (name + ".fq.xz")
        p.write_bytes(data)
        rc_h, rec_h, msg_h = read_host(p)
        rc_g, rec_g, msg_g, used = read_gpu_ex(ctx, p, 1 | 2 | _ffi.GPU_INFLATE_XZ)
        assert rc_g == rc_h and used == (1 if name == "ok" else 0), (name, rc_g, rc_h, used)
        assert (rec_g == rec_h) if rc_h == 0 else (msg_g == msg_h), name
        rc_n, rec_n, _, used_n = read_gpu_ex(ctx, p, 3)                  # without the flag: the host decodes, as before
        assert rc_n == rc_h and used_n == 0 and (rc_h != 0 or rec_n == rec_h), name
    upload_still_works(ctx)


def test_cli_gpu_xz(tmp_path):
    from lrge_amd import build as B, readio
    tn, ts = readio.load(os.path.join(GOLDEN, "toy_reads.fa.gz"))
    p = tmp_path / "toy.fq.xz"
    text = W.fastq_bytes(tn, ts)
    comp = XW.xz_of(text, len(text) // 70 + 1, XW.CHECK_CRC64)                       # (the default of XZ_MIN_BLOCKS is 64: the CLI sets no options)
    assert X.walk(comp)["blocks"] >= 64
    p.write_bytes(comp)
    args = [B.CLI_PATH, str(p), "-T", "10", "-Q", "5", "--seed", "6", "-f"]
    a = subprocess.run(args, capture_output=True, text=True, timeout=120)
    b = subprocess.run(args + ["--gpu-ingest", "--gpu-xz"], capture_output=True, text=True, timeout=120)
    c = subprocess.run(args + ["--gpu-xz"], capture_output=True, text=True, timeout=120)
    d = subprocess.run(args + ["--gpu-ingest"], capture_output=True, text=True, timeout=120)
    assert a.returncode == 0 and b.returncode == 0 and c.returncode == 0 and d.returncode == 0, (a.stderr, b.stderr, c.stderr, d.stderr)
    assert a.stdout == b.stdout == c.stdout == d.stdout and a.stdout.strip()
    assert "gpu-ingest: device" in b.stderr and "gpu-ingest: host" in d.stderr      # --gpu-ingest alone: xz stays with the host
