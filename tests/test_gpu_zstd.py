"""Zstandard decompressed on the device (k_zs_heads / k_zs_literals / k_zs_sequences / k_zs_execute / k_zs_resolve / k_zs_xxh64):
byte-equal to libzstd and to the host twin over the corpus of tests/zstd_corpus.py and the streams of tests/zstd_writer.py, the
twin's stats field for field at the default round and at rounds of two blocks, read sets opened from Zstandard text kept in HBM
against the host reader, what is not accepted, the checksum option, the fall-back of the record reader, the CLI.  The largest text
is 600 KB."""
import os
import subprocess

import numpy as np
import pytest

import bgzf_writer as W
import zstd_corpus as Z
import zstd_writer as ZW
from test_gpu_ingest import check_seqset, read_host, upload_still_works
from test_zstd_twin import STAT_KEYS, all_cases, load_twin, not_accepted_cases, run as run_twin

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ztwin():
    from lrge_amd import build as B
    return load_twin(B.build_zstd_twin())


def inflate_flags():
    from lrge_amd import _ffi
    return _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INFLATE_ZSTD


@pytest.mark.parametrize("round_blocks", [0, 2])
def test_streams_and_stats_equal_libzstd_and_the_twin(ctx, knobs, ztwin, round_blocks):
    if round_blocks:
        knobs.set("ZSTD_ROUND_BLOCKS", round_blocks)
    for name, comp, plain in all_cases():
        out, st = ctx.zstd_inflate(comp)
        rc, out_t, st_t, _ = run_twin(ztwin, comp, round_blocks)
        assert rc == 0 and out == out_t == plain, name
        assert [st[k] for k in STAT_KEYS] == [st_t[k] for k in STAT_KEYS], (name, st, st_t)
    _, st = ctx.zstd_inflate(Z.by_name("chain_w17")[1])
    assert st["blocks"] == 5 and st["rounds"] == (3 if round_blocks else 1), st


def three_frames():
    """three frames of FASTQ records with a skippable frame between them"""
    fq = Z.fastq(90_000, 61)
    cut1, cut2 = fq.index(b"\n@read", 30_000) + 1, fq.index(b"\n@read", 60_000) + 1
    return Z.compress(fq[:cut1], 3) + Z.skippable(b"index", 2) + Z.compress(fq[cut1:cut2], 19, checksum=False) + Z.compress(fq[cut2:], 1, content_size=False), fq


def test_open_reads_from_zstd(ctx, tmp_path, knobs):
    from lrge_amd import _ffi
    fq = Z.fastq(300_000, 62)
    one = Z.compress(fq, 3)
    assert Z.walk(one)["per_frame"] == [3]
    multi, fq3 = three_frames()
    assert Z.walk(multi)["frames"] == 3 and Z.walk(multi)["skippable_frames"] == 1
    for tag, comp, plain in (("three_blocks", one, fq), ("three_frames", multi, fq3)):
        p = tmp_path / (tag + ".fq.zst")
        p.write_bytes(comp)
        rc_h, rec_h, msg = read_host(p)
        assert rc_h == 0 and len(rec_h) > 100, msg
        seqs = [s for _, s in rec_h]
        for round_blocks in (0, 2):
            if round_blocks:
                knobs.set("ZSTD_ROUND_BLOCKS", round_blocks)
            else:
                knobs.unset("ZSTD_ROUND_BLOCKS")
            for src in (comp, str(p)):
                dr = ctx.open_reads(src, inflate_flags())
                assert dr.n == len(rec_h) and dr.text_bytes == len(plain)
                assert dr.names == [n for n, _ in rec_h]
                assert np.array_equal(dr.lens, np.array([len(s) for s in seqs], dtype=np.uint32))
                check_seqset(ctx, dr, seqs, list(range(dr.n)), (tag, round_blocks))
                dr.free()
    every_other = (_ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INFLATE_BZIP2 | _ffi.GPU_INGEST_BAM | _ffi.GPU_INGEST_SAM | _ffi.GPU_INGEST_WINDOWED |
                   _ffi.GPU_INGEST_WINDOWED_ALN)
    for flags in (_ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP, every_other):        # without the flag: as before
        with pytest.raises(_ffi.UnprovenInput) as ei:
            ctx.open_reads(one, flags)
        assert "reads_open: bzip2, zstd and xz input is decompressed on the host" in str(ei.value)
    xz = b"\xfd7zXZ\x00" + bytes(20)
    with pytest.raises(_ffi.UnprovenInput) as ei:                                    # xz with the flag: the same text
        ctx.open_reads(xz, inflate_flags())
    assert "reads_open: bzip2, zstd and xz input is decompressed on the host" in str(ei.value)


def test_windowed_flag_leaves_zstd_resident(ctx, knobs):
    from lrge_amd import _ffi
    fq = Z.fastq(300_000, 62)
    comp = Z.compress(fq, 3)
    knobs.set("INGEST_WINDOW_BYTES", 50_000)
    dr = ctx.open_reads(comp, inflate_flags() | _ffi.GPU_INGEST_WINDOWED)
    assert dr.window_stats()[0] == 0 and dr.text_bytes == len(fq)
    ref = ctx.open_reads(comp, inflate_flags())
    assert dr.names == ref.names and np.array_equal(dr.lens, ref.lens)
    dr.free()
    ref.free()
    for flags in (inflate_flags(), inflate_flags() | _ffi.GPU_INGEST_WINDOWED):
        knobs.set("INGEST_MAX_BYTES", len(fq) - 1)
        with pytest.raises(_ffi.UnprovenInput) as ei:
            ctx.open_reads(comp, flags)
        assert "reads_open: text above INGEST_MAX_BYTES (%d)" % (len(fq) - 1) in str(ei.value)
        knobs.set("INGEST_MAX_BYTES", len(fq))
        ctx.open_reads(comp, flags).free()
    upload_still_works(ctx)


def test_not_accepted(ctx):
    from lrge_amd import _ffi
    for name, data, status, at, host in not_accepted_cases():
        with pytest.raises(_ffi.LrgeHipError) as ei:
            ctx.zstd_inflate(data)
        assert ei.value.code == _ffi.ERR_PARSE and "file offset" in str(ei.value), (name, str(ei.value))
        if at is not None:
            assert "file offset %d:" % at in str(ei.value), (name, at, str(ei.value))
        if name in ("wrong_checksum", "dictionary_id", "truncated_in_a_block"):
            with pytest.raises(_ffi.UnprovenInput) as ei:
                ctx.open_reads(data, inflate_flags())
            assert "reads_open: zstd data not accepted by the device (" in str(ei.value) and "near file offset" in str(ei.value), (name, str(ei.value))
        upload_still_works(ctx)


def test_checksum_option(ctx, knobs):
    from lrge_amd import _ffi
    _, comp, plain = Z.by_name("fastq_l3")
    flipped = comp[:-1] + bytes([comp[-1] ^ 1])
    with pytest.raises(_ffi.LrgeHipError):
        ctx.zstd_inflate(flipped)
    knobs.set("ZSTD_CHECKSUM", 0)
    out, st = ctx.zstd_inflate(flipped)
    assert out == plain and st["checksums_checked"] == 0 and st["checksum_us"] == 0
    knobs.set("ZSTD_CHECKSUM", 1)
    out, st = ctx.zstd_inflate(comp)
    assert out == plain and st["checksums_checked"] == 1


def test_records_fall_back_to_the_host(ctx, tmp_path):
    """lrge_hip_read_records_gpu_ex with the flag: the device's records on an accepted file, the host's records or message otherwise"""
    from lrge_amd import _ffi
    from test_gpu_gzip import read_gpu_ex
    comp, _ = three_frames()
    cases = {"ok": comp, "trailing": comp + b"junk", "truncated": comp[:len(comp) // 2], "wrong_checksum": comp[:-1] + bytes([comp[-1] ^ 1])}
    for name, data in cases.items():
        p = tmp_path / (name + ".fq.zst")
        p.write_bytes(data)
        rc_h, rec_h, msg_h = read_host(p)
        rc_g, rec_g, msg_g, used = read_gpu_ex(ctx, p, 1 | 2 | _ffi.GPU_INFLATE_ZSTD)
        assert rc_g == rc_h and used == (1 if name == "ok" else 0), (name, rc_g, rc_h, used)
        assert (rec_g == rec_h) if rc_h == 0 else (msg_g == msg_h), name
        rc_n, rec_n, _, used_n = read_gpu_ex(ctx, p, 3)                  # without the flag: the host decodes, as before
        assert rc_n == rc_h and used_n == 0 and (rc_h != 0 or rec_n == rec_h), name


def test_cli_gpu_zstd(tmp_path):
    from lrge_amd import build as B, readio
    tn, ts = readio.load(os.path.join(GOLDEN, "toy_reads.fa.gz"))
    p = tmp_path / "toy.fq.zst"
    p.write_bytes(Z.compress(W.fastq_bytes(tn, ts)))
    args = [B.CLI_PATH, str(p), "-T", "10", "-Q", "5", "--seed", "6", "-f"]
    a = subprocess.run(args, capture_output=True, text=True, timeout=120)
    b = subprocess.run(args + ["--gpu-ingest", "--gpu-zstd"], capture_output=True, text=True, timeout=120)
    c = subprocess.run(args + ["--gpu-zstd"], capture_output=True, text=True, timeout=120)
    d = subprocess.run(args + ["--gpu-ingest"], capture_output=True, text=True, timeout=120)
    assert a.returncode == 0 and b.returncode == 0 and c.returncode == 0 and d.returncode == 0, (a.stderr, b.stderr, c.stderr, d.stderr)
    assert a.stdout == b.stdout == c.stdout == d.stdout and a.stdout.strip()
    assert "gpu-ingest: device" in b.stderr and "gpu-ingest: host" in d.stderr      # --gpu-ingest alone: Zstandard stays with the host
