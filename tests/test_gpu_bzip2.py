"""bzip2 decompressed on the device (k_bz_find / k_bz_decode / k_bz_scatter / k_bz_walk / k_bz_rle_count / k_bz_rle_write):
byte-equal to libbz2 over the corpus of tests/bzip2_corpus.py and the streams of tests/bzip2_writer.py, the stats of the host
twin field for field at the default round and at rounds of two candidates, read sets opened from bzip2 text kept in HBM
against the host reader, what is not accepted, the CLI."""
import bz2
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bgzf_writer as W
import bzip2_corpus as Z
import bzip2_writer as ZW
from test_bzip2_twin import STAT_KEYS, flip_stream_crc, load_twin, not_accepted_cases, run as run_twin
from test_gpu_ingest import check_seqset, read_host

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def btwin():
    from lrge_amd import build as B
    return load_twin(B.build_bzip2_twin())


def test_corpus_and_writer_streams_equal_libbz2(ctx):
    for name, comp, plain in Z.cases() + ZW.cases():
        out, st = ctx.bzip2_inflate(comp)
        assert out == plain == bz2.decompress(comp), name
        assert st["bytes_out"] == len(plain), (name, st)


@pytest.mark.parametrize("round_blocks", [0, 2])
def test_stats_equal_the_twin(ctx, knobs, btwin, round_blocks):
    if round_blocks:
        knobs.set("BZIP2_ROUND_BLOCKS", round_blocks)
    for name, comp, plain in Z.cases() + ZW.cases():
        out, st = ctx.bzip2_inflate(comp)
        rc, out_t, st_t, _ = run_twin(btwin, comp, round_blocks)
        assert rc == 0 and out == out_t == plain, name
        assert [st[k] for k in STAT_KEYS] == [st_t[k] for k in STAT_KEYS], (name, st, st_t)
    _, comp, _ = Z.three_blocks()
    _, st = ctx.bzip2_inflate(comp)
    assert st["blocks"] == 3 and st["rounds"] == (2 if round_blocks else 1), st


def test_open_reads_from_bzip2(ctx, tmp_path, knobs):
    from lrge_amd import _ffi
    _, comp, plain = Z.three_blocks()
    p = tmp_path / "three.fq.bz2"
    p.write_bytes(comp)
    rc_h, rec_h, msg = read_host(p)
    assert rc_h == 0 and len(rec_h) > 100, msg
    flags = _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INFLATE_BZIP2
    seqs = [s for _, s in rec_h]
    for round_blocks in (0, 2):                         # one round, and text appended behind an earlier round's
        if round_blocks:
            knobs.set("BZIP2_ROUND_BLOCKS", round_blocks)
        for src in (comp, str(p)):
            dr = ctx.open_reads(src, flags)
            assert dr.n == len(rec_h) and dr.text_bytes == len(plain)
            assert dr.names == [n for n, _ in rec_h]
            assert np.array_equal(dr.lens, np.array([len(s) for s in seqs], dtype=np.uint32))
            check_seqset(ctx, dr, seqs, list(range(dr.n)), ("three_blocks", round_blocks))
            dr.free()
    with pytest.raises(_ffi.UnprovenInput):             # without the flag: as before
        ctx.open_reads(comp)
    with pytest.raises(_ffi.UnprovenInput):
        ctx.open_reads(comp, _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INGEST_BAM | _ffi.GPU_INGEST_SAM)


def test_not_accepted(ctx, btwin):
    from lrge_amd import _ffi
    _, comp, _ = Z.three_blocks()
    flags = _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INFLATE_BZIP2
    for name, data, status, _ in not_accepted_cases():
        if name == "stream_crc":
            data = flip_stream_crc(btwin, comp)
        with pytest.raises(_ffi.LrgeHipError) as ei:
            ctx.bzip2_inflate(data)
        assert ei.value.code == _ffi.ERR_PARSE and "file offset" in str(ei.value), (name, str(ei.value))
        if name in ("two_streams", "block_crc", "randomised"):
            with pytest.raises(_ffi.UnprovenInput):
                ctx.open_reads(data, flags)


def test_records_fall_back_to_the_host(ctx, tmp_path):
    """lrge_hip_read_records_gpu_ex with the flag: the device's records on an accepted file, the host's records or message otherwise"""
    from lrge_amd import _ffi
    from test_gpu_gzip import read_gpu_ex
    _, comp, _ = Z.three_blocks()
    cases = {"ok": comp, "two_streams": comp + bz2.compress(b"@x\nA\n+\nI\n"), "truncated": comp[:len(comp) // 2]}
    for name, data in cases.items():
        p = tmp_path / (name + ".fq.bz2")
        p.write_bytes(data)
        rc_h, rec_h, msg_h = read_host(p)
        rc_g, rec_g, msg_g, used = read_gpu_ex(ctx, p, 1 | 2 | _ffi.GPU_INFLATE_BZIP2)
        assert rc_g == rc_h and used == (1 if name == "ok" else 0), (name, rc_g, rc_h, used)
        assert (rec_g == rec_h) if rc_h == 0 else (msg_g == msg_h), name
        rc_n, rec_n, _, used_n = read_gpu_ex(ctx, p, 3)                  # without the flag: the host decodes, as before
        assert rc_n == rc_h and used_n == 0 and (rc_h != 0 or rec_n == rec_h), name


def test_cli_gpu_bzip2(tmp_path):
    from lrge_amd import build as B, readio
    tn, ts = readio.load(os.path.join(GOLDEN, "toy_reads.fa.gz"))
    p = tmp_path / "toy.fq.bz2"
    p.write_bytes(bz2.compress(W.fastq_bytes(tn, ts)))
    args = [B.CLI_PATH, str(p), "-T", "10", "-Q", "5", "--seed", "6", "-f"]
    a = subprocess.run(args, capture_output=True, text=True, timeout=120)
    b = subprocess.run(args + ["--gpu-ingest", "--gpu-bzip2"], capture_output=True, text=True, timeout=120)
    c = subprocess.run(args + ["--gpu-bzip2"], capture_output=True, text=True, timeout=120)
    d = subprocess.run(args + ["--gpu-ingest"], capture_output=True, text=True, timeout=120)
    assert a.returncode == 0 and b.returncode == 0 and c.returncode == 0 and d.returncode == 0, (a.stderr, b.stderr, c.stderr, d.stderr)
    assert a.stdout == b.stdout == c.stdout == d.stdout and a.stdout.strip()
    assert "gpu-ingest: device" in b.stderr and "gpu-ingest: host" in d.stderr      # --gpu-ingest alone: bzip2 stays with the host
