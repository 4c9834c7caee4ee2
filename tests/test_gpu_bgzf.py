"""BGZF decompressed on the device (k_inflate): byte-equal to zlib over the corpus of tests/test_bgzf_twin.py, with many
chunks and on an input of more than 1 GB; lrge_hip_read_records_gpu against lrge_hip_read_records on BGZF and non-BGZF
input; damaged blocks (already proven on the host twin) refused with the block's file offset; the CLI's --gpu-inflate."""
import bz2
import ctypes as C
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_writer as W
from test_bgzf_twin import corpus, damage_base, damage_cases, fits, twin, twin_bgzf  # noqa: F401  (twin: fixture)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_char), C.c_uint64, C.POINTER(C.c_char), C.c_uint64)


def corpus_file():
    blocks, plain = [], []
    for name, d, level, st, mem in corpus():
        if fits(d, level, st, mem):
            blocks.append(W.bgzf_block(d, level, st, mem))
            plain.append(d)
    return b"".join(blocks) + W.EOF_BLOCK, b"".join(plain)


def test_corpus_equals_zlib(ctx):
    f, plain = corpus_file()
    assert ctx.bgzf_inflate(f) == plain == gzip.decompress(f)


def test_corpus_many_chunks(ctx, knobs):
    f, plain = corpus_file()
    knobs.set("INFLATE_CHUNK_BYTES", 300000)          # a few blocks per chunk
    assert ctx.bgzf_inflate(f) == plain
    knobs.set("INFLATE_CHUNK_BYTES", 1)               # one block per chunk
    assert ctx.bgzf_inflate(f) == plain


def test_more_than_1gb(ctx):
    """16 MiB of FASTQ in BGZF blocks, the block sequence repeated 72 times (blocks are independent): 1.2 GB out."""
    rng = np.random.default_rng(5)
    seqs = [rng.choice(np.frombuffer(b"ACGT", np.uint8), 1000).tobytes() for _ in range(8000)]
    fq = W.fastq_bytes([b"r%d" % i for i in range(len(seqs))], seqs)[:16 << 20]
    one = W.bgzf_compress(fq, eof=False, level=1)
    reps = 72
    out = ctx.bgzf_inflate(one * reps + W.EOF_BLOCK)
    assert len(out) == reps * len(fq) > 1 << 30
    mv = memoryview(out)
    for r in range(reps):
        assert mv[r * len(fq):(r + 1) * len(fq)] == fq, r


# ---- records ----
def read_host(path):
    from lrge_amd import _ffi
    L = _ffi.lib()
    out = []
    cb = CB(lambda u, n, nl, b, bl: out.append((C.string_at(n, nl), C.string_at(b, bl))))
    err = C.create_string_buffer(512)
    L.lrge_hip_read_records.argtypes = [C.c_char_p, CB, C.c_void_p, C.c_char_p, C.c_uint64]
    rc = L.lrge_hip_read_records(os.fsencode(str(path)), cb, None, err, 512)
    return rc, out, err.value.decode()


def read_gpu(ctx, path):
    L = ctx._lib
    out = []
    cb = CB(lambda u, n, nl, b, bl: out.append((C.string_at(n, nl), C.string_at(b, bl))))
    used = C.c_int(-1)
    L.lrge_hip_read_records_gpu.argtypes = [C.c_void_p, C.c_char_p, CB, C.c_void_p, C.POINTER(C.c_int)]
    rc = L.lrge_hip_read_records_gpu(ctx.h, os.fsencode(str(path)), cb, None, C.byref(used))
    msg = L.lrge_hip_last_error(ctx.h).decode() if rc else ""
    return rc, out, msg, used.value


def toy_reads():
    from lrge_amd import readio
    return readio.load(os.path.join(GOLDEN, "toy_reads.fa.gz"))


def synth_reads():
    from lrge_amd import synth
    _, q, t = synth.make_config("tiny_twoset")
    return list(t.names) + list(q.names), t.seqs() + q.seqs()


def test_records_bgzf_device(ctx, tmp_path):
    tn, ts = toy_reads()
    sn, ss = synth_reads()
    files = {"toy.bam": W.bgzf_compress(W.bam_bytes(tn, ts)),
             "synth.bam": W.bgzf_compress(W.bam_bytes(sn, ss), level=9),
             "synth.fq.gz": W.bgzf_compress(W.fastq_bytes(sn, ss), level=1),
             "synth.fa.gz": W.bgzf_compress(W.fasta_bytes(sn, ss), fname=b"synth.fa")}
    for name, data in files.items():
        p = tmp_path / name
        p.write_bytes(data)
        rc_h, rec_h, _ = read_host(p)
        rc_g, rec_g, _, used = read_gpu(ctx, p)
        assert rc_h == 0 and rc_g == 0 and used == 1, name
        assert rec_g == rec_h and len(rec_h) > 10, name


def test_records_other_input_host_path(ctx, tmp_path):
    from conftest import write_unaligned_bam
    sn, ss = synth_reads()
    fq = W.fastq_bytes(sn, ss)
    (tmp_path / "plain.fq.gz").write_bytes(gzip.compress(fq))
    write_unaligned_bam(str(tmp_path / "conftest.bam"), sn, ss)
    (tmp_path / "reads.fq.bz2").write_bytes(bz2.compress(fq))
    (tmp_path / "reads.fq").write_bytes(fq)
    for name in ("plain.fq.gz", "conftest.bam", "reads.fq.bz2", "reads.fq"):
        rc_h, rec_h, _ = read_host(tmp_path / name)
        rc_g, rec_g, _, used = read_gpu(ctx, tmp_path / name)
        assert rc_h == 0 and rc_g == 0 and used == 0, name
        assert rec_g == rec_h and len(rec_h) == len(sn), name


def test_damaged_blocks(ctx, twin, tmp_path):   # noqa: F811
    from lrge_amd import _ffi
    base, plain = damage_base()
    assert ctx.bgzf_inflate(base) == plain
    picked = []
    for kind, d in damage_cases(base, 600, 99):
        rc, _, off = twin_bgzf(twin, d)
        if rc > 0 and kind != 2:
            picked.append((d, off))
        if len(picked) == 6:
            break
    assert len(picked) == 6
    for i, (d, off) in enumerate(picked):
        with pytest.raises(_ffi.LrgeHipError) as ei:
            ctx.bgzf_inflate(d)
        assert ei.value.code == _ffi.ERR_PARSE and ("file offset %d:" % off) in str(ei.value)
        p = tmp_path / ("bad%d.fq.gz" % i)
        p.write_bytes(d)
        rc_h, _, msg_h = read_host(p)
        rc_g, _, msg_g, used = read_gpu(ctx, p)
        assert rc_h != 0 and (rc_g, msg_g, used) == (rc_h, msg_h, 0)


def test_cli_gpu_inflate(tmp_path):
    from lrge_amd import build as B
    tn, ts = toy_reads()
    bam = tmp_path / "toy.bam"
    bam.write_bytes(W.bgzf_compress(W.bam_bytes(tn, ts)))
    args = [B.CLI_PATH, str(bam), "-T", "10", "-Q", "5", "--seed", "6", "-f"]
    a = subprocess.run(args, capture_output=True, text=True, timeout=120)
    b = subprocess.run(args + ["--gpu-inflate"], capture_output=True, text=True, timeout=120)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == b.stdout and a.stdout.strip()
