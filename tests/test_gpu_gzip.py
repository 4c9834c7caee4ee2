"""Plain and multi-member gzip decompressed on the device (k_gz_find / k_gz_decode / k_gz_window / k_gz_resolve): byte-equal
to zlib over the corpus of tests/gzip_corpus.py at default and tiny chunks and rounds, one single-member input above 1 GB,
the slot overflow retry and its TOO_MANY end, lrge_hip_read_records_gpu_ex against the host path, damaged files, the CLI."""
import ctypes as C
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_writer as W
import gzip_corpus as G

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_char), C.c_uint64, C.POINTER(C.c_char), C.c_uint64)


def test_corpus_default(ctx):
    for name, comp, plain in G.cases():
        assert ctx.gzip_inflate(comp) == plain, name


def test_corpus_tiny_chunks_and_rounds(ctx, knobs):
    knobs.set("GZIP_CHUNK_BYTES", 512)
    knobs.set("GZIP_ROUND_BYTES", 8192)
    knobs.set("GZIP_SLOT_RATIO", 64)
    tot = {"rejected_starts": 0, "speculative_starts": 0, "chunks": 0}
    for name, comp, plain in G.cases():
        out, st = ctx.gzip_inflate(comp, stats=True)
        assert out == plain, name
        for k in tot:
            tot[k] += st[k]
    assert tot["chunks"] > 1000 and tot["speculative_starts"] > 500 and tot["rejected_starts"] > 0, tot


def test_single_member_above_1gb(ctx):
    rng = np.random.default_rng(5)
    seqs = [rng.choice(np.frombuffer(b"ACGT", np.uint8), 1000).tobytes() for _ in range(4000)]
    fq = W.fastq_bytes([b"r%d" % i for i in range(len(seqs))], seqs)
    reps = (1100 << 20) // len(fq) + 1
    c = zlib.compressobj(1, zlib.DEFLATED, 31)
    parts = [c.compress(fq) for _ in range(reps)] + [c.flush()]
    comp = b"".join(parts)
    del parts
    out, st = ctx.gzip_inflate(comp, stats=True)
    assert len(out) == reps * len(fq) > 1 << 30 and st["members"] == 1
    mv = memoryview(out)
    for r in (0, 1, reps // 2, reps - 1):
        assert mv[r * len(fq):(r + 1) * len(fq)] == fq, r
    assert zlib.crc32(out) == zlib.crc32(fq * reps)


def test_overflow_retry_and_too_many(ctx, knobs):
    from lrge_amd import _ffi
    knobs.set("GZIP_CHUNK_BYTES", 65536)
    knobs.set("GZIP_SLOT_RATIO", 1)
    fq = G.fastq(300)
    out, st = ctx.gzip_inflate(G.gz(fq, 9), stats=True)
    assert out == fq and st["overflow_retries"] >= 1
    knobs.set("GZIP_CHUNK_BYTES", 512)
    with pytest.raises(_ffi.LrgeHipError) as ei:
        ctx.gzip_inflate(G.gz(b"A" * 400000, 9))
    assert ei.value.code == _ffi.ERR_TOO_MANY


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


def read_gpu_ex(ctx, path, flags):
    L = ctx._lib
    out = []
    cb = CB(lambda u, n, nl, b, bl: out.append((C.string_at(n, nl), C.string_at(b, bl))))
    used = C.c_int(-1)
    L.lrge_hip_read_records_gpu_ex.argtypes = [C.c_void_p, C.c_char_p, C.c_int, CB, C.c_void_p, C.POINTER(C.c_int)]
    rc = L.lrge_hip_read_records_gpu_ex(ctx.h, os.fsencode(str(path)), flags, cb, None, C.byref(used))
    msg = L.lrge_hip_last_error(ctx.h).decode() if rc else ""
    return rc, out, msg, used.value


def synth_reads():
    from lrge_amd import synth
    _, q, t = synth.make_config("tiny_twoset")
    return list(t.names) + list(q.names), t.seqs() + q.seqs()


def test_records_plain_and_concatenated(ctx, tmp_path):
    sn, ss = synth_reads()
    fq = W.fastq_bytes(sn, ss)
    files = {"plain.fq.gz": gzip.compress(fq),
             "concat.fq.gz": b"".join(gzip.compress(fq[i:i + 100000]) for i in range(0, len(fq), 100000)),
             "bgzf.fq.gz": W.bgzf_compress(fq)}
    for name, data in files.items():
        p = tmp_path / name
        p.write_bytes(data)
        rc_h, rec_h, _ = read_host(p)
        rc_g, rec_g, _, used = read_gpu_ex(ctx, p, 3)
        assert rc_h == 0 and rc_g == 0 and used == 1, name
        assert rec_g == rec_h and len(rec_h) == len(sn), name
        rc_b, rec_b, _, used_b = read_gpu_ex(ctx, p, 1)            # BGZF only: as lrge_hip_read_records_gpu
        assert rc_b == 0 and rec_b == rec_h and used_b == (1 if name == "bgzf.fq.gz" else 0), name


def test_damaged_files_host_message(ctx, tmp_path):
    from test_gzip_twin import damage_base, damage_cases
    base, plain = damage_base()
    assert ctx.gzip_inflate(base) == plain
    n = 0
    for kind, d in damage_cases(base, 300, 77):
        try:
            gzip.decompress(d)
            continue
        except Exception:
            pass
        p = tmp_path / ("bad%d.fq.gz" % n)
        p.write_bytes(d)
        rc_h, _, msg_h = read_host(p)
        rc_g, _, msg_g, used = read_gpu_ex(ctx, p, 3)
        if rc_h != 0:
            assert (rc_g, msg_g, used) == (rc_h, msg_h, 0)
            n += 1
        if n == 8:
            break
    assert n == 8


def test_cli_gpu_gzip(tmp_path):
    from lrge_amd import build as B, readio
    tn, ts = readio.load(os.path.join(GOLDEN, "toy_reads.fa.gz"))
    p = tmp_path / "toy.fq.gz"
    p.write_bytes(gzip.compress(W.fastq_bytes(tn, ts)))
    args = [B.CLI_PATH, str(p), "-T", "10", "-Q", "5", "--seed", "6", "-f"]
    a = subprocess.run(args, capture_output=True, text=True, timeout=120)
    b = subprocess.run(args + ["--gpu-gzip"], capture_output=True, text=True, timeout=120)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == b.stdout and a.stdout.strip()
