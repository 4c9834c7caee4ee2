"""Speculative gzip decoding without a GPU: the host twin (lrge_amd/csrc/gzip_twin.cpp, which runs gzip_round.h's rounds and
chain walk over the core of gzip_core.h sequentially) against zlib over levels, strategies, members, flushes, headers, BGZF
and chunk sizes; the finder's property; a seeded damage campaign; the kernels' resources from the compiler."""
import ctypes as C
import gzip
import os
import random
import re
import subprocess
import time
import zlib

import pytest

import gzip_corpus as G

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHUNKS = [512, 4096, 65536, 512 << 10]


@pytest.fixture(scope="module")
def gtwin():
    from lrge_amd import build as B
    L = C.CDLL(B.build_gzip_twin())
    L.gzip_twin_inflate.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.gzip_twin_result.argtypes = [C.c_void_p]
    L.gzip_twin_result.restype = C.c_uint64
    L.gzip_twin_find.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32]
    L.gzip_twin_find.restype = C.c_uint32
    L.gzip_twin_boundaries.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32]
    return L


def run(L, data, chunk=512 << 10, rnd=256 << 20, ratio=8):
    """(rc, bytes, stats): rc 0 decoded, -1 too many symbols for the slots, > 0 the status of the first bad chunk"""
    st = (C.c_uint64 * 7)()
    bad = C.c_uint64()
    rc = L.gzip_twin_inflate(data, len(data), chunk, rnd, ratio, st, C.byref(bad))
    n = L.gzip_twin_result(None)
    buf = C.create_string_buffer(max(1, n))
    L.gzip_twin_result(buf)
    keys = ("members", "chunks", "speculative", "rejected", "redecoded", "overflow_retries", "bytes_out")
    return rc, buf.raw[:n], dict(zip(keys, list(st)))


@pytest.mark.parametrize("chunk", CHUNKS)
def test_corpus_equals_zlib(gtwin, chunk):
    spec = 0
    for name, comp, plain in G.cases():
        assert gzip.decompress(comp) == plain, name
        rc, out, st = run(gtwin, comp, chunk, rnd=max(4 * chunk, 1 << 16), ratio=64)
        assert rc == 0, (name, chunk, rc, st)
        assert out == plain, (name, chunk)
        assert st["bytes_out"] == len(plain)
        spec += st["speculative"]
    if chunk <= 4096:
        assert spec > 100


def test_members_counted(gtwin):
    fq = G.fastq(400)
    parts = [fq[i:i + 3000] for i in range(0, len(fq), 3000)]
    rc, out, st = run(gtwin, b"".join(G.gz(p) for p in parts), 4096, 1 << 16)
    assert rc == 0 and out == fq and st["members"] == len(parts)


def test_fixed_only_stream_is_one_serial_chunk(gtwin):
    """Z_FIXED: no candidate anywhere after the header, so every chunk merges into the first (slow but exact)"""
    fq = G.fastq(600)
    comp = G.gz(fq, 6, zlib.Z_FIXED)
    rc, out, st = run(gtwin, comp, 512, 1 << 30, ratio=64)
    assert rc == 0 and out == fq
    assert st["speculative"] == 0 and st["chunks"] > 50


def test_rounds_and_rejected_starts(gtwin):
    fq = G.fastq(3000)
    comp = G.gz(fq, 6)
    rc, out, st = run(gtwin, comp, 512, 4096)
    assert rc == 0 and out == fq
    assert st["chunks"] > 50 and st["redecoded"] >= st["rejected"]


def test_overflow_retry_and_too_many(gtwin):
    run_bytes = b"A" * 400000
    comp = G.gz(run_bytes, 9)
    rc, out, st = run(gtwin, comp, 512, 1 << 20, ratio=1)
    assert rc == -1                                  # the run does not fit even in 4x of the smallest slot
    fq = G.fastq(300)
    rc, out, st = run(gtwin, G.gz(fq, 9), 65536, 1 << 20, ratio=1)
    assert rc == 0 and out == fq and st["overflow_retries"] >= 1


def test_finder_property(gtwin):
    """on each chunk the candidate is never past the first true dynamic / stored / member-header boundary at or after the
    chunk's start (the boundaries from a serial decode)"""
    fq = G.fastq(1500)
    files = [G.gz(fq, 6), G.gz(fq, 9, zlib.Z_FILTERED), G.gz_flushed(fq, zlib.Z_SYNC_FLUSH), G.gz_flushed(fq, zlib.Z_FULL_FLUSH, 5000, 1),
             b"".join(G.gz(fq[i:i + 20000]) for i in range(0, len(fq), 20000)), G.gz(fq, 0)]
    checked = 0
    for f in files:
        bits = (C.c_uint32 * 100000)()
        kind = (C.c_uint32 * 100000)()
        nb = gtwin.gzip_twin_boundaries(f, len(f), bits, kind, 100000)
        assert nb > 0
        targets = sorted(bits[i] for i in range(nb) if kind[i] in (1, 2, 3))
        for chunk in (512, 4096):
            for c0 in range(chunk, len(f), chunk):
                nxt = [b for b in targets if b >= 8 * c0]
                if not nxt:
                    continue
                cand = gtwin.gzip_twin_find(f, len(f), 8 * c0, 8 * len(f))
                assert cand != 0xFFFFFFFF and cand <= nxt[0], (chunk, c0, cand, nxt[0])
                checked += 1
    assert checked > 100


def damage_cases(base, n, seed):
    rng = random.Random(seed)
    for i in range(n):
        b = bytearray(base)
        kind = i % 3
        if kind == 0:
            for _ in range(rng.randint(1, 3)):
                pos = rng.randrange(len(b))
                b[pos] ^= 1 << rng.randrange(8)
        elif kind == 1:
            pos = rng.randrange(len(b) - 1)
            v = rng.choice([0, 1, 0xFFFF, rng.randrange(65536), (b[pos] | b[pos + 1] << 8) ^ (1 << rng.randrange(16))])
            b[pos], b[pos + 1] = v & 0xFF, v >> 8
        else:
            b = b[:rng.randrange(len(b))]
        yield kind, bytes(b)


def damage_base():
    fq = G.fastq(120, seed=11)
    return (G.gz(fq[:6000], 6) + G.gz_flushed(fq[6000:14000], zlib.Z_SYNC_FLUSH, 2000) + G.gz(fq[14000:18000], 1, zlib.Z_FIXED) +
            G.gz_header(fq[18000:], fname=b"n", fhcrc=True, level=9)), fq


def zlib_multi(d):
    try:
        return gzip.decompress(d)
    except Exception:
        return None


def test_damage_campaign(gtwin):
    base, plain = damage_base()
    assert run(gtwin, base, 512, 4096)[:2] == (0, plain)
    outcome = {"error": 0, "exact": 0}
    for kind, d in damage_cases(base, 1500, 2026):
        t0 = time.perf_counter()
        rc, out, _ = run(gtwin, d, 512, 4096)
        assert time.perf_counter() - t0 < 2.0
        if rc == 0:
            assert out == zlib_multi(d), "damaged input decoded to different bytes without an error"
            outcome["exact"] += 1
        else:
            outcome["error"] += 1
    assert outcome["error"] > 1000


def test_trailing_bytes_refused(gtwin):
    fq = G.fastq(100)
    comp = G.gz(fq)
    assert run(gtwin, comp)[0] == 0
    assert run(gtwin, comp + b"\0")[0] > 0
    assert run(gtwin, comp + b"garbage!" * 3)[0] > 0
    assert run(gtwin, comp[:-1])[0] > 0
    assert run(gtwin, b"")[0] > 0


def test_k_gzip_resources(tmp_path):
    src = tmp_path / "k.hip"
    src.write_text('#include "%s"\n' % os.path.join(ROOT, "lrge_amd", "csrc", "k_gzip.h"))
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-o", str(tmp_path / "k.o"), str(src),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    txt = r.stderr
    for k in ("k_gz_find", "k_gz_decode", "k_gz_window", "k_gz_resolve"):
        i = txt.index("Function Name: _Z%d%s" % (len(k), k))
        block = txt[i:i + 2000]
        val = lambda key: int(re.search(key + r": (\d+)", block).group(1))   # noqa: E731
        assert val(r"ScratchSize \[bytes/lane\]") == 0, k
        assert val("VGPRs Spill") == 0, k
        lds = val(r"LDS Size \[bytes/block\]")
        assert lds <= 160 * 1024 // 2, (k, lds)
        if k == "k_gz_decode":
            assert lds > 65536, lds                  # the 32 Ki-symbol u16 ring in LDS; two workgroups per CU
