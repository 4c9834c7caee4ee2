"""BGZF decoding without a GPU: the block scan of liblrge_hip.so (lrge_hip_bgzf_scan), the host twin of k_inflate
(lrge_amd/csrc/inflate_twin.cpp: the kernel's bit-level core built with g++) against zlib, a seeded damage campaign on the
twin, and the kernel's resources from the compiler (no scratch; the LDS budget that gives two workgroups per CU)."""
import ctypes as C
import gzip
import os
import random
import re
import subprocess
import time
import zlib

import numpy as np
import pytest

import bgzf_writer as W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STRATEGIES = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED]


@pytest.fixture(scope="module")
def twin():
    from lrge_amd import build as B
    L = C.CDLL(B.build_twin())
    L.inflate_twin_raw.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.inflate_twin_crc.argtypes = [C.c_char_p, C.c_uint32]
    L.inflate_twin_crc.restype = C.c_uint32
    L.inflate_twin_scan.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.inflate_twin_bgzf.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    return L


def twin_bgzf(L, data, cap=None):
    """(status, bytes, bad block offset): status 0 = decoded, -2 = not BGZF, > 0 = the first bad block's INF_E_* code."""
    n, total = C.c_uint64(), C.c_uint64()
    if L.inflate_twin_scan(data, len(data), C.byref(n), C.byref(total)) != 0:
        return -2, None, None
    out = C.create_string_buffer(max(1, total.value))
    bad = C.c_uint64()
    rc = L.inflate_twin_bgzf(data, len(data), out, total.value, C.byref(bad))
    return rc, out.raw[:total.value], bad.value


def scan(data):
    from lrge_amd import _ffi
    n, total = C.c_uint64(), C.c_uint64()
    rc = _ffi.lib().lrge_hip_bgzf_scan(data, len(data), C.byref(n), C.byref(total))
    return rc, n.value, total.value


def payloads():
    """The corpus: FASTQ text, BAM records, random bytes (stored blocks), one long single-byte run (length 258, distance 1),
    a pattern of period 32 768 (the largest distance), short-period overlapping copies."""
    rng = random.Random(7)
    nrng = np.random.default_rng(7)
    names = [b"read%05d" % i for i in range(400)]
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(50, 400))) for _ in range(400)]
    half = nrng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    return {
        "fastq": W.fastq_bytes(names, seqs)[:65536],
        "bam": W.bam_bytes(names, seqs)[:65536],
        "random": nrng.integers(0, 256, W.DEFAULT_BLOCK, dtype=np.uint8).tobytes(),
        "run": b"A" * 65536,
        "period32k": half + half,
        "short_period": b"".join(bytes(rng.choice(b"ACGT") for _ in range(p)) * (65536 // p // 8) for p in (1, 2, 3, 5, 7, 13, 64, 100))[:65536],
    }


def corpus():
    """(name, data, level, strategy, memlevel) for every combination; sizes 0, 1, 65 280 and 65 536 included."""
    out = []
    for name, d in payloads().items():
        for level in (0, 1, 6, 9):
            for st in STRATEGIES:
                for mem in (1, 9):
                    out.append((name, d, level, st, mem))
    for size in (0, 1, 65280, 65536):
        for level in (0, 1, 9):
            d = payloads()["fastq"][:size]
            if level == 0 and size == 65536:
                continue              # a stored 64 KiB block does not fit in one BGZF member
            out.append(("size%d" % size, d, level, zlib.Z_DEFAULT_STRATEGY, 8))
    return out


def fits(d, level, st, mem):
    return len(W.deflate_raw(d, level, st, mem)) + 26 <= 65536


# ---- scan ----
def test_scan_accepts_bgzf_with_other_subfields_and_fname():
    data = b"hello BGZF " * 1000
    blocks = [W.bgzf_block(data[:5000]),
              W.bgzf_block(data[5000:9000], extra_before=b"XY\x03\x00abc", fname=b"reads.fq"),
              W.bgzf_block(data[9000:], extra_after=b"ZZ\x00\x00", comment=b"a comment", fhcrc=True),
              W.EOF_BLOCK]
    buf = b"".join(blocks)
    assert scan(buf) == (0, 4, len(data))


def test_scan_rejects_non_bgzf(tmp_path):
    from conftest import write_unaligned_bam
    data = b"ACGT" * 30000
    good = W.bgzf_compress(data)
    assert scan(good)[0] == 0
    assert scan(gzip.compress(data))[0] != 0                        # plain gzip: no BC
    p = tmp_path / "conftest_style.bam"
    write_unaligned_bam(str(p), [b"r1", b"r2"], [b"ACGT" * 100, b"TTGCA" * 50])
    assert scan(p.read_bytes())[0] != 0                             # multi-member gzip without BC
    assert scan(good[:-1])[0] != 0                                  # truncated
    assert scan(good[:len(good) - len(W.EOF_BLOCK) - 3])[0] != 0     # truncated inside a block
    assert scan(good + b"\0")[0] != 0                               # trailing bytes
    assert scan(good + b"\x1f\x8b")[0] != 0
    assert scan(b"")[0] != 0
    bad_hcrc = bytearray(W.bgzf_block(data[:100], fhcrc=True))
    bad_hcrc[18] ^= 1                                              # the header CRC (zlib checks it too)
    assert scan(bytes(bad_hcrc))[0] != 0


# ---- host twin against zlib ----
def test_twin_crc_stripes_match_zlib(twin):
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 63, 64, 65, 1000, 65280, 65536):
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert twin.inflate_twin_crc(d, n) == zlib.crc32(d), n


def test_twin_corpus_equals_zlib(twin):
    n = 0
    for name, d, level, st, mem in corpus():
        comp = W.deflate_raw(d, level, st, mem)
        out = C.create_string_buffer(max(1, len(d)))
        rc = twin.inflate_twin_raw(comp, len(comp), out, len(d))
        assert rc == 0, (name, level, st, mem, rc)
        assert out.raw[:len(d)] == zlib.decompress(comp, -15) == d, (name, level, st, mem)
        if fits(d, level, st, mem):
            f = W.bgzf_block(d, level, st, mem) + W.EOF_BLOCK
            rc, got, _ = twin_bgzf(twin, f)
            assert rc == 0 and got == d, (name, level, st, mem, rc)
            n += 1
    assert n > 150           # (stored 64 KiB blocks do not fit in a BGZF member)


def damage_base():
    rng = random.Random(11)
    names = [b"r%d" % i for i in range(60)]
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(20, 120))) for _ in range(60)]
    fq = W.fastq_bytes(names, seqs)
    parts = [(fq[:3000], 6, zlib.Z_DEFAULT_STRATEGY), (fq[3000:5000], 1, zlib.Z_FIXED), (fq[5000:6000], 0, zlib.Z_DEFAULT_STRATEGY),
             (b"A" * 2000 + fq[6000:8000], 9, zlib.Z_RLE), (fq[8000:9000], 6, zlib.Z_HUFFMAN_ONLY)]
    return b"".join([W.bgzf_block(d, lv, st) for d, lv, st in parts] + [W.EOF_BLOCK]), b"".join(d for d, _, _ in parts)


def damage_cases(base, n, seed):
    """Seeded damage: bit flips, overwritten length fields, truncations."""
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


def test_twin_damage_campaign(twin):
    base, plain = damage_base()
    assert twin_bgzf(twin, base)[:2] == (0, plain)
    outcome = {"error": 0, "exact": 0}
    for kind, d in damage_cases(base, 2400, 2026):
        t0 = time.perf_counter()
        rc, got, _ = twin_bgzf(twin, d)
        assert time.perf_counter() - t0 < 1.0
        if rc == 0:
            # the original bytes, or -- a file cut exactly between two blocks is still valid BGZF -- the bytes of the
            # blocks that are left; zlib says the same
            assert got == gzip.decompress(d), "damaged input decoded to different bytes without an error"
            assert got == plain or (kind == 2 and plain.startswith(got))
            outcome["exact"] += 1
        else:
            outcome["error"] += 1
    assert outcome["error"] > 1500


def pack_bits(bits):
    """deflate's bit order: the first bit of the stream is bit 0 of the first byte"""
    return bytes(sum(bit << k for k, bit in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8))


def test_twin_rejects_each_error_class(twin):
    """Hand-made raw deflate streams, one per status of inflate_core.h."""
    out = C.create_string_buffer(64)
    assert twin.inflate_twin_raw(b"\x07", 1, out, 0) == 1                      # BTYPE 3
    assert twin.inflate_twin_raw(b"\x01\x02\x00\x00\x00", 5, out, 2) == 2      # LEN != ~NLEN
    assert twin.inflate_twin_raw(b"\x01\x05\x00\xfa\xffab", 7, out, 5) == 6    # stored block longer than the input
    lit = W.deflate_raw(b"abc", 6, zlib.Z_FIXED)
    assert twin.inflate_twin_raw(lit, len(lit), out, 2) == 7                   # more output than ISIZE
    assert twin.inflate_twin_raw(lit, len(lit), out, 4) == 8                   # less
    assert twin.inflate_twin_raw(lit + b"\0", len(lit) + 1, out, 3) == 6       # data after the final block
    assert twin.inflate_twin_raw(lit[:-1], len(lit) - 1, out, 3) == 6          # truncated
    # fixed block: literal 'a', then length 3 distance 2 (before the block start)
    bits = [1, 1, 0] + [int(c) for c in format(0x30 + ord("a"), "08b")] + [0, 0, 0, 0, 0, 0, 1] + [0, 0, 0, 0, 1] + [0] * 7
    raw = pack_bits(bits)
    assert twin.inflate_twin_raw(raw, len(raw), out, 4) == 5
    # dynamic block whose code-length code is over-subscribed: HCLEN = 4 codes of length 1
    bits = [1, 0, 1] + [0] * 5 + [0] * 5 + [0] * 4 + [1, 0, 0] * 4
    raw = pack_bits(bits)
    assert twin.inflate_twin_raw(raw, len(raw), out, 1) == 3


# ---- kernel resources ----
def test_k_inflate_resources(tmp_path):
    src = tmp_path / "k.hip"
    src.write_text('#include "%s"\n' % os.path.join(ROOT, "lrge_amd", "csrc", "k_inflate.h"))
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-o", str(tmp_path / "k.o"), str(src),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    txt = r.stderr
    i = txt.index("Function Name: _Z9k_inflate")
    block = txt[i:i + 2000]
    val = lambda key: int(re.search(key + r": (\d+)", block).group(1))
    assert val(r"ScratchSize \[bytes/lane\]") == 0
    assert val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0
    lds = val(r"LDS Size \[bytes/block\]")
    assert 65536 < lds <= 160 * 1024 // 2, lds          # the whole block's output in LDS; two workgroups per CU
