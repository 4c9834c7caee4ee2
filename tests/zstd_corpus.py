"""Zstandard inputs for the block-parallel decode tests, made with the system's libzstd (ctypes: ZSTD_compress2 with the level,
the window log, the checksum and the content-size flag set per case), and a small walker over frames and blocks that names which
block types, literals types and sequence modes a stream uses.  The corpus asserts its own shapes with the walker, so a name
cannot drift from what the stream holds."""
import ctypes as C
import random
import struct

from bzip2_corpus import fastq, noise

MAGIC = b"\x28\xb5\x2f\xfd"
C_LEVEL, C_WINDOW_LOG, C_CONTENT_SIZE, C_CHECKSUM = 100, 101, 200, 201      # ZSTD_cParameter
_Z = None


def lib():
    global _Z
    if _Z is None:
        z = C.CDLL("libzstd.so.1")
        z.ZSTD_createCCtx.restype = C.c_void_p
        z.ZSTD_freeCCtx.argtypes = [C.c_void_p]
        z.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
        z.ZSTD_CCtx_setParameter.restype = C.c_size_t
        z.ZSTD_compress2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
        z.ZSTD_compress2.restype = C.c_size_t
        z.ZSTD_compressBound.argtypes = [C.c_size_t]
        z.ZSTD_compressBound.restype = C.c_size_t
        z.ZSTD_isError.argtypes = [C.c_size_t]
        z.ZSTD_createDStream.restype = C.c_void_p
        z.ZSTD_freeDStream.argtypes = [C.c_void_p]
        z.ZSTD_initDStream.argtypes = [C.c_void_p]
        z.ZSTD_initDStream.restype = C.c_size_t
        z.ZSTD_decompressStream.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        z.ZSTD_decompressStream.restype = C.c_size_t
        _Z = z
    return _Z


def compress(data, level=3, window_log=0, checksum=True, content_size=True):
    """one frame"""
    z = lib()
    cctx = z.ZSTD_createCCtx()
    try:
        for k, v in ((C_LEVEL, level), (C_WINDOW_LOG, window_log), (C_CHECKSUM, int(checksum)), (C_CONTENT_SIZE, int(content_size))):
            assert not z.ZSTD_isError(z.ZSTD_CCtx_setParameter(cctx, k, v)), (k, v)
        cap = z.ZSTD_compressBound(len(data))
        buf = C.create_string_buffer(cap)
        n = z.ZSTD_compress2(cctx, buf, cap, data, len(data))
        assert not z.ZSTD_isError(n)
        return buf.raw[:n]
    finally:
        z.ZSTD_freeCCtx(cctx)


class _Buf(C.Structure):
    _fields_ = [("p", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]


def decompress(data):
    """what the host readers' loop over ZSTD_decompressStream gives for the whole of `data` (every frame, skippable frames
    skipped), or None where it reports an error or the data ends inside a frame"""
    z = lib()
    ds = z.ZSTD_createDStream()
    try:
        if z.ZSTD_isError(z.ZSTD_initDStream(ds)):
            return None
        src = C.create_string_buffer(data, max(1, len(data)))
        ib = _Buf(C.cast(src, C.c_void_p), len(data), 0)
        cap = 1 << 17
        dst = C.create_string_buffer(cap)
        out, last = [], 0
        while ib.pos < ib.size:
            ob = _Buf(C.cast(dst, C.c_void_p), cap, 0)
            last = z.ZSTD_decompressStream(ds, C.byref(ob), C.byref(ib))
            if z.ZSTD_isError(last):
                return None
            out.append(dst.raw[:ob.pos])
            while ob.pos == cap:                            # the decoder holds more than the buffer took
                ob = _Buf(C.cast(dst, C.c_void_p), cap, 0)
                last = z.ZSTD_decompressStream(ds, C.byref(ob), C.byref(ib))
                if z.ZSTD_isError(last):
                    return None
                out.append(dst.raw[:ob.pos])
        return b"".join(out) if last == 0 else None
    finally:
        z.ZSTD_freeDStream(ds)


def skippable(payload=b"lrge", nibble=0):
    return struct.pack("<II", 0x184D2A50 | nibble, len(payload)) + payload


# ---- the walker ----
BLOCK_NAMES = ("raw", "rle", "compressed")
LIT_NAMES = ("raw", "rle", "huffman", "treeless")
MODE_NAMES = ("predefined", "rle", "fse", "repeat")


def walk(data):
    """{frames, skippable_frames, blocks, raw_blocks, rle_blocks, sequences, checksums, per_frame: [blocks], lit: set of
    (type, streams), weights: set of "direct" / "fse", modes: set of (table, mode), nseq: [per compressed block]}"""
    st = dict(frames=0, skippable_frames=0, blocks=0, raw_blocks=0, rle_blocks=0, sequences=0, checksums=0, per_frame=[], lit=set(), weights=set(), modes=set(),
              nseq=[], types=[])
    p = 0
    while p < len(data):
        magic, = struct.unpack_from("<I", data, p)
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            p += 8 + struct.unpack_from("<I", data, p + 4)[0]
            st["skippable_frames"] += 1
            continue
        assert magic == 0xFD2FB528, hex(magic)
        fhd = data[p + 4]
        single, did = (fhd >> 5) & 1, fhd & 3
        p += 5 + (0 if single else 1) + (4 if did == 3 else did)
        fcs = fhd >> 6
        p += (1 if single else 0) if fcs == 0 else 1 << fcs
        st["frames"] += 1
        st["per_frame"].append(0)
        while True:
            bh = data[p] | data[p + 1] << 8 | data[p + 2] << 16
            p += 3
            last, typ, size = bh & 1, (bh >> 1) & 3, bh >> 3
            st["blocks"] += 1
            st["per_frame"][-1] += 1
            st["types"].append(BLOCK_NAMES[typ])
            st["raw_blocks"] += typ == 0
            st["rle_blocks"] += typ == 1
            if typ == 2:
                _walk_block(data[p:p + size], st)
            p += 1 if typ == 1 else size
            if last:
                break
        if fhd & 4:
            p += 4
            st["checksums"] += 1
    return st


def _walk_block(b, st):
    typ, sf = b[0] & 3, (b[0] >> 2) & 3
    if typ < 2:
        hdr = {0: 1, 2: 1, 1: 2, 3: 3}[sf]
        regen = b[0] >> 3 if hdr == 1 else (int.from_bytes(b[:hdr], "little") >> 4)
        size, streams = (regen if typ == 0 else 1), 1
    else:
        hdr = {0: 3, 1: 3, 2: 4, 3: 5}[sf]
        bits = {3: 10, 4: 14, 5: 18}[hdr]
        v = int.from_bytes(b[:hdr], "little") >> 4
        size, streams = v >> bits, (1 if sf == 0 else 4)
        if typ == 2:
            st["weights"].add("direct" if b[hdr] >= 128 else "fse")
    st["lit"].add((LIT_NAMES[typ], streams))
    at = hdr + size
    n = b[at]
    at += 1
    if n == 255:
        n = b[at] + (b[at + 1] << 8) + 0x7F00
        at += 2
    elif n >= 128:
        n = ((n - 128) << 8) + b[at]
        at += 1
    st["nseq"].append(n)
    st["sequences"] += n
    if n:
        m = b[at]
        for name, shift in (("ll", 6), ("of", 4), ("ml", 2)):
            st["modes"].add((name, MODE_NAMES[(m >> shift) & 3]))


def stats_of(data):
    """the stats a decoder of `data` must report, but for rounds and checksums_checked"""
    w = walk(data)
    return {k: w[k] for k in ("frames", "skippable_frames", "blocks", "raw_blocks", "rle_blocks", "sequences")}


# ---- the corpus ----
_CASES = None


def chain_text():
    return fastq(150_000, 31) * 4


def cases():
    """(name, zstd bytes, plain bytes); computed once"""
    global _CASES
    if _CASES is not None:
        return _CASES
    fq = fastq(400_000, 21)
    rng = random.Random(5)
    rnd = bytes(rng.getrandbits(8) for _ in range(200_000))
    out = [
        ("empty", compress(b""), b""),
        ("one_byte", compress(b"x"), b"x"),
        ("small_40", compress(noise(40, 40)), noise(40, 40)),
        ("small_100", compress(noise(100, 100)), noise(100, 100)),
        ("small_900", compress(noise(900, 900)), noise(900, 900)),
        ("fastq_l1", compress(fq, 1), fq),
        ("fastq_l3", compress(fq, 3), fq),
        ("fastq_l9", compress(fq, 9), fq),
        ("fastq_l19", compress(fq, 19), fq),
        ("fastq_l3_no_checksum_no_size", compress(fq, 3, checksum=False, content_size=False), fq),
        ("incompressible", compress(rnd), rnd),
        ("one_symbol", compress(b"A" * 300_000), b"A" * 300_000),
        ("chain_w17", compress(chain_text(), 3, window_log=17), chain_text()),
        ("all_bytes", compress(bytes(range(256)) * 40), bytes(range(256)) * 40),
    ]
    a, b, c = fastq(60_000, 41), fastq(50_000, 42), fastq(70_000, 43)
    out.append(("three_frames_skippable", compress(a) + skippable(b"between", 3) + compress(b, 9, checksum=False) + compress(c, 1) + skippable(b"", 15), a + b + c))
    out.append(("skippable_first", skippable(b"x" * 300) + compress(a), a))
    _CASES = out
    shapes = {name: walk(comp) for name, comp, _ in out}
    for name, comp, plain in out:
        assert decompress(comp) == plain, name
    s = shapes
    assert s["fastq_l3"]["per_frame"] == [4] and s["fastq_l3"]["types"] == ["compressed"] * 4, s["fastq_l3"]
    for lvl in ("fastq_l1", "fastq_l3"):
        assert {("huffman", 4), ("treeless", 4)} <= s[lvl]["lit"] and "fse" in s[lvl]["weights"], (lvl, s[lvl])
        assert {("ll", "fse"), ("of", "fse"), ("ml", "fse")} <= s[lvl]["modes"], (lvl, s[lvl])
    assert any(m[1] == "repeat" for m in s["fastq_l9"]["modes"] | s["fastq_l19"]["modes"]), (s["fastq_l9"]["modes"], s["fastq_l19"]["modes"])
    assert set(s["incompressible"]["types"]) == {"raw"}, s["incompressible"]["types"]
    assert "rle" in s["one_symbol"]["types"], s["one_symbol"]["types"]
    assert s["small_40"]["types"] == ["raw"] and s["small_100"]["lit"] == {("huffman", 1)} and s["small_900"]["lit"] == {("huffman", 4)}, (s["small_40"], s["small_100"])
    assert s["small_100"]["nseq"] == [0] and s["small_900"]["nseq"] == [0], (s["small_100"], s["small_900"])
    assert s["chain_w17"]["per_frame"] == [5], s["chain_w17"]["per_frame"]
    assert s["three_frames_skippable"]["frames"] == 3 and s["three_frames_skippable"]["skippable_frames"] == 2 and s["three_frames_skippable"]["checksums"] == 2
    assert s["fastq_l3_no_checksum_no_size"]["checksums"] == 0 and s["empty"]["blocks"] == 1
    return _CASES


def by_name(name):
    return next(c for c in cases() if c[0] == name)
