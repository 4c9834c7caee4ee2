"""Block-parallel xz decoding without a GPU: the host twin (lrge_amd/csrc/xz_twin.cpp, which runs xz_round.h's walk, rounds and
launches over the loops of xz_core.h, with the 64 lanes of every copy step) against liblzma over the corpus of tests/xz_corpus.py
and the streams of tests/xz_writer.py; what is not accepted, beside what liblzma does with it; a seeded campaign of single-byte
edits; the public surface."""
import ctypes as C
import lzma
import os
import random
import re
import struct

import pytest

import xz_corpus as X
import xz_writer as XW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT_KEYS = ("streams", "blocks", "chunks", "raw_chunks", "checks_checked", "rounds", "launches", "bytes_out")
# xz_core.h
(E_MAGIC, E_INPUT, E_FOOTER, E_RESERVED, E_CHECK_ID, E_HEADER_CRC, E_FLAGS, E_INDEX, E_FILTER, E_PADDING, E_SIZES, E_CONTROL, E_PROPS, E_DICT_SIZE, E_DIST,
 E_END_MARKER, E_MATCH_CROSS, E_RC, E_CHECK, E_FEW_BLOCKS, E_TOO_BIG) = range(1, 22)


@pytest.fixture(scope="module")
def xtwin():
    from lrge_amd import build as B
    return load_twin(B.build_xz_twin())


def load_twin(path):
    L = C.CDLL(path)
    L.xz_twin_inflate.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.xz_twin_result.argtypes = [C.c_void_p]
    L.xz_twin_result.restype = C.c_uint64
    L.xz_twin_crc.argtypes = [C.c_char_p, C.c_uint64, C.c_int]
    L.xz_twin_crc.restype = C.c_uint64
    return L


def run(L, data, round_blocks=0, launch_bytes=0, check=1, min_blocks=0, budget=0):
    """(rc, bytes, stats, byte offset): rc 0 decoded, > 0 the XZ_E_* status"""
    st = (C.c_uint64 * 8)()
    bad = C.c_uint64()
    rc = L.xz_twin_inflate(data, len(data), round_blocks, launch_bytes, check, min_blocks, budget, st, C.byref(bad))
    n = L.xz_twin_result(None)
    buf = C.create_string_buffer(max(1, n))
    L.xz_twin_result(buf)
    return rc, buf.raw[:n], dict(zip(STAT_KEYS, list(st))), bad.value


def all_cases():
    return X.cases() + XW.cases()


def launches_of(comp, round_blocks, launch_bytes):
    """the launches the driver must take: per round, the most launches any of its blocks needs"""
    w = X.walk(comp)
    per = w["per_block"] if launch_bytes == 1 else [1 if k else 0 for k in w["per_block"]]      # (no corpus block is above 2 MiB but chunk_of_2_mib's)
    k = round_blocks or 4096
    return sum(max(per[i:i + k]) for i in range(0, len(per), k))


@pytest.mark.parametrize("round_blocks", [0, 1, 2])
@pytest.mark.parametrize("launch_bytes", [1, 0])
def test_corpus_and_writer_streams_equal_liblzma(xtwin, round_blocks, launch_bytes):
    for name, comp, plain in all_cases():
        assert X.decompress(comp) == plain, name
        rc, out, st, bad = run(xtwin, comp, round_blocks, launch_bytes)
        assert rc == 0 and out == plain, (name, rc, bad, st)
        w = X.walk(comp)
        assert {k: st[k] for k in ("streams", "blocks", "chunks", "raw_chunks")} == {k: w[k] for k in ("streams", "blocks", "chunks", "raw_chunks")}, (name, st, w)
        assert st["checks_checked"] == w["checks"] and st["bytes_out"] == len(plain), (name, st)
        assert st["rounds"] == (-(-st["blocks"] // round_blocks) if round_blocks else min(1, st["blocks"])), (name, st)
        if name != "chunk_of_2_mib":
            assert st["launches"] == launches_of(comp, round_blocks, launch_bytes), (name, st)


def test_one_block_crosses_launches(xtwin):
    name, comp, plain = X.by_name("one_block_300k")
    w = X.walk(comp)
    assert w["blocks"] == 1 and w["chunks"] >= 3
    rc, out, st, _ = run(xtwin, comp, 0, 1)
    assert rc == 0 and out == plain and st["launches"] == w["chunks"] >= 3 and st["rounds"] == 1
    rc, out, st, _ = run(xtwin, comp, 0, 150_000)            # whole chunks of at most 150 000 bytes: the chunks are of 2 MiB at most, here about 100 KB
    assert rc == 0 and out == plain and 2 <= st["launches"] <= w["chunks"]
    # the 2 MiB chunk and its tail: two chunks, the default launch holds one of them
    name, comp, plain = XW.by_name("chunk_of_2_mib")
    rc, out, st, _ = run(xtwin, comp)
    assert rc == 0 and out == plain and st["launches"] == 2
    rc, out, st, _ = run(xtwin, comp, 0, 4 << 20)
    assert rc == 0 and out == plain and st["launches"] == 1


def test_corpus_holds_what_it_says():
    shapes = {name: X.walk(comp) for name, comp, _ in X.cases()}
    assert shapes["random_bytes"]["raw_chunks"] >= 2 and shapes["incompressible_stretches"]["raw_chunks"] >= 1
    assert 0 < shapes["incompressible_stretches"]["raw_chunks"] < shapes["incompressible_stretches"]["chunks"]
    assert shapes["three_streams_padded"]["streams"] == 3 and shapes["fastq_p6"]["blocks"] == 4
    name, comp, plain = X.by_name("three_streams_padded")
    assert lzma.decompress(comp) != plain and X.decompress(comp) == plain      # (lzma.decompress stops at stream padding)


def test_check_option(xtwin):
    for nm, width in (("three_blocks_crc32_sizes", 4), ("three_blocks_crc64_sizes", 8)):
        name, comp, plain = XW.by_name(nm)
        at = X.walk(comp)["check_at"][1]
        flipped = comp[:at] + bytes([comp[at] ^ 1]) + comp[at + 1:]
        rc, _, st, bad = run(xtwin, flipped)
        assert (rc, bad) == (E_CHECK, at) and X.decompress(flipped) is None
        rc, out, st, _ = run(xtwin, flipped, check=0)
        assert rc == 0 and out == plain and st["checks_checked"] == 0


def test_min_blocks_and_budget(xtwin):
    name, comp, plain = XW.by_name("three_blocks_crc32_sizes")
    assert run(xtwin, comp, min_blocks=3)[0] == 0
    rc, _, _, bad = run(xtwin, comp, min_blocks=4)
    assert (rc, bad) == (E_FEW_BLOCKS, 0)
    assert run(xtwin, XW.stream([]), min_blocks=1)[0] == E_FEW_BLOCKS and run(xtwin, XW.stream([]), min_blocks=0)[0] == 0
    assert run(xtwin, comp, 0, budget=len(plain))[0] == 0
    assert run(xtwin, comp, 0, budget=len(plain) - 1)[0] == E_TOO_BIG
    assert run(xtwin, comp, 1, budget=len(plain) - 1)[0] == E_TOO_BIG        # (the twin keeps every round's text: its budget is the whole text)


def test_writer_keeps_its_streams():
    """liblzma decodes every stream the writer writes to the text it intended, and the streams hold the forms they are named for"""
    cases = XW.cases()
    assert len(cases) >= 18
    for name, comp, plain in cases:
        assert X.decompress(comp) == plain, name
    shapes = {name: X.walk(comp) for name, comp, _ in cases}
    ctl = [c for _, _, c in shapes["controls_mid_block"]["chunk_at"]]
    assert [c & 0xE0 if c >= 0x80 else c for c in ctl] == [0xE0, 0x80, 0xA0, 0xC0, 2, 0x80, 0x80, 0xC0, 1, 0xC0, 2, 0xA0, 0xE0]
    assert [c for _, _, c in shapes["slot_classes"]["chunk_at"]][0] == 1
    assert shapes["empty_stream_between"]["streams"] == 3 and shapes["streams_with_padding"]["streams"] == 3
    at, payload, c = shapes["controls_mid_block"]["chunk_at"][6]
    name, comp, plain = XW.by_name("controls_mid_block")
    assert comp[at:at + 3] == bytes([0x80, 0, 0])                            # a chunk of one byte
    name, comp, plain = XW.by_name("chunk_of_2_mib")
    at = X.walk(comp)["chunk_at"][0][0]
    assert comp[at:at + 3] == bytes([0xE0 | 0x1F, 0xFF, 0xFF]) and len(plain) == (1 << 21) + 5


def test_crc64_of_the_writer(xtwin):
    """CRC-64/XZ on the published check value, and the twin's stripes against the writer at sizes around the stripe count"""
    assert XW.crc64(b"123456789") == 0x995DC9BBDF1939FA
    data = XW._noise(5000, 9)
    for n in (0, 1, 63, 64, 65, 127, 128, 129, 4999, 5000):
        assert xtwin.xz_twin_crc(data[:n], n, 1) == XW.crc64(data[:n]), n
        assert xtwin.xz_twin_crc(data[:n], n, 0) == struct.unpack("<I", XW.crc32(data[:n]))[0], n


# ---- what is not accepted ----
def _recrc(data, at, n):
    """data with the CRC32 of data[at, at + n) written behind it"""
    return data[:at + n] + XW.crc32(data[at:at + n]) + data[at + n + 4:]


def _one(block, check=XW.CHECK_CRC32, plain=None, **kw):
    payload, p = block.done()
    return XW.stream([(payload, p if plain is None else plain)], check, **kw)


def not_accepted_cases():
    """(name, bytes, status, byte offset or ("chunk", k) for the k-th chunk's control byte, what liblzma does: "error" or "accepts")"""
    text = XW._noise(30_000, 20)
    ok = XW.by_name("three_blocks_crc32_sizes")[1]
    w = X.walk(ok)
    b0, c0 = w["block_at"][0], w["chunk_at"][0][0]
    hs = c0 - b0                                                            # the block header's size
    ia = w["index_at"][0]
    out = []
    delta = lzma.compress(text, format=lzma.FORMAT_XZ, filters=[{"id": lzma.FILTER_DELTA, "dist": 1}, {"id": lzma.FILTER_LZMA2, "preset": 1}])
    bcj = lzma.compress(text, format=lzma.FORMAT_XZ, filters=[{"id": lzma.FILTER_X86}, {"id": lzma.FILTER_LZMA2, "preset": 1}])
    out.append(("delta_filter", delta, E_FILTER, 12, "accepts"))
    out.append(("bcj_filter", bcj, E_FILTER, 12, "accepts"))
    alone = XW.stream([(XW.raw_payload(text[:3000]), text[:3000])])
    hdr = XW.block_header(filters=XW.vli(3) + XW.vli(1) + b"\0")
    out.append(("a_filter_other_than_lzma2_alone", alone[:12] + hdr + alone[12 + len(hdr):], E_FILTER, 12, "error"))
    sha = lzma.compress(text[:5000], check=lzma.CHECK_SHA256)
    out.append(("sha256_check", sha, E_CHECK_ID, len(sha) - 12, "accepts"))
    out.append(("reserved_check_id", XW.stream([], check=2), E_CHECK_ID, 20, "accepts"))
    flags = bytes([1, XW.CHECK_CRC32])
    res = XW.MAGIC + flags + XW.crc32(flags) + XW.index_and_footer([], flags)
    out.append(("reserved_stream_flag", res, E_RESERVED, len(res) - 12, "error"))
    h = bytearray(ok[b0:b0 + hs])
    h[1] |= 0x04
    out.append(("reserved_block_flag", ok[:b0] + bytes(h[:-4]) + XW.crc32(bytes(h[:-4])) + ok[b0 + hs:], E_RESERVED, b0, "error"))
    h = bytearray(ok[b0:b0 + hs])
    h[3] ^= 1                                                                # (the compressed size field)
    out.append(("header_size_differs_from_index", ok[:b0] + bytes(h[:-4]) + XW.crc32(bytes(h[:-4])) + ok[b0 + hs:], E_SIZES, b0, "error"))
    out.append(("dict_size_byte_41", XW.stream([(XW.raw_payload(text[:3000]), text[:3000])], dict_b=41), E_DICT_SIZE, 12, "error"))
    pk = XW.lits(b"ACGTACGTAC") + [("match", 4, 8), ("lit", 65)]
    B = XW.Block
    out.append(("first_chunk_without_dictionary_reset", _one(B().lzma(pk, 0xC0, (3, 0, 2))), E_CONTROL, ("chunk", 0), "error"))
    b = B().raw(b"ACGTACGT", True)
    b.lc, b.lp, b.pb = 3, 0, 2
    out.append(("lzma_chunk_with_no_properties", _one(b.lzma(pk, 0xA0)), E_CONTROL, ("chunk", 1), "error"))
    out.append(("lc_plus_lp_5", _one(B().lzma(pk, 0xE0, (3, 2, 2))), E_PROPS, ("chunk", 0), "error"))
    out.append(("control_byte_3", _one(B().raw(b"ACGT", True)).replace(b"\x01\x00\x03ACGT", b"\x03\x00\x03ACGT"), E_CONTROL, ("chunk", 0), "error"))
    b = B()
    b.lenient = True
    out.append(("distance_beyond_the_block", _one(b.lzma(XW.lits(b"ACGTACGTAC") + [("match", 11, 4)], 0xE0, (3, 0, 2))), E_DIST, ("chunk", 0), "error"))
    b = B()
    b.lenient = True
    out.append(("rep_at_the_first_byte", _one(b.lzma([("rep", 0, 4), ("lit", 65)], 0xE0, (3, 0, 2))), E_DIST, ("chunk", 0), "error"))
    b = B().raw(XW._noise(6000, 30), True).lzma([("match", 5000, 9), ("lit", 66)], 0xC0, (3, 0, 2))
    out.append(("distance_beyond_the_dictionary_size", _one(b, dict_b=0), E_DIST, ("chunk", 1), "error"))
    b = B()
    b.lenient = True
    b.raw(XW._noise(100, 31), True).raw(XW._noise(50, 32), True).lzma([("match", 60, 5), ("lit", 66)], 0xC0, (3, 0, 2))
    out.append(("distance_beyond_a_mid_block_dictionary_reset", _one(b), E_DIST, ("chunk", 2), "error"))
    b = B().lzma(pk + [("match", 1 << 32, 2)], 0xE0, (3, 0, 2), usize_delta=1)      # (a byte short of its stated size, so the marker is decoded)
    out.append(("end_marker", _one(b, plain=bytes(b.plain) + b"A", sizes=False), E_END_MARKER, ("chunk", 0), "error"))
    b = B().lzma(pk + [("match", 4, 8)], 0xE0, (3, 0, 2), usize_delta=-1)
    out.append(("match_crosses_its_chunk", _one(b, plain=bytes(b.plain[:-1]), sizes=False), E_MATCH_CROSS, ("chunk", 0), "error"))
    out.append(("range_coder_first_byte", _one(B().lzma(pk, 0xE0, (3, 0, 2), first_byte=1)), E_RC, ("chunk", 0), "error"))
    out.append(("range_coder_one_byte_long", _one(B().lzma(pk, 0xE0, (3, 0, 2), extra=b"\0")), E_RC, ("chunk", 0), "error"))
    b = B().lzma(pk, 0xE0, (3, 0, 2))
    out.append(("range_coder_one_byte_short", None, E_RC, ("chunk", 0), "error", b))
    b = B().lzma(pk, 0xE0, (3, 0, 2))
    out.append(("chunks_do_not_sum_to_the_index", _one(b, plain=bytes(b.plain) + b"A", sizes=False), E_SIZES, 12 + len(XW.block_header()) + len(b.payload), "error"))
    ck = w["check_at"][2]
    out.append(("wrong_check", ok[:ck + 3] + bytes([ok[ck + 3] ^ 0x80]) + ok[ck + 4:], E_CHECK, ck, "error"))
    pad_at = next(w["check_at"][i] - 1 for i in range(3) if ok[w["check_at"][i] - 1] == 0 and ok[w["check_at"][i] - 2] == 0)
    out.append(("block_padding_not_zero", ok[:pad_at] + b"\x01" + ok[pad_at + 1:], E_PADDING, None, "error"))
    cut = len(ok) // 2
    while ok[cut - 1] == 0:
        cut += 1
    out.append(("truncated_in_a_block", ok[:cut], E_FOOTER, cut - 12, "error"))
    out.append(("truncated_in_the_footer", ok[:-1], E_FOOTER, len(ok) - 13, "error"))
    out.append(("truncated_in_the_header", ok[:20], E_INPUT, 0, "error"))
    out.append(("bytes_behind_the_last_stream", ok + b"junk", E_FOOTER, len(ok) - 8, "error"))
    out.append(("padding_of_one_byte", ok + b"\0", E_PADDING, len(ok) - 11, "error"))
    out.append(("padding_in_front", b"\0\0\0\0" + ok, E_MAGIC, 0, "error"))
    out.append(("junk_between_streams", ok + b"junk" + ok, E_FOOTER, len(ok) - 8, "error"))
    out.append(("not_xz_at_all", b"@read\nACGT\n+\nIIII\n" * 4, E_MAGIC, 0, "error"))
    out.append(("stream_header_crc", ok[:8] + bytes([ok[8] ^ 1]) + ok[9:], E_HEADER_CRC, 0, "error"))
    out.append(("stream_footer_crc", ok[:-12] + bytes([ok[-12] ^ 1]) + ok[-11:], E_HEADER_CRC, len(ok) - 12, "error"))
    out.append(("index_crc", ok[:-13] + bytes([ok[-13] ^ 1]) + ok[-12:], E_HEADER_CRC, ia, "error"))
    out.append(("block_header_crc", ok[:b0 + hs - 1] + bytes([ok[b0 + hs - 1] ^ 1]) + ok[b0 + hs:], E_HEADER_CRC, b0, "error"))
    f64 = bytes([0, XW.CHECK_CRC64])
    out.append(("flags_differ", ok[:6] + f64 + XW.crc32(f64) + ok[12:], E_FLAGS, 0, "error"))
    idx = bytearray(ok[ia:len(ok) - 12])
    npad = 0
    while idx[len(idx) - 5 - npad] == 0:
        npad += 1
    isz = len(idx)
    i2 = bytearray(idx)
    i2[1] += 1                                                               # one record more than there are
    out.append(("index_record_count", ok[:ia] + bytes(i2[:-4]) + XW.crc32(bytes(i2[:-4])) + ok[ia + isz:], E_INDEX, ia, "error"))
    if npad:
        i3 = bytearray(idx)
        i3[len(i3) - 5] = 1
        out.append(("index_padding_not_zero", ok[:ia] + bytes(i3[:-4]) + XW.crc32(bytes(i3[:-4])) + ok[ia + isz:], E_INDEX, ia, "error"))
    return [_finish(c) for c in out]


def _finish(c):
    if c[1] is not None:
        return c
    # the chunk states one compressed byte fewer than the range coder wrote: the byte goes to the front of what follows
    name, _, status, at, host, b = c
    payload = bytearray(b.payload)
    payload[4] -= 1
    plain = bytes(b.plain)
    return (name, XW.stream([(bytes(payload[:-1]) + b"\0", plain)], XW.CHECK_CRC32, sizes=False), status, 12 + len(XW.block_header()), host)


def test_not_accepted(xtwin):
    """every refusal with its status and file offset; where the decoder is stricter than liblzma 5.2.5 the row says "accepts":
    other filters and SHA-256 (out of scope), and a reserved check ID on a stream of no block (liblzma skips a check it does not
    know).  Inside LZMA2 the decoder refuses nothing liblzma takes."""
    seen = set()
    for name, data, status, at, host in not_accepted_cases():
        rc, _, _, bad = run(xtwin, data)
        assert rc == status, (name, rc, status, bad)
        if isinstance(at, tuple):                                            # ("chunk", k): the control byte of the stream's k-th chunk
            at = X.walk(data)["chunk_at"][at[1]][0]
        if at is not None:
            assert bad == at, (name, bad, at)
        got = X.decompress(data)
        assert ("accepts" if got is not None else "error") == host, (name, host)
        seen.add(status)
    assert seen >= {E_MAGIC, E_INPUT, E_FOOTER, E_RESERVED, E_CHECK_ID, E_HEADER_CRC, E_FLAGS, E_INDEX, E_FILTER, E_PADDING, E_SIZES, E_CONTROL, E_PROPS, E_DICT_SIZE,
                    E_DIST, E_END_MARKER, E_MATCH_CROSS, E_RC, E_CHECK}


def test_first_failing_block_decides(xtwin):
    """two damaged blocks of one round: the status and the offset are the first one's in file order, whatever the launch sizes"""
    name, comp, plain = XW.by_name("three_blocks_crc32_nosizes")
    w = X.walk(comp)
    second, third = w["chunk_at"][1][1] + 700, w["chunk_at"][2][1] + 30
    e = bytearray(comp)
    e[second] ^= 0x55
    e[third] ^= 0x55
    want = run(xtwin, bytes(e), 1)
    assert want[0] != 0
    for rb, lb in ((0, 0), (0, 1), (2, 0), (3, 1)):
        rc, _, _, bad = run(xtwin, bytes(e), rb, lb)
        assert (rc, bad) == (want[0], want[3]), (rb, lb)
    assert X.decompress(bytes(e)) is None


def test_single_byte_edits(xtwin):
    """2 000 and more single-byte edits over small streams of every check kind: every edit gives a refusal or the bytes liblzma
    gives (none is skipped).  The recorded stricter cases are container ones an edit cannot reach past the CRC32s: no edited
    stream that liblzma accepts may be refused"""
    rng = random.Random(78)
    pool = [c for c in all_cases() if c[0] in ("three_blocks_none_sizes", "three_blocks_crc32_nosizes", "three_blocks_crc64_sizes", "reps_every_state",
                                               "lengths_every_pos_state", "streams_with_padding", "empty_stream_between")]
    small = XW.Block().lzma(XW.lits(b"ACGTTGCA") + [("match", 4, 6), ("lit", 10), ("rep", 0, 3)], 0xE0, (3, 0, 2)).raw(b"IIII", False).lzma([("lit", 33), ("srep",)], 0x80)
    for check in (XW.CHECK_NONE, XW.CHECK_CRC32, XW.CHECK_CRC64):
        payload, plain = small.done()
        pool.append(("small_%d" % check, XW.stream([(payload, plain)] * 2, check), plain * 2))
    assert len(pool) == 10
    accepted = refused = stricter = 0
    for name, comp, plain in pool:
        assert run(xtwin, comp)[0] == 0, name
        for _ in range(210):
            i = rng.randrange(len(comp))
            e = bytearray(comp)
            e[i] ^= 1 << rng.randrange(8)
            e = bytes(e)
            rc, out, _, _ = run(xtwin, e, rng.choice((0, 1, 2)), rng.choice((0, 1)))
            got = X.decompress(e)
            if rc == 0:
                accepted += 1
                assert got == out, (name, i)
            else:
                refused += 1
                stricter += got is not None
    assert accepted + refused == 2100 and refused > 1500 and stricter == 0, (accepted, refused, stricter)


def test_public_surface():
    from lrge_amd import _ffi, build as B, engine
    hdr = open(os.path.join(ROOT, "include", "lrge_hip.h")).read()
    assert re.search(r"#define\s+LRGE_GPU_INFLATE_XZ\s+256\b", hdr) and _ffi.GPU_INFLATE_XZ == 256
    assert "lrge_hip_xz_inflate" in _ffi.EXPORTS and re.search(r"\blrge_hip_xz_inflate\s*\(", hdr)
    fields = re.search(r"typedef struct lrge_hip_xz_stats \{(.*?)\}", hdr, re.S).group(1)
    assert re.findall(r"uint64_t\s+(\w+);", fields) == _ffi.XZ_STAT_NAMES and tuple(_ffi.XZ_STAT_NAMES[:8]) == STAT_KEYS
    assert {"streams", "blocks", "chunks", "raw_chunks", "checks_checked", "rounds", "launches", "bytes_out", "check_us"} <= set(_ffi.XZ_STAT_NAMES)
    assert hasattr(engine.Context, "xz_inflate") and hasattr(B, "build_xz_twin") and B.XZ_TWIN_PATH.endswith(".so")
    assert "--gpu-xz" in open(os.path.join(ROOT, "tools", "lrge_hip_cli.cpp")).read()
    assert "xz_inflater" in open(os.path.join(ROOT, "include", "lrge_hip.hpp")).read()
    # without the flag the ingest's answer to xz input is the one it always gave
    assert "reads_open: bzip2, zstd and xz input is decompressed on the host" in open(os.path.join(ROOT, "lrge_amd", "csrc", "host_fastx.inl")).read()


def test_sanitized_standalone_program(tmp_path):
    """tools/xz_check.cpp: the corpus, the writer's streams, the refusals and 300 edited streams over the same twin, built with
    AddressSanitizer and UBSan as a program of its own and run as a child process."""
    import subprocess
    exe = str(tmp_path / "xz_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "lrge_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "xz_check.cpp")])
    d = tmp_path / "cases"
    d.mkdir()
    for name, comp, plain in all_cases():
        (d / (name + ".xz")).write_bytes(comp)
        (d / (name + ".plain")).write_bytes(plain)
    for name, data, status, _, _ in not_accepted_cases():
        (d / ("refused_" + name + ".xz")).write_bytes(data)
        (d / ("refused_" + name + ".status")).write_text(str(status))
    rng = random.Random(3)
    pool = [c[1] for c in all_cases() if len(c[1]) < 20_000]
    for i in range(300):
        e = bytearray(rng.choice(pool))
        e[rng.randrange(len(e))] ^= 1 << rng.randrange(8)
        (d / ("%03d.edit" % i)).write_bytes(bytes(e))
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "xz_check: ok" in r.stdout
