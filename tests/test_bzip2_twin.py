"""Block-parallel bzip2 decoding without a GPU: the host twin (lrge_amd/csrc/bz_twin.cpp, which runs bz_round.h's rounds and chain
over the loops of bz_core.h) against libbz2 over the corpus of tests/bzip2_corpus.py and the streams of tests/bzip2_writer.py;
the finder at every bit alignment; the chain on edited candidate lists; what is not accepted, beside what the C++ host reader
does with it; a seeded campaign of single-byte edits."""
import bz2
import ctypes as C
import os
import random
import time

import pytest

import bzip2_corpus as Z
import bzip2_writer as ZW

END_FLAG = 1 << 63
BLOCK_MAGIC, END_MAGIC = ZW.BLOCK_MAGIC, ZW.END_MAGIC
E_INPUT, E_RANDOMISED, E_BLOCK_CRC, E_STREAM_CRC, E_TRAILING, E_CHAIN, E_RUN = 2, 3, 11, 12, 13, 14, 15      # bz_core.h
STAT_KEYS = ("blocks", "candidates", "rejected_candidates", "rounds", "bytes_out")


@pytest.fixture(scope="module")
def btwin():
    from lrge_amd import build as B
    return load_twin(B.build_bzip2_twin())


def load_twin(path):
    L = C.CDLL(path)
    L.bz_twin_inflate.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.c_int64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.bz_twin_result.argtypes = [C.c_void_p]
    L.bz_twin_result.restype = C.c_uint64
    L.bz_twin_find.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint64]
    L.bz_twin_find.restype = C.c_uint64
    return L


def run(L, data, round_blocks=0, cand=None):
    """(rc, bytes, stats, byte offset): rc 0 decoded, > 0 the BZ_E_* status"""
    st = (C.c_uint64 * 5)()
    bad = C.c_uint64()
    if cand is None:
        rc = L.bz_twin_inflate(data, len(data), round_blocks, None, -1, st, C.byref(bad))
    else:
        arr = (C.c_uint64 * max(1, len(cand)))(*cand)
        rc = L.bz_twin_inflate(data, len(data), round_blocks, arr, len(cand), st, C.byref(bad))
    n = L.bz_twin_result(None)
    buf = C.create_string_buffer(max(1, n))
    L.bz_twin_result(buf)
    return rc, buf.raw[:n], dict(zip(STAT_KEYS, list(st))), bad.value


def find(L, data):
    cap = len(data) + 16
    arr = (C.c_uint64 * cap)()
    n = L.bz_twin_find(data, len(data), arr, cap)
    assert n <= cap
    return list(arr[:n])


def libbz2_first_stream(data):
    """what libbz2 returns for the first stream of `data` (the C++ host reader's BzDecoder), or None when it gives an error"""
    d = bz2.BZ2Decompressor()
    try:
        out = d.decompress(data)
    except Exception:
        return None
    return out if d.eof else None


@pytest.mark.parametrize("round_blocks", [0, 1, 2])
def test_corpus_equals_libbz2(btwin, round_blocks):
    for name, comp, plain in Z.cases():
        assert bz2.decompress(comp) == plain, name
        rc, out, st, _ = run(btwin, comp, round_blocks)
        assert rc == 0 and out == plain, (name, rc, st)
        assert st["bytes_out"] == len(plain) and st["rejected_candidates"] == 0 and st["blocks"] == st["candidates"], (name, st)
        if round_blocks:
            assert st["rounds"] == -(-st["blocks"] // round_blocks), (name, st)


def test_corpus_shapes(btwin):
    """the corpus is what its names say: block counts, block starts off the byte grid, a 14-byte empty stream"""
    by = {name: (comp, plain) for name, comp, plain in Z.cases()}
    assert len(by["empty"][0]) == 14
    blocks = {name: run(btwin, comp)[2]["blocks"] for name, (comp, _) in by.items()}
    assert blocks["empty"] == 0 and blocks["one_byte"] == 1 and blocks["one_block"] == 1 and blocks["three_blocks"] == 3, blocks
    assert blocks["three_blocks_as_one_l9"] == 1 and blocks["run_over_block_boundary"] == 2 and blocks["block_ends_inside_run"] == 2, blocks
    starts = [c for c in find(btwin, by["three_blocks"][0]) if not c & END_FLAG]
    assert len(starts) == 3 and starts[0] == 32 and all(s % 8 for s in starts[1:]), starts


def test_writer_streams_equal_libbz2(btwin):
    assert len(ZW.dropped()) <= 2, ZW.dropped()
    assert len(ZW.cases()) >= 14
    for name, comp, plain in ZW.cases():
        for k in (0, 1):
            rc, out, st, _ = run(btwin, comp, k)
            assert rc == 0 and out == plain, (name, k, rc, st)


def test_finder_at_every_bit_alignment(btwin):
    rng = random.Random(5)
    for kind, magic in ((0, BLOCK_MAGIC), (END_FLAG, END_MAGIC)):
        for shift in range(8):
            for at in (0, 1, 15, 16, 17, 100):
                n = at + 7 + 40
                v = int.from_bytes(bytes(rng.randrange(256) for _ in range(n)), "big")
                lo = 8 * n - (8 * at + shift) - 48
                v = (v & ~(((1 << 48) - 1) << lo)) | magic << lo
                data = v.to_bytes(n, "big")
                assert 8 * at + shift | kind in find(btwin, data), (kind, shift, at)
    # a magic cut off by the end of the input is no candidate
    data = (BLOCK_MAGIC >> 8).to_bytes(5, "big")
    assert find(btwin, b"\0" * 20 + data) == []
    assert find(btwin, b"\0" * 20 + BLOCK_MAGIC.to_bytes(6, "big")) == [160]


def test_chain_rejects_candidates_off_the_chain(btwin):
    _, comp, plain = Z.three_blocks()
    true = find(btwin, comp)
    assert sum(1 for c in true if not c & END_FLAG) == 3 and sum(1 for c in true if c & END_FLAG) == 1
    rng = random.Random(9)
    end = max(c & ~END_FLAG for c in true)
    fakes = sorted(rng.sample([b for b in range(33, end) if b not in true], 20))
    mixed = sorted(true + fakes, key=lambda c: c & ~END_FLAG)
    for k in (0, 1, 2, 5):
        rc, out, st, _ = run(btwin, comp, k, mixed)
        assert rc == 0 and out == plain, (k, rc)
        assert st["rejected_candidates"] == len(fakes) and st["blocks"] == 3 and st["candidates"] == 3 + len(fakes), (k, st)


def test_chain_reports_a_missing_start(btwin):
    _, comp, _ = Z.three_blocks()
    true = find(btwin, comp)
    for drop in range(len(true)):
        rc, out, st, bad = run(btwin, comp, 0, true[:drop] + true[drop + 1:])
        assert rc == E_CHAIN and bad <= len(comp), (drop, rc, bad)
        if drop == 0:
            assert bad == 4


def not_accepted_cases():
    """(name, bytes, the status, what the host reader gives: the first stream's text, or None for an error)"""
    _, comp, plain = Z.three_blocks()
    other = bz2.compress(b"second stream", 1)
    rnd = bytearray(comp)
    rnd[14] |= 0x80                                     # bit 112 = 32 + 48 + 32: the first block's randomised bit
    bad_block = bytearray(comp)
    bad_block[10] ^= 1                                  # inside the first block's stored CRC (bits 80..111)
    # (stream_crc: a bit of the combined CRC behind the end magic, flipped by flip_stream_crc where the finder is at hand)
    return [("two_streams", comp + other, E_TRAILING, plain),
            ("trailing_byte", comp + b"\0", E_TRAILING, plain),
            ("randomised", bytes(rnd), E_RANDOMISED, None),
            ("truncated", comp[:len(comp) // 2], None, None),
            ("truncated_in_trailer", comp[:-3], E_INPUT, None),
            ("block_crc", bytes(bad_block), E_BLOCK_CRC, None),
            ("stream_crc", comp, E_STREAM_CRC, None),
            ("stops_behind_four_equal", ZW.stops_behind_four_equal(), E_RUN, None)]


def flip_stream_crc(L, comp):
    end = next(c & ~END_FLAG for c in find(L, comp) if c & END_FLAG)
    d = bytearray(comp)
    bit = end + 48 + 5
    d[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(d)


def test_not_accepted(btwin):
    _, comp, plain = Z.three_blocks()
    for name, data, status, host in not_accepted_cases():
        if name == "stream_crc":
            data = flip_stream_crc(btwin, comp)
        rc, _, _, bad = run(btwin, data)
        assert rc > 0 and (status is None or rc == status), (name, rc)
        assert bad <= len(data), (name, bad)
        assert libbz2_first_stream(data) == host, name


def edited(comp, k, seed):
    rng = random.Random(seed)
    for _ in range(k):
        d = bytearray(comp)
        at = rng.randrange(len(d))
        d[at] ^= 1 << rng.randrange(8)
        yield at, bytes(d)


def test_single_byte_edits(btwin):
    _, comp, plain = Z.three_blocks()
    accepted = 0
    for at, d in edited(comp, 300, 77):
        t0 = time.perf_counter()
        rc, out, _, _ = run(btwin, d)
        assert time.perf_counter() - t0 < 1.0, at
        if rc == 0:
            assert out == libbz2_first_stream(d), at
            accepted += 1
    assert accepted <= 300


def test_host_reader_on_the_not_accepted(btwin, tmp_path):
    """the C++ host reader (lrge_hip_read_records, libbz2 on the host): the records of the first stream where libbz2 returns it,
    an error otherwise"""
    from lrge_amd import _ffi
    L = _ffi.lib()
    CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_char), C.c_uint64, C.POINTER(C.c_char), C.c_uint64)
    L.lrge_hip_read_records.argtypes = [C.c_char_p, CB, C.c_void_p, C.c_char_p, C.c_uint64]
    _, comp, plain = Z.three_blocks()
    for name, data, _, host in not_accepted_cases():
        if name == "stream_crc":
            data = flip_stream_crc(btwin, comp)
        p = tmp_path / (name + ".fq.bz2")
        p.write_bytes(data)
        n = [0]
        cb = CB(lambda u, a, al, b, bl: n.__setitem__(0, n[0] + 1))
        err = C.create_string_buffer(512)
        rc = L.lrge_hip_read_records(os.fsencode(str(p)), cb, None, err, 512)
        if host is not None:
            assert rc == 0 and n[0] == host.count(b"\n") // 4 > 100, (name, rc, err.value)
        else:
            assert rc != 0, name
