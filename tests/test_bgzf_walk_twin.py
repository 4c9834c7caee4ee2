"""The incremental BGZF block walk of the streamed first pass (lrge_amd/csrc/bgzf_scan.h BgzfWalk) without a
GPU: fed a file in pieces of every size from 1 to the file's length it gives the block table of the whole-buffer scan
(bgzf_scan_blocks, through the host twin lrge_amd/csrc/inflate_twin.cpp), and where that scan refuses a file the walk refuses it
too, naming one file offset whatever the piece.  tools/stream_check.cpp drives the same walk and the byte source
(lrge_amd/csrc/fx_input.h) as a program of its own under AddressSanitizer and UBSan."""
import ctypes as C
import gzip
import os
import random
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_writer as W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_rng = random.Random(30)
TEXT = bytes(_rng.choice(b"ACGTN\n@+") for _ in range(9000))


def _blocks(sizes, **kw):
    out, at = [], 0
    for n in sizes:
        out.append(W.bgzf_block(TEXT[at:at + n], **kw))
        at += n
    return out


GOOD = {
    "blocks_100_to_3000": b"".join(_blocks([100, 3000, 777, 1500]) + [W.EOF_BLOCK]),
    "empty_member_in_the_middle": b"".join(_blocks([900, 1200]) + [W.bgzf_block(b"")] + _blocks([400]) + [W.EOF_BLOCK]),
    "no_end_marker": b"".join(_blocks([1000, 2000])),
    "fname_and_fhcrc": b"".join(_blocks([800]) + [W.bgzf_block(TEXT[:1300], fname=b"reads.fq", comment=b"a comment", fhcrc=True),
                                                  W.bgzf_block(TEXT[:500], extra_before=b"XY\x03\x00abc", extra_after=b"ZZ\x00\x00")] + [W.EOF_BLOCK]),
    "one_member": W.bgzf_block(TEXT[:2500]),
    "end_marker_alone": W.EOF_BLOCK,
}
assert len(W.EOF_BLOCK) == 28


def _bad_fhcrc():
    b = bytearray(W.bgzf_block(TEXT[:600], fhcrc=True))
    b[18] ^= 0x55                                            # (18: the first of the two FHCRC bytes behind the 18-byte header)
    return bytes(b)


def _isize_above_the_limit():
    b = bytearray(W.bgzf_block(TEXT[:600]))
    b[-4:] = struct.pack("<I", 65537)
    return bytes(b)


_good2 = b"".join(_blocks([700, 1100]))
# name -> (file, the offset both walks refuse it at: the start of the first member that is no whole BGZF block)
REFUSED = {
    "truncated_last_member": (_good2 + W.bgzf_block(TEXT[:900])[:-5], len(_good2)),
    "truncated_inside_the_header": (_good2 + W.bgzf_block(TEXT[:900])[:11], len(_good2)),
    "trailing_bytes": (_good2 + b"\x00" * 7, len(_good2)),
    "trailing_text": (_good2 + b"trailing bytes that are no gzip member at all\n", len(_good2)),
    "member_without_bc": (_good2 + gzip.compress(TEXT[:800], 6, mtime=0) + W.EOF_BLOCK, len(_good2)),
    "member_with_another_subfield_only": (_good2 + bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0]) + b"XY\x02\x00ab" + W.deflate_raw(b"x") + struct.pack("<II", zlib.crc32(b"x"), 1), len(_good2)),
    "bad_fhcrc": (_good2 + _bad_fhcrc() + W.EOF_BLOCK, len(_good2)),
    "isize_above_the_limit": (_good2 + _isize_above_the_limit() + W.EOF_BLOCK, len(_good2)),
    "empty_file": (b"", 0),
    "plain_gzip": (gzip.compress(TEXT[:800], 6, mtime=0), 0),
}


# the bytes the file holds of the refused member, where its own 8-byte trailer decides (the ISIZE word; the missing end)
OWN_TRAILER = {"isize_above_the_limit": len(_isize_above_the_limit()), "truncated_last_member": len(W.bgzf_block(TEXT[:900])) - 5}


@pytest.fixture(scope="module")
def twin():
    from lrge_amd import build as B
    L = C.CDLL(B.build_twin())
    u64p = C.POINTER(C.c_uint64)
    L.inflate_twin_scan_table.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p, u64p]
    L.inflate_twin_walk_pieces.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, u64p, u64p, u64p]
    return L


CAP = 64


def whole(L, data):
    """(table [n, 7], text bytes) of the whole-buffer scan, or None: refused"""
    tab, n, total = np.zeros((CAP, 7), dtype=np.uint64), C.c_uint64(), C.c_uint64()
    if L.inflate_twin_scan_table(data, len(data), tab.ctypes.data, CAP, C.byref(n), C.byref(total)) != 0:
        return None
    assert n.value <= CAP
    return tab[:n.value].copy(), total.value


def pieces(L, data, piece):
    """the same of the incremental walk over pieces of `piece` bytes, or ("refused", file offset)"""
    tab, n, total, bad = np.zeros((CAP, 7), dtype=np.uint64), C.c_uint64(), C.c_uint64(), C.c_uint64()
    if L.inflate_twin_walk_pieces(data, len(data), piece, tab.ctypes.data, CAP, C.byref(n), C.byref(total), C.byref(bad)) != 0:
        return "refused", bad.value
    assert n.value <= CAP
    return tab[:n.value].copy(), total.value


@pytest.mark.parametrize("name", sorted(GOOD))
def test_every_piece_size_gives_the_whole_buffer_table(twin, name):
    data = GOOD[name]
    ref = whole(twin, data)
    assert ref is not None and len(ref[0]) >= 1
    assert int(ref[0][:, 4].sum()) == len(data)              # (the members tile the file)
    for piece in range(1, len(data) + 1):
        got = pieces(twin, data, piece)
        assert not isinstance(got[0], str), (name, piece, got)
        assert got[1] == ref[1] and np.array_equal(got[0], ref[0]), (name, piece)


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_both_walks_refuse_and_the_offset_is_one(twin, name):
    data, off = REFUSED[name]
    assert whole(twin, data) is None
    for piece in range(1, max(1, len(data)) + 1):
        assert pieces(twin, data, piece) == ("refused", off), (name, piece)


def test_piece_boundaries_inside_header_extra_field_and_trailer(twin):
    """said outright for one file a refusal kind, although the sweeps above cover it: the third member starts at `off`; its 18-byte
    header, its extra field (bytes 12 to 18 of it), the 8-byte trailer of the member in front and -- where it decides -- the refused
    member's own trailer are each cut by a boundary"""
    for name in ("truncated_last_member", "trailing_text", "member_without_bc", "bad_fhcrc", "isize_above_the_limit"):
        data, off = REFUSED[name]
        cuts = [off + 5, off + 14, off - 3]                  # inside the header, inside the extra field, inside the trailer in front
        if name in OWN_TRAILER:                              # ... and inside what the file has of the refused member's own trailer, which decides
            cuts.append(off + OWN_TRAILER[name] - 3)
        for cut in cuts:
            hit = [p for p in range(2, len(data)) if cut % p == 0 and 0 < cut < len(data)]
            assert hit, (name, cut)
            for piece in hit[:3] + hit[-1:]:
                assert pieces(twin, data, piece) == ("refused", off), (name, cut, piece)
    data = GOOD["fname_and_fhcrc"]
    ref = whole(twin, data)
    starts = [int(x) for x in ref[0][:, 0]]
    for s in starts[1:]:
        for cut in (s + 5, s + 14, s - 3):
            for piece in [p for p in range(2, len(data)) if cut % p == 0][:4]:
                got = pieces(twin, data, piece)
                assert not isinstance(got[0], str) and np.array_equal(got[0], ref[0]), (cut, piece)


def test_sanitized_standalone_program(tmp_path):
    """tools/stream_check.cpp: fx_input.h and the incremental walk on the files above at a few piece sizes against a whole-file
    read, built with AddressSanitizer and UBSan as a program of its own and run as a child process"""
    exe = str(tmp_path / "stream_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "lrge_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "stream_check.cpp")])
    files = []
    for name, data in list(GOOD.items()) + [(k, v[0]) for k, v in REFUSED.items()] + [("plain_text", TEXT)]:
        files.append(str(tmp_path / name))
        (tmp_path / name).write_bytes(data)
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "stream_check: ok (%d files)" % len(files) in r.stdout
