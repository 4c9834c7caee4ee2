"""Identifier ranks by a fixed number of LSD sort passes, on the CPU: lrge_amd/csrc/names_lsd_twin.cpp, the
host backend of the pass loop the device runs (name_lsd_round.h) over the rules of name_lsd.h, against engine.name_ranks on raw
name arrays; the sort and word counts against W = ceil(Lmax / 8); the verdicts; and tools/name_lsd_check.cpp, the same case
families under AddressSanitizer and UBSan in a stand-alone program."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def load_twin():
    from lrge_amd import build as Bd
    L = C.CDLL(Bd.build_names_lsd_twin())
    L.names_lsd_twin_ranks.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
    L.names_lsd_host_sort_ranks.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    L.names_lsd_word_key.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32]
    L.names_lsd_word_key.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def twin():
    return load_twin()


def table(names):
    blob = b"".join(names)
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum([len(n) for n in names], out=off[1:])
    return blob, off


def twin_ranks(L, names, idx=None, max_bytes=0):
    """(rc, ranks of the selection, stats dict) of the twin on `names` (list of bytes), idx None = every name in order"""
    blob, off = table(names)
    if idx is None:
        n, p = len(names), None
    else:
        ix = np.ascontiguousarray(idx, dtype=np.uint32)
        n, p = int(ix.size), (ix.ctypes.data if ix.size else None)
    out = np.full(max(1, n), 0xFFFFFFFF, dtype=np.uint32)
    st = np.zeros(4, dtype=np.uint64)
    rc = L.names_lsd_twin_ranks(blob, off.ctypes.data, len(names), p, n, out.ctypes.data, st.ctypes.data, max_bytes)
    return rc, out[:n], dict(sorts=int(st[0]), words=int(st[1]), distinct=int(st[2]))


def check(L, names, idx=None, what=""):
    from lrge_amd import engine
    sel = list(names) if idx is None else [names[i] for i in idx]
    rc, got, st = twin_ranks(L, names, idx)
    assert rc == 0, what
    (exp,) = engine.name_ranks(sel)
    assert np.array_equal(got, exp), (what, got.tolist()[:20], exp.tolist()[:20])
    W = (max(map(len, sel), default=0) + 7) // 8
    assert st["words"] == W, (what, st)
    if len(sel) >= 2:
        assert st["sorts"] == W + 1, (what, st)
    else:
        assert st["sorts"] == 0, (what, st)
    assert st["distinct"] == len(set(sel)), (what, st)
    return st


def pacbio_names(rng, n, movies=1):
    return [b"m64011_190830_220126/%d/ccs" % z if movies == 1 else b"m6401%d_190830_220126/%d/ccs" % (rng.randrange(movies), z)
            for z in rng.sample(range(1, 180_000_000), n)]


def uuid_names(rng, n):
    h = "0123456789abcdef"
    return [("".join(rng.choice(h) for _ in range(8)) + "-" + "".join(rng.choice(h) for _ in range(4)) + "-" + "".join(rng.choice(h) for _ in range(4)) + "-" +
             "".join(rng.choice(h) for _ in range(4)) + "-" + "".join(rng.choice(h) for _ in range(12))).encode() for _ in range(n)]


def test_word_key_is_the_big_endian_zero_padded_word(twin):
    name = bytes(range(1, 30))
    for ln in (0, 1, 7, 8, 9, 15, 16, 17, 29):
        for shift in range(8):
            for w in range(5):
                exp = int.from_bytes(name[:ln][8 * w:8 * w + 8].ljust(8, b"\0"), "big")
                assert twin.names_lsd_word_key(name[:ln], ln, shift, w) == exp, (ln, shift, w)
    assert twin.names_lsd_word_key(b"\xff\x80\x00\x7f", 4, 5, 0) == 0xFF80007F00000000


def test_empty_and_single(twin):
    rc, got, st = twin_ranks(twin, [])
    assert rc == 0 and got.size == 0 and st == dict(sorts=0, words=0, distinct=0)
    rc, got, st = twin_ranks(twin, [b"abc", b"x"], [])
    assert rc == 0 and got.size == 0 and st["sorts"] == 0
    for name in (b"", b"a", b"abcdefg", b"abcdefgh", b"q" * 40):
        st = check(twin, [name], None, name)
        assert st["sorts"] == 0 and st["distinct"] == 1
    check(twin, [b"abc", b"x"], [1], "one of two")


def test_all_names_equal(twin):
    for ln in range(0, 27):
        st = check(twin, [b"z" * ln] * 5, None, ln)
        assert st["distinct"] == 1 and st["sorts"] == (ln + 7) // 8 + 1


def test_prefix_chain(twin):
    for top in range(0, 21):
        names = [b"a" * k for k in range(0, top + 1)]
        random.Random(top).shuffle(names)
        check(twin, names, None, top)
    alpha = bytes(range(ord("a"), ord("z") + 1))
    names = [alpha[:k] for k in range(0, 26)]
    random.Random(1).shuffle(names)
    check(twin, names, None, "alphabet chain")


def test_pairs_first_differing_at_byte_k(twin):
    for k in range(0, 25):
        for tail in (b"", b"tail"):
            a, b = b"p" * k + b"A" + tail, b"p" * k + b"B" + tail
            check(twin, [b, a], None, (k, tail))
            check(twin, [b"p" * k + b"A", b"p" * k], None, (k, "prefix"))
        for x in (0x00, 0x7f, 0x80, 0xff):
            for y in (0x00, 0x7f, 0x80, 0xff):
                check(twin, [b"p" * k + bytes([x]) + b"t", b"p" * k + bytes([y]) + b"t", b"p" * k], None, (k, x, y))


def test_odd_bytes(twin):
    odd = [0x00, 0x7f, 0x80, 0xff, 0x01, 0xfe]
    names = [b""]
    for a in odd:
        names.append(bytes([a]))
        for b in odd:
            names.append(bytes([a, b]))
            names.append(b"same-prefix" + bytes([a, b]))
            names.append(b"same-prefix" + bytes([a]) + b"\x00" * 3 + bytes([b]))
    names += [b"\x00" * k for k in range(1, 12)] + [b"\xff" * k for k in range(1, 12)]
    random.Random(5).shuffle(names)
    check(twin, names)


def test_trailing_zero_bytes_are_ordered_by_the_length_pass(twin):
    check(twin, [b"ab\0\0", b"ab", b"ab\0", b"ab\0\0", b"ab", b"a", b"ab\0\0\0\0\0\0\0", b"ab\0\0\0\0\0\0"])
    rc, got, _ = twin_ranks(twin, [b"ab\0\0", b"ab\0", b"ab"])
    assert rc == 0 and got.tolist() == [2, 1, 0]


def test_lengths_around_the_word_boundaries(twin):
    rng = random.Random(29)
    for ln in (7, 8, 9, 15, 16, 17):
        names = [bytes(rng.choice(b"xy") for _ in range(ln)) for _ in range(40)]
        names += [names[0][:ln - 1], names[1] + b"x", names[2][:ln - 1] + b"\0", names[3]]
        check(twin, names, None, ln)
    names = [bytes(rng.choice(b"xy") for _ in range(ln)) for ln in (7, 8, 9, 15, 16, 17) for _ in range(30)]
    check(twin, names, None, "mixed")


def test_heavy_ties(twin):
    rng = random.Random(11)
    pool = [bytes(rng.choice(b"ab") for _ in range(rng.randrange(0, 13))) for _ in range(10)]
    names = [rng.choice(pool) for _ in range(1000)]
    st = check(twin, names)
    assert st["distinct"] == len(set(pool) & set(names)) <= 10


def test_shared_prefix_and_r_style_names(twin):
    rng = random.Random(17)
    names = pacbio_names(rng, 600)
    assert all(n[:21] == names[0][:21] for n in names)
    check(twin, names)
    check(twin, [b"r%08d" % i for i in range(60, 75)])
    check(twin, [b"r%08d" % i for i in reversed(range(60, 75))])


def test_large_uuid_and_pacbio_sets(twin):
    rng = random.Random(19)
    st = check(twin, uuid_names(rng, 5000))
    assert st["words"] == 5 and st["sorts"] == 6
    st = check(twin, pacbio_names(rng, 5000))
    assert st["words"] == 5                       # 21 bytes of movie, up to 9 digits, "/ccs"
    check(twin, pacbio_names(rng, 1500, movies=3))


def test_index_lists_with_repeats_and_two_lists(twin):
    from lrge_amd import engine
    rng = random.Random(23)
    names = pacbio_names(rng, 400) + uuid_names(rng, 300) + [b"dup", b"dup", b"du", b""]
    n = len(names)
    check(twin, names, rng.sample(range(n), 250), "shuffled subset")
    st = check(twin, names, [rng.randrange(n) for _ in range(900)], "repeats")
    assert st["distinct"] < 900
    check(twin, names, list(reversed(range(n))), "reverse order")
    check(twin, names, list(range(n)), "identity list")
    q, t = rng.sample(range(n), 120), rng.sample(range(n), 200)
    rc, got, _ = twin_ranks(twin, names, q + t)
    eq, et = engine.name_ranks([names[i] for i in q], [names[i] for i in t])
    assert rc == 0 and np.array_equal(got[:120], eq) and np.array_equal(got[120:], et)


def test_every_blob_alignment(twin):
    rng = random.Random(31)
    body = uuid_names(rng, 50) + [b"ab", b"ab\0", b"abcdefgh", b"abcdefghi", b""]
    for lead in range(8):
        names = [b"#" * lead] + body
        check(twin, names, list(range(1, len(names))), lead)
        check(twin, names, None, ("with the lead", lead))


def test_host_sort_export_matches(twin):
    from lrge_amd import engine
    rng = random.Random(37)
    names = uuid_names(rng, 300) + [b"", b"a", b"a\0", b"a"]
    blob, off = table(names)
    idx = np.array([rng.randrange(len(names)) for _ in range(500)], dtype=np.uint32)
    out = np.zeros(500, dtype=np.uint32)
    assert twin.names_lsd_host_sort_ranks(blob, off.ctypes.data, len(names), idx.ctypes.data, 500, out.ctypes.data) == 0
    (exp,) = engine.name_ranks([names[i] for i in idx])
    assert np.array_equal(out, exp)


def test_verdicts(twin):
    names = [b"a", b"b", b"c"]
    assert twin_ranks(twin, names, [0, 3])[0] == -9
    assert twin_ranks(twin, names, [2 ** 32 - 1, 0])[0] == -9
    out = np.zeros(4, dtype=np.uint32)
    off = np.array([0, 1, 2, 3], dtype=np.uint64)
    assert twin.names_lsd_twin_ranks(b"abc", off.ctypes.data, 3, None, 2, out.ctypes.data, None, 0) == -9     # no list: n must be the name count
    assert twin.names_lsd_twin_ranks(b"abc", off.ctypes.data, 3, None, 2 ** 32, out.ctypes.data, None, 0) == -3
    assert twin.names_lsd_twin_ranks(b"abc", off.ctypes.data, 3, None, 3, out.ctypes.data, None, 0) == 0 and out[:3].tolist() == [0, 1, 2]
    bad = np.array([0, 2, 1, 3], dtype=np.uint64)                                                           # offsets that are not monotone
    assert twin.names_lsd_twin_ranks(b"abc", bad.ctypes.data, 3, None, 3, out.ctypes.data, None, 0) == -9
    assert twin_ranks(twin, [b"x" * 257, b"y"])[0] == -10
    assert twin_ranks(twin, [b"x" * 257, b"y", b"z"], [1, 2])[0] == 0                                       # the long one is not selected
    rc, got, st = twin_ranks(twin, [b"x" * 256, b"y", b"x" * 255])
    assert rc == 0 and got.tolist() == [1, 2, 0] and st["words"] == 32 and st["sorts"] == 33
    assert twin_ranks(twin, [b"x" * 40, b"y"], None, max_bytes=39)[0] == -10
    assert twin_ranks(twin, [b"x" * 40, b"y"], None, max_bytes=40)[0] == 0


def test_sanitized_standalone_program(tmp_path):
    """tools/name_lsd_check.cpp: the case families above, generated inside the program, over the same twin, built with
    AddressSanitizer and UBSan as a program of its own and run as a child process."""
    exe = str(tmp_path / "name_lsd_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "lrge_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "name_lsd_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "name_lsd_check: ok" in r.stdout
