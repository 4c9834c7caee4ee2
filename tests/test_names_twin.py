"""Identifier ranks by radix refinement, on the CPU: lrge_amd/csrc/names_twin.cpp, which runs the rounds
a device form would run over the core of name_core.h, against engine.name_ranks on raw name arrays; the round
counts and the sorted-entry totals against a model written from the reference ordering alone."""
import ctypes as C
import random

import numpy as np
import pytest

FIRST, NEXT = 7, 3          # symbols per key: round 0, later rounds (name_core.h)


def load_twin():
    from lrge_amd import build as Bd
    L = C.CDLL(Bd.build_names_twin())
    L.names_twin_ranks.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.names_twin_max_rounds.argtypes = [C.c_uint32]
    L.names_twin_max_rounds.restype = C.c_uint32
    return L


@pytest.fixture(scope="module")
def twin():
    return load_twin()


def twin_ranks(L, names, idx=None):
    """(rc, ranks of the selection, stats dict) of the twin on `names` (list of bytes), idx None = every name in order"""
    blob = b"".join(names)
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum([len(n) for n in names], out=off[1:])
    if idx is None:
        n, p = len(names), None
    else:
        ix = np.ascontiguousarray(idx, dtype=np.uint32)
        n, p = int(ix.size), (ix.ctypes.data if ix.size else None)
    out = np.full(max(1, n), 0xFFFFFFFF, dtype=np.uint32)
    st = np.zeros(3, dtype=np.uint64)
    rc = L.names_twin_ranks(blob, off.ctypes.data, len(names), p, n, out.ctypes.data, st.ctypes.data)
    return rc, out[:n], dict(rounds=int(st[0]), sorted_entries=int(st[1]), tied_entries=int(st[2]))


def symbols(name, k):
    """the first k symbols of an identifier: byte + 1, 0 past the end"""
    return tuple(name[i] + 1 if i < len(name) else 0 for i in range(k))


def model_stats(sel):
    """rounds, sorted entries and tied entries from the selected names alone: round 0 sorts everything; round k sorts the
    entries whose first FIRST + NEXT * (k - 1) symbols are shared with another entry and do not end with the end symbol"""
    from collections import Counter
    if not sel:
        return dict(rounds=0, sorted_entries=0, tied_entries=0)
    rounds, total, depth = 1, len(sel), FIRST
    active = list(sel)
    while True:
        groups = Counter(symbols(n, depth) for n in active)
        active = [n for n in active if groups[symbols(n, depth)] > 1 and symbols(n, depth)[-1] != 0]
        if not active:
            break
        rounds += 1
        total += len(active)
        depth += NEXT
    c = Counter(sel)
    return dict(rounds=rounds, sorted_entries=total, tied_entries=sum(v for v in c.values() if v > 1))


def check(L, names, idx=None, what=""):
    from lrge_amd import engine
    sel = list(names) if idx is None else [names[i] for i in idx]
    rc, got, st = twin_ranks(L, names, idx)
    assert rc == 0, what
    (exp,) = engine.name_ranks(sel)
    assert np.array_equal(got, exp), (what, got.tolist()[:20], exp.tolist()[:20])
    assert st == model_stats(sel), (what, st, model_stats(sel))
    bound = 1 + max(0, -(-(max(map(len, sel), default=0) + 1 - FIRST) // NEXT))
    assert st["rounds"] <= bound, (what, st, bound)
    assert bound == L.names_twin_max_rounds(max(map(len, sel), default=0)) or not sel
    return st


def pacbio_names(rng, n, movies=1):
    return [b"m64011_190830_220126/%d/ccs" % z if movies == 1 else b"m6401%d_190830_220126/%d/ccs" % (rng.randrange(movies), z)
            for z in rng.sample(range(1, 180_000_000), n)]


def uuid_names(rng, n):
    h = "0123456789abcdef"
    return [("".join(rng.choice(h) for _ in range(8)) + "-" + "".join(rng.choice(h) for _ in range(4)) + "-" + "".join(rng.choice(h) for _ in range(4)) + "-" +
             "".join(rng.choice(h) for _ in range(4)) + "-" + "".join(rng.choice(h) for _ in range(12))).encode() for _ in range(n)]


def test_empty_and_single(twin):
    rc, got, st = twin_ranks(twin, [])
    assert rc == 0 and got.size == 0 and st == dict(rounds=0, sorted_entries=0, tied_entries=0)
    rc, got, st = twin_ranks(twin, [b"abc", b"x"], [])
    assert rc == 0 and got.size == 0 and st["rounds"] == 0
    for name in (b"", b"a", b"abcdefg", b"abcdefgh", b"q" * 40):
        st = check(twin, [name], None, name)
        assert st == dict(rounds=1, sorted_entries=1, tied_entries=0)


def test_all_names_equal(twin):
    for ln in range(0, 27):
        names = [b"z" * ln] * 5
        st = check(twin, names, None, ln)
        # equal identifiers stay together until their end symbol has been read: exactly the bound
        assert st["rounds"] == twin.names_twin_max_rounds(ln) == 1 + max(0, -(-(ln + 1 - FIRST) // NEXT)), (ln, st)
        assert st["tied_entries"] == 5 and st["sorted_entries"] == 5 * st["rounds"]


def test_prefix_chain(twin):
    """a, ab, abc, ... : each name is a proper prefix of the next; the pair of lengths (k, k + 1) first differs at symbol k"""
    alpha = bytes(range(ord("a"), ord("z") + 1))
    for top in range(1, 26):
        names = [alpha[:k] for k in range(1, top + 1)]
        random.Random(top).shuffle(names)
        st = check(twin, names, None, top)
        # the longest pair, of lengths top - 1 and top, is apart once symbol top - 1 has been read: top symbols
        assert st["rounds"] == 1 + max(0, -(-(top - FIRST) // NEXT)), (top, st)
        assert st["tied_entries"] == 0
    check(twin, [b""] + [alpha[:k] for k in range(1, 26)], None, "with the empty name")


def test_pairs_first_differing_at_byte_k(twin):
    for k in range(0, 25):
        for tail in (b"", b"tail"):
            a, b = b"p" * k + b"A" + tail, b"p" * k + b"B" + tail
            st = check(twin, [b, a], None, (k, tail))
            assert st["rounds"] == 1 + max(0, -(-(k + 1 - FIRST) // NEXT)), (k, st)     # symbol k is read in that round
            assert st["sorted_entries"] == 2 * st["rounds"] and st["tied_entries"] == 0
            # one name ends where the other goes on
            check(twin, [b"p" * k + b"A", b"p" * k], None, (k, "prefix"))


def test_rounds_are_one_when_names_differ_within_seven_bytes(twin):
    rng = random.Random(3)
    names = [bytes([65 + i // 26, 97 + i % 26]) + bytes(rng.randrange(33, 127) for _ in range(rng.randrange(0, 30))) for i in range(300)]
    st = check(twin, names)
    assert st == dict(rounds=1, sorted_entries=300, tied_entries=0)


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


def test_heavy_ties_over_two_letters(twin):
    rng = random.Random(11)
    names = [bytes(rng.choice(b"ab") for _ in range(rng.randrange(0, 13))) for _ in range(3000)]
    st = check(twin, names)
    assert st["tied_entries"] > 1000 and st["rounds"] == 3          # length 12 plus its end: 7 + 3 + 3 symbols


def test_pacbio_style_names(twin):
    rng = random.Random(17)
    names = pacbio_names(rng, 2500)
    assert all(n[:21] == names[0][:21] for n in names)
    st = check(twin, names)
    assert st["rounds"] >= 6 and st["tied_entries"] == 0
    check(twin, pacbio_names(rng, 1500, movies=3))
    check(twin, uuid_names(rng, 2000))


def test_index_lists_with_repeats(twin):
    from lrge_amd import engine
    rng = random.Random(23)
    names = pacbio_names(rng, 400) + uuid_names(rng, 300) + [b"dup", b"dup", b"du", b""]
    n = len(names)
    sub = rng.sample(range(n), 250)
    check(twin, names, sub, "shuffled subset")
    rep = [rng.randrange(n) for _ in range(900)]
    st = check(twin, names, rep, "repeats")
    assert st["tied_entries"] > 0
    q, t = rng.sample(range(n), 120), rng.sample(range(n), 200)
    rc, got, _ = twin_ranks(twin, names, q + t)
    eq, et = engine.name_ranks([names[i] for i in q], [names[i] for i in t])
    assert rc == 0 and np.array_equal(got[:120], eq) and np.array_equal(got[120:], et)
    check(twin, names, list(range(n)), "identity list")


def test_argument_errors(twin):
    names = [b"a", b"b", b"c"]
    assert twin_ranks(twin, names, [0, 3])[0] == -9
    assert twin_ranks(twin, names, [2 ** 32 - 1])[0] == -9
    out = np.zeros(4, dtype=np.uint32)
    off = np.array([0, 1, 2, 3], dtype=np.uint64)
    assert twin.names_twin_ranks(b"abc", off.ctypes.data, 3, None, 2, out.ctypes.data, None) == -9     # no list: n must be the name count
    assert twin.names_twin_ranks(b"abc", off.ctypes.data, 3, None, 2 ** 32, out.ctypes.data, None) == -3
    assert twin.names_twin_ranks(b"abc", off.ctypes.data, 3, None, 3, out.ctypes.data, None) == 0 and out[:3].tolist() == [0, 1, 2]
