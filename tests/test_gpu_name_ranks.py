"""Identifier ranks on the device by fixed LSD passes (lrge_hip_name_ranks, lrge_hip_reads_name_ranks) against
engine.name_ranks: the case families of tests/test_names_lsd_twin.py through ctypes and the C ABI, the edges of the wavefront and
of the sort's and the scan's 4096-entry tiles, one multi-tile run, an ordinary overlap call on the same context afterwards,
DeviceReads.name_ranks resident and windowed, and the opt-in callers: the strategies and lrge-hip --gpu-names."""
import ctypes as C
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT, to_arrays

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOY = os.path.join(GOLDEN, "toy_reads.fa.gz")


@pytest.fixture(scope="module")
def nctx():
    """a context of this module's own: the device form stays off the session context of the other GPU tests"""
    from lrge_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def dev_ranks(ctx, names, idx=None):
    """(rc, ranks, stats) of lrge_hip_name_ranks on `names` (list of bytes); idx None: every name in order"""
    blob = b"".join(names)
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum([len(n) for n in names], out=off[1:])
    if idx is None:
        n, p = len(names), None
    else:
        ix = np.ascontiguousarray(idx, dtype=np.uint32)
        n, p = int(ix.size), (ix.ctypes.data if ix.size else None)
    out = np.full(max(1, n), 0xFFFFFFFF, dtype=np.uint32)
    st = np.zeros(4, dtype=np.uint64)
    rc = ctx._lib.lrge_hip_name_ranks(ctx.h, blob, off.ctypes.data, len(names), p, n, out.ctypes.data, st.ctypes.data)
    return rc, out[:n], dict(sorts=int(st[0]), words=int(st[1]), distinct=int(st[2]), us=int(st[3]))


def check(ctx, names, idx=None, what=""):
    from lrge_amd import engine
    sel = list(names) if idx is None else [names[i] for i in idx]
    rc, got, st = dev_ranks(ctx, names, idx)
    assert rc == 0, (what, ctx._lib.lrge_hip_last_error(ctx.h))
    (exp,) = engine.name_ranks(sel)
    assert np.array_equal(got, exp), (what, got.tolist()[:20], exp.tolist()[:20])
    W = (max(map(len, sel), default=0) + 7) // 8
    assert st["words"] == W and st["sorts"] == (W + 1 if len(sel) >= 2 else 0), (what, st)
    assert st["distinct"] == len(set(sel)), (what, st)
    return st


def pacbio_names(rng, n, top=180_000_000):
    return [b"m64011_190830_220126/%d/ccs" % z for z in rng.sample(range(1, top), n)]


def uuid_names(rng, n):
    h = "0123456789abcdef"
    return [("".join(rng.choice(h) for _ in range(8)) + "-" + "".join(rng.choice(h) for _ in range(4)) + "-" + "".join(rng.choice(h) for _ in range(4)) + "-" +
             "".join(rng.choice(h) for _ in range(4)) + "-" + "".join(rng.choice(h) for _ in range(12))).encode() for _ in range(n)]


def families():
    """(what, names, idx) of the twin test's case families, at its sizes"""
    rng = random.Random(41)
    yield "empty", [], None
    yield "empty selection", [b"abc", b"x"], []
    for name in (b"", b"a", b"abcdefg", b"abcdefgh", b"q" * 40):
        yield ("single", name), [name], None
    for ln in range(0, 27):
        yield ("all equal", ln), [b"z" * ln] * 5, None
    for top in range(0, 21):
        names = [b"a" * k for k in range(0, top + 1)]
        random.Random(top).shuffle(names)
        yield ("prefix chain", top), names, None
    odd = (0x00, 0x7f, 0x80, 0xff)
    for k in range(0, 25):
        p = b"p" * k
        yield ("pair", k), [p + b"B", p + b"A"], None
        yield ("pair with tail", k), [p + b"Btail", p + b"Atail"], None
        yield ("pair, one ends", k), [p + b"A", p], None
        # the four bytes at the parting position, all in one call: every ordered pair of them meets
        yield ("odd bytes", k), [p + bytes([x]) + b"t" for x in odd] + [p] + [p + bytes([x]) for x in odd], None
    yield "trailing zero bytes", [b"ab\0\0", b"ab", b"ab\0", b"ab\0\0", b"ab", b"a", b"ab\0\0\0\0\0\0\0", b"ab\0\0\0\0\0\0"], None
    for ln in (7, 8, 9, 15, 16, 17):
        names = [bytes(rng.choice(b"xy") for _ in range(ln)) for _ in range(40)]
        names += [names[0][:ln - 1], names[1] + b"x", names[2][:ln - 1] + b"\0", names[3]]
        yield ("word boundary", ln), names, None
    pool = [bytes(rng.choice(b"ab") for _ in range(rng.randrange(0, 13))) for _ in range(10)]
    yield "heavy ties", [rng.choice(pool) for _ in range(1000)], None
    yield "21-byte shared prefix", pacbio_names(rng, 600), None
    yield "r-style", [b"r%08d" % i for i in range(60, 75)], None
    yield "r-style reversed", [b"r%08d" % i for i in reversed(range(60, 75))], None
    names = pacbio_names(rng, 400) + uuid_names(rng, 300) + [b"dup", b"dup", b"du", b""]
    n = len(names)
    yield "shuffled subset", names, rng.sample(range(n), 250)
    yield "repeats", names, [rng.randrange(n) for _ in range(900)]
    yield "reverse order", names, list(reversed(range(n)))
    yield "5000 UUID-like", uuid_names(rng, 5000), None
    yield "5000 PacBio-like", pacbio_names(rng, 5000), None
    body = uuid_names(rng, 50) + [b"ab", b"ab\0", b"abcdefgh", b"abcdefghi", b""]
    for lead in range(8):
        yield ("alignment", lead), [b"#" * lead] + body, list(range(1, len(body) + 1))


def test_case_families(nctx):
    for what, names, idx in families():
        check(nctx, names, idx, what)


def test_two_lists_ranked_together(nctx):
    from lrge_amd import engine
    rng = random.Random(23)
    names = pacbio_names(rng, 400) + uuid_names(rng, 300) + [b"dup", b"dup", b"du", b""]
    q, t = rng.sample(range(len(names)), 120), rng.sample(range(len(names)), 200)
    rc, got, _ = dev_ranks(nctx, names, q + t)
    eq, et = engine.name_ranks([names[i] for i in q], [names[i] for i in t])
    assert rc == 0 and np.array_equal(got[:120], eq) and np.array_equal(got[120:], et)
    gq, gt = nctx.name_ranks([names[i] for i in q], [names[i] for i in t])
    assert np.array_equal(gq, eq) and np.array_equal(gt, et)
    assert nctx.name_rank_stats["sorts"] == nctx.name_rank_stats["words"] + 1


def test_verdicts(nctx):
    from lrge_amd import _ffi
    names = [b"a", b"b", b"c"]
    assert dev_ranks(nctx, names, [0, 3])[0] == -9
    L = nctx._lib
    out = np.zeros(4, dtype=np.uint32)
    off = np.array([0, 1, 2, 3], dtype=np.uint64)
    assert L.lrge_hip_name_ranks(nctx.h, b"abc", off.ctypes.data, 3, None, 2, out.ctypes.data, None) == -9
    assert L.lrge_hip_name_ranks(nctx.h, b"abc", off.ctypes.data, 3, None, 2 ** 32, out.ctypes.data, None) == -3
    assert dev_ranks(nctx, [b"x" * 257, b"y"])[0] == -10
    with pytest.raises(_ffi.UnprovenInput):
        nctx.name_ranks([b"x" * 257, b"y"])
    rc, got, st = dev_ranks(nctx, [b"x" * 256, b"y", b"x" * 255])
    assert rc == 0 and got.tolist() == [1, 2, 0] and st["words"] == 32 and st["sorts"] == 33
    nctx.set_option("NAME_RANK_MAX_BYTES", 39)
    try:
        assert dev_ranks(nctx, [b"x" * 40, b"y"])[0] == -10
        assert dev_ranks(nctx, [b"x" * 39, b"y"])[0] == 0
    finally:
        nctx.set_option("NAME_RANK_MAX_BYTES", None)
    nctx.set_option("DEBUG_ALLOC_FAIL_ALWAYS", 1)                  # memory that cannot be had
    try:
        assert dev_ranks(nctx, names)[0] == _ffi.ERR_DEVICE
    finally:
        nctx.set_option("DEBUG_ALLOC_FAIL_ALWAYS", None)
    check(nctx, names)


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 4095, 4096, 4097, 8193])
def test_wavefront_and_tile_edges(nctx, n):
    rng = random.Random(n)
    check(nctx, uuid_names(rng, n), None, ("uuid", n))
    names = [b"the-same-twenty-three-" + bytes([rng.randrange(256)]) for _ in range(n)]      # equal but for the last byte
    check(nctx, names, None, ("last byte", n))


def toy_reads():
    txt = gzip.open(TOY).read().split(b">")[1:]
    return [r.split(b"\n", 1)[0].split()[0] for r in txt], [r.split(b"\n", 1)[1].replace(b"\n", b"") for r in txt]


def test_multi_tile_run_then_an_ordinary_overlap(nctx):
    """200 000 PacBio-like names (32 bytes at most: W = 4) with 1 % duplicates; then the same context maps the toy reads with the
    device's ranks and with the host's: the arena and the stream are left sound"""
    from lrge_amd import engine
    rng = random.Random(5)
    names = pacbio_names(rng, 198_000, top=10_000_000)
    names += [names[rng.randrange(len(names))] for _ in range(2_000)]
    rng.shuffle(names)
    st = check(nctx, names, None, "200 000")
    assert st["words"] == 4 and st["sorts"] == 5 and st["distinct"] < 200_000
    tn, ts = toy_reads()
    q, t = list(range(0, 150)), list(range(150, 450))
    qn, tnn = [tn[i] for i in q], [tn[i] for i in t]
    hq, ht = engine.name_ranks(qn, tnn)
    dq, dt = nctx.name_ranks(qn, tnn)
    assert np.array_equal(hq, dq) and np.array_equal(ht, dt)
    res = []
    for qr, tr in ((dq, dt), (hq, ht)):
        Q = nctx.upload(*to_arrays([ts[i] for i in q]), qr)
        T = nctx.upload(*to_arrays([ts[i] for i in t]), tr)
        ix = engine.Index(nctx, T, 0)
        res.append(ix.overlap_twoset(Q))
        ix.free(); Q.free(); T.free()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and int(res[0][0].sum()) > 0


def test_device_reads_name_ranks(nctx):
    """a handle opened from the toy reads, resident and through windows: DeviceReads.name_ranks and lrge_hip_reads_name_ranks
    against engine.name_ranks of the same names, without the names list being built"""
    from lrge_amd import _ffi, engine
    tn, _ = toy_reads()
    rng = random.Random(3)
    q, t = rng.sample(range(500), 150), [rng.randrange(500) for _ in range(300)]
    eq, et = engine.name_ranks([tn[i] for i in q], [tn[i] for i in t])
    (eall,) = engine.name_ranks(tn)
    data = gzip.open(TOY).read()                   # (plain text: a gzip member of this size arrives in one round, i.e. one window)
    flags = _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INGEST_WINDOWED
    for window in (None, 262144):
        if window:
            nctx.set_option("INGEST_WINDOW_BYTES", window)
        try:
            dr = nctx.open_reads(data, flags)
        finally:
            nctx.set_option("INGEST_WINDOW_BYTES", None)
        assert dr.n == 500 and (dr.window_stats()[0] >= 2 if window else dr.window_stats()[0] == 0), dr.window_stats()
        gq, gt = dr.name_ranks(q, t)
        assert np.array_equal(gq, eq) and np.array_equal(gt, et), window
        (gall,) = dr.name_ranks(np.arange(500))
        assert np.array_equal(gall, eall)
        assert dr._names is None
        # the handle's own form
        idx = np.array(q + t, dtype=np.uint32)
        out = np.zeros(idx.size, dtype=np.uint32)
        st = np.zeros(4, dtype=np.uint64)
        assert nctx._lib.lrge_hip_reads_name_ranks(dr.h, idx.ctypes.data, idx.size, out.ctypes.data, st.ctypes.data) == 0
        assert np.array_equal(out[:150], eq) and np.array_equal(out[150:], et) and st[0] == 6 and st[1] == 5
        out = np.zeros(500, dtype=np.uint32)
        assert nctx._lib.lrge_hip_reads_name_ranks(dr.h, None, 500, out.ctypes.data, None) == 0 and np.array_equal(out, eall)
        assert nctx._lib.lrge_hip_reads_name_ranks(dr.h, None, 499, out.ctypes.data, None) == -9
        assert dr.names == tn
        S = dr.seqset(q, gq)                       # the handle still serves read sets
        assert S.n == 150
        S.free(); dr.free()


def test_python_strategies_are_bit_equal():
    from lrge_amd import ava, twoset
    res = []
    for flag in (False, True):
        s = twoset.Builder().target_num_reads(300).query_num_reads(150).seed(1).device_name_ranks(flag).build(TOY)
        est, no_map = s.generate_estimates()
        res.append((est.copy(), no_map))
        assert s.name_ranks_by == ("device" if flag else "host")
    assert res[0][0].tobytes() == res[1][0].tobytes() and res[0][1] == res[1][1] and res[0][0].size == 150
    res = []
    for flag in (False, True):
        s = ava.AvaStrategy(TOY, ava.Builder().num_reads(300).seed(1), device_name_ranks=flag)
        est, no_map = s.generate_estimates()
        res.append((est.copy(), no_map))
        assert s.name_ranks_by == ("device" if flag else "host")
    assert res[0][0].tobytes() == res[1][0].tobytes() and res[0][1] == res[1][1] and res[0][0].size == 300


def run_cli(args):
    """lrge-hip --gpu-ingest with and without --gpu-names: the same stdout, exit status and messages"""
    from lrge_amd import build as Bd
    a = subprocess.run([Bd.CLI_PATH] + args + ["--gpu-ingest"], capture_output=True, text=True, timeout=300)
    b = subprocess.run([Bd.CLI_PATH] + args + ["--gpu-ingest", "--gpu-names"], capture_output=True, text=True, timeout=300)
    rest = lambda s: [ln for ln in s.splitlines() if "gpu-names" not in ln]   # noqa: E731
    assert a.returncode == b.returncode, (a.stderr, b.stderr)
    assert a.stdout == b.stdout, (a.stdout, b.stdout)
    assert rest(a.stderr) == rest(b.stderr), (a.stderr, b.stderr)
    assert "gpu-names" not in a.stderr
    return a, b


def test_cli_gpu_names(tmp_path):
    for strat in (["-T", "300", "-Q", "150"], ["-n", "300"]):
        a, b = run_cli([TOY] + strat + ["-s", "1", "-f"])
        assert a.returncode == 0 and a.stdout.strip(), a.stderr
        assert "gpu-ingest: device" in b.stderr and "gpu-names: device" in b.stderr, b.stderr
    names, seqs = toy_reads()
    # one repeated identifier in an all-vs-all run: the same error both ways
    dup = tmp_path / "dup.fa"
    dup.write_bytes(b"".join(b">%s\n%s\n" % (names[0] if i == 7 else names[i], seqs[i]) for i in range(500)))
    a, b = run_cli([str(dup), "-n", "500", "-s", "1", "-f"])
    assert a.returncode != 0 and "Duplicate read identifier" in a.stderr and "Duplicate read identifier" in b.stderr
    assert "gpu-names: device" in b.stderr
    # one identifier above the cap: the host sort takes the names, the estimate is the same
    long_ = tmp_path / "long.fa"
    long_.write_bytes(b"".join(b">%s\n%s\n" % (b"L" * 300 if i == 7 else names[i], seqs[i]) for i in range(500)))
    a, b = run_cli([str(long_), "-n", "500", "-s", "1", "-f"])
    assert a.returncode == 0 and a.stdout.strip() and "gpu-names: host" in b.stderr, b.stderr
