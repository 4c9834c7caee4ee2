"""The PAF writer's rules on the CPU: lrge_amd/csrc/paf_twin.cpp -- the measure, scan and write steps of the
device path as loops over csrc/paf_core.h -- against lrge_amd/paf.py, byte for byte; the dv code against Python's "%.4f"; the
proof of a p; the near miss (round-half-up) that the tie cases must catch; and tools/paf_check.cpp, the same cases from heap blocks
of exact size under AddressSanitizer and UBSan in a stand-alone program."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

I32_MIN, I32_MAX, U32_MAX = -2 ** 31, 2 ** 31 - 1, 2 ** 32 - 1
F32_EPS = np.float32(np.finfo(np.float32).eps)


def load_twin():
    from lrge_amd import build as Bd
    L = C.CDLL(Bd.build_paf_twin())
    vp = C.c_void_p
    L.paf_twin_format.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp, C.c_char_p, vp, C.c_char_p, vp, vp, vp, vp, C.c_uint64, vp, C.c_uint64,
                                  C.POINTER(C.c_uint64), vp, C.c_uint64, C.POINTER(C.c_uint64), vp]
    L.paf_twin_dv_code.argtypes = [C.c_float, C.c_int]
    L.paf_twin_dv_code.restype = C.c_uint32
    L.paf_twin_dv_text.argtypes = [C.c_uint32, C.c_char_p]
    L.paf_twin_dv_text.restype = C.c_uint32
    L.paf_twin_p_unproven.argtypes = [C.c_double, C.c_double]
    L.paf_twin_pow_ulps.restype = C.c_double
    L.paf_twin_code_of_p.argtypes = [C.c_double]
    L.paf_twin_code_of_p.restype = C.c_uint32
    L.paf_twin_fixed_bound.restype = C.c_uint32
    return L


@pytest.fixture(scope="module")
def twin():
    return load_twin()


def table(names):
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum([len(n) for n in names], out=off[1:])
    return b"".join(names), off


# ------------------------------------------------------------------------------------------
# dv code
# ------------------------------------------------------------------------------------------
def dv_text(L, x, half_up=0):
    buf = C.create_string_buffer(16)
    n = L.paf_twin_dv_text(L.paf_twin_dv_code(float(np.float32(x)), half_up), buf)
    return buf.raw[:n].decode()


def dv_model(x):
    x = np.float32(x)
    return "0" if float(x) < float(F32_EPS) else "%.4f" % float(x)


def neighbours(x):
    x = np.float32(x)
    return [np.nextafter(x, np.float32(-2)), x, np.nextafter(x, np.float32(2))]


TIES = [0.03125, 0.09375, 0.15625]      # k / 32: 312.5, 937.5 and 1562.5 steps of 1e-4, exact in binary


def dv_cases():
    xs = neighbours(F32_EPS) + neighbours(np.float32(0.99995)) + [np.float32(-1.0), np.float32(0.0)]
    for t in TIES:
        xs += neighbours(t)
    rng = np.random.Generator(np.random.PCG64(31))
    xs += list(rng.random(100_000, dtype=np.float32))
    xs += list(np.exp2(rng.uniform(-23.0, -10.0, 10_000)).astype(np.float32))
    return xs


def test_dv_code_is_percent_4f(twin):
    xs = dv_cases()
    assert all(0.0 <= float(x) < 1.0 for x in xs[-110_000:]) and all(2.0 ** -23 <= float(x) <= 2.0 ** -10 for x in xs[-10_000:])
    bad = [(float(x), dv_text(twin, x), dv_model(x)) for x in xs if dv_text(twin, x) != dv_model(x)]
    assert not bad, bad[:5]
    assert dv_text(twin, F32_EPS) == "0.0000" and dv_text(twin, np.nextafter(F32_EPS, np.float32(0))) == "0"
    # the float nearest to 0.99995 lies below it (0.99994999...) and prints 0.9999, as "%.4f" has it; its upper neighbour is the
    # first float that prints 1.0000
    lo, at, hi = neighbours(np.float32(0.99995))
    assert [dv_text(twin, x) for x in (lo, at, hi)] == ["0.9999", "0.9999", "1.0000"] and float(at) < 0.99995 < float(hi)
    assert dv_text(twin, 1.0) == "1.0000" and dv_text(twin, -1.0) == "0"
    assert [dv_text(twin, t) for t in TIES] == ["0.0312", "0.0938", "0.1562"]


def test_round_half_up_fails_the_ties(twin):
    """The near miss: with round-half-up in place of ties-to-even the tie cases differ from "%.4f", so they can tell the two apart;
    off the ties both roundings agree."""
    assert [dv_text(twin, t, half_up=1) for t in TIES] == ["0.0313", "0.0938", "0.1563"]
    assert [dv_text(twin, t, half_up=1) != dv_model(t) for t in TIES] == [True, False, True]
    for t in TIES:
        lo, _, hi = neighbours(t)
        assert dv_text(twin, lo, half_up=1) == dv_model(lo) and dv_text(twin, hi, half_up=1) == dv_model(hi)


# ------------------------------------------------------------------------------------------
# the proof of a p
# ------------------------------------------------------------------------------------------
def test_proof_flags_a_window_over_a_code_boundary(twin):
    W = twin.paf_twin_pow_ulps()
    assert W == 5.0      # glibc's 1 ulp (manual, x86_64) + the 4 assumed for the device library
    for lo, hi in [(0.9, 0.95), (0.5, 0.6), (0.99, 0.999), (1e-3, 2e-3)]:
        assert twin.paf_twin_code_of_p(lo) != twin.paf_twin_code_of_p(hi)
        while math.nextafter(lo, 2.0) < hi:      # two adjacent doubles with different codes
            mid = 0.5 * (lo + hi)
            if twin.paf_twin_code_of_p(mid) == twin.paf_twin_code_of_p(lo):
                lo = mid
            else:
                hi = mid
        assert twin.paf_twin_code_of_p(lo) != twin.paf_twin_code_of_p(hi)
        for p in (lo, hi):
            assert twin.paf_twin_p_unproven(p, W) == 1
            far = 100.0 * W * math.ulp(p)
            assert twin.paf_twin_p_unproven(p + far, W) == 0 and twin.paf_twin_p_unproven(p - far, W) == 0
    assert twin.paf_twin_p_unproven(float("nan"), W) == 1


# ------------------------------------------------------------------------------------------
# the whole formatter
# ------------------------------------------------------------------------------------------
class Case:
    """Synthetic records over small read sets: everything paf.paf_lines and the twin read."""

    def __init__(self, q_names, q_lens, t_names, t_lens, rl, ss, nk, recs):
        from lrge_amd import _ffi
        self.q_names, self.t_names = q_names, t_names
        self.q_lens, self.t_lens = np.array(q_lens, dtype=np.uint32), np.array(t_lens, dtype=np.uint32)
        self.rl, self.ss, self.nk = np.array(rl, dtype=np.int32), np.array(ss, dtype=np.uint64), np.array(nk, dtype=np.uint32)
        self.recs = np.zeros(len(recs), dtype=_ffi.CHAIN)
        for i, r in enumerate(recs):
            for k, v in r.items():
                self.recs[i][k] = v

    def expected(self):
        from lrge_amd import paf
        lines = paf.paf_lines(self.recs, self.q_names, self.q_lens, self.t_names, self.t_lens, self.rl, self.ss, self.nk)
        return [(l + "\n").encode() for l in lines]


def run_twin(L, c, piece):
    qb, qo = table(c.q_names)
    tb, to = table(c.t_names)
    n = len(c.recs)
    need, ns = C.c_uint64(), C.c_uint64()
    st = np.zeros(4, dtype=np.uint64)
    ends = np.zeros(max(n, 1), dtype=np.uint64)
    recs = np.ascontiguousarray(c.recs)
    args = [recs.ctypes.data, n, len(c.q_names), len(c.t_names), c.q_lens.ctypes.data, c.t_lens.ctypes.data, qb, qo.ctypes.data, tb, to.ctypes.data,
            c.rl.ctypes.data, c.ss.ctypes.data, c.nk.ctypes.data, piece]
    rc = L.paf_twin_format(*args, None, 0, C.byref(need), ends.ctypes.data, 0, C.byref(ns), st.ctypes.data)      # the size alone
    if rc:
        return rc, b"", [], st
    out = C.create_string_buffer(max(1, need.value))
    rc = L.paf_twin_format(*args, out, need.value, C.byref(need), ends.ctypes.data, len(ends), C.byref(ns), st.ctypes.data)
    return rc, out.raw[:need.value], [int(e) for e in ends[:ns.value]], st


def rec(query=0, target=0, rev=0, score=100, cnt=5, qs=10, qe=900, rs=20, re=910, mlen=400, blen=890, n_seeds=9):
    return dict(query=query, target=target, rev=rev, score=score, cnt=cnt, qs=qs, qe=qe, rs=rs, re=re, mlen=mlen, blen=blen, n_seeds=n_seeds)


def synthetic_case():
    name_lens = [1, 63, 64, 65, 128, 1024]
    q_names = [bytes([ord("a") + (i + j) % 26 for j in range(l)]) for i, l in enumerate(name_lens)] + [b"q_nokept", b"q_k15"]
    t_names = [bytes([ord("A") + (i + 2 * j) % 26 for j in range(l)]) for i, l in enumerate(reversed(name_lens))] + [b"t6", b"t_k15"]
    widths = [10 ** (w - 1) for w in range(1, 11)]                       # 1, 10, ..., 10^9: widths 1 to 10
    q_lens = [1000, 9, 99, 1234567, U32_MAX, 2 ** 31, 40000, 1000]
    t_lens = [2000, 10 ** 9, 7, 65536, U32_MAX - 1, 12, 50000, 1000]
    NOKEPT, K15 = len(q_names) - 2, len(q_names) - 1
    rl = [0, 7, -3, I32_MAX, I32_MIN, 123456, 99, 15]
    ss = [1500, 19 * 7, 1, 15 * 10 ** 6, 300, 2 ** 40, 0, 150]           # avg_k: 15, 19, 1, 15, 15, 2^40 / 3, -, 15
    nk = [100, 7, 1, 10 ** 6, 20, 3, 0, 10]
    # the two read lengths (the only u32 fields) and rl at every width: reads of 10^0 .. 10^9 and 2^32 - 1 bases in both sets, and
    # queries whose rl is +10^0 .. +10^9, INT32_MAX, then -10^0 .. -10^9, INT32_MIN
    W0_Q, W0_T = len(q_names), len(t_names)
    width_lens = widths + [U32_MAX]
    for j in range(22):
        q_names.append(b"qw%d_" % j + b"x" * (j % 7))
        q_lens.append(width_lens[j % 11])
        mag = widths[j % 11] if j % 11 < 10 else (I32_MAX if j < 11 else -I32_MIN)
        rl.append(mag if j < 11 else -mag)
        ss.append([1500, 133, 15 * 10 ** 6][j % 3]); nk.append([100, 7, 10 ** 6][j % 3])
    for j in range(11):
        t_names.append(b"tw%d" % j)
        t_lens.append(width_lens[10 - j])
    nt = len(t_names)
    recs = []
    for j in range(22):
        for k in range(11):
            recs.append(rec(query=W0_Q + j, target=W0_T + k, rev=(j + k) & 1, cnt=5 + k, n_seeds=9 + j))
    ifields = ["score", "qs", "qe", "rs", "re", "mlen", "blen"]
    for i, v in enumerate(widths):                                        # every integer field at every width, both signs
        vi = min(v, I32_MAX)
        for f in ifields:
            recs.append(rec(query=i % 6, target=(i + 1) % 6, rev=i & 1, **{f: vi}))
            recs.append(rec(query=(i + 2) % 6, target=i % 6, rev=(i + 1) & 1, **{f: -vi}))
        recs.append(rec(query=i % 6, target=i % 6, cnt=vi, n_seeds=min(vi + 3, I32_MAX)))       # cm at every width, dv > 0
        recs.append(rec(query=i % 6, target=i % 6, cnt=3, n_seeds=vi + 3 if vi + 3 <= I32_MAX else I32_MAX))
    for f in ifields:                                                     # INT32_MIN and INT32_MAX
        recs.append(rec(query=1, target=2, **{f: I32_MIN}))
        recs.append(rec(query=3, target=4, rev=1, **{f: I32_MAX}))
    recs.append(rec(query=2, target=2, cnt=I32_MAX, n_seeds=5))           # cnt >= n_tot: dv 0
    recs.append(rec(query=2, target=2, cnt=3, n_seeds=I32_MAX))           # n_tot above int32 once the corrections are added
    recs.append(rec(query=NOKEPT, target=6, cnt=I32_MIN, n_seeds=I32_MIN))   # n_kept == 0: dv -1 whatever the record says
    recs.append(rec(query=NOKEPT, target=6, cnt=-7, n_seeds=I32_MAX, rev=1))
    for c, ns in [(9, 9), (10, 9), (9, 10), (1, 2), (0, 4), (3, 3000), (2999, 3000), (29999, 30000)]:
        recs.append(rec(query=0, target=0, cnt=c, n_seeds=ns))
    # both end corrections on and off at the avg_k border (15), reads of 1000 bases: qs and rs at 15 (not above) and 16 (above),
    # qlen - qs and tlen - re at 15 and 16 (qs, re at 985 and 984); cnt = n_seeds, so a correction that fires turns dv from 0 into
    # something positive, and two of them into something larger
    for qs in (15, 16, 984, 985):
        for rs in (15, 16):
            for re in (984, 985):
                recs.append(rec(query=K15, target=7, cnt=20, n_seeds=20, qs=qs, rs=rs, re=re, rev=qs & 1))
    rng = np.random.Generator(np.random.PCG64(7))
    for _ in range(200):
        ns = int(rng.integers(3, 5000))
        recs.append(rec(query=int(rng.integers(0, 6)), target=int(rng.integers(0, nt)), rev=int(rng.integers(0, 2)), score=int(rng.integers(0, 10 ** 6)),
                        cnt=int(rng.integers(1, ns + 1)), qs=int(rng.integers(0, 5000)), qe=int(rng.integers(0, 10 ** 5)), rs=int(rng.integers(0, 5000)),
                        re=int(rng.integers(0, 10 ** 5)), mlen=int(rng.integers(0, 10 ** 5)), blen=int(rng.integers(0, 10 ** 5)), n_seeds=ns))
    return Case(q_names, q_lens, t_names, t_lens, rl, ss, nk, recs)


@pytest.fixture(scope="module")
def case():
    return synthetic_case()


def test_formatter_equals_paf_lines(twin, case):
    exp = case.expected()
    text = b"".join(exp)
    assert len(exp) > 400
    # what the cases are there for is there: both strands, "dv:f:0" beside other divergences, a 10-digit length, INT32_MIN, a 1024-byte name
    assert any(b"\t-\t" in l for l in exp) and any(b"\t+\t" in l for l in exp)
    assert any(l.split(b"\t")[15] == b"dv:f:0" for l in exp) and any(l.split(b"\t")[15].startswith(b"dv:f:0.") for l in exp)
    assert any(l.split(b"\t")[15] == b"dv:f:1.0000" for l in exp)
    assert any(b"\t4294967295\t" in l for l in exp) and any(b"\t-2147483648\t" in l for l in exp) and any(b"rl:i:-2147483648\n" in l for l in exp)
    assert max(len(l.split(b"\t")[0]) for l in exp) == 1024 and max(len(l.split(b"\t")[5]) for l in exp) == 1024
    # the two u32 fields and rl were there at every width, rl under both signs
    assert {len(l.split(b"\t")[1]) for l in exp} == set(range(1, 11)) == {len(l.split(b"\t")[6]) for l in exp}
    rls = [l.split(b"\t")[16][5:-1] for l in exp]
    assert {len(r) for r in rls if not r.startswith(b"-")} == set(range(1, 11)) == {len(r) - 1 for r in rls if r.startswith(b"-")}
    # the end corrections both fire and stay off in the avg_k = 15 block
    k15 = [l.split(b"\t")[15] for l in exp if l.startswith(b"q_k15\t")]
    assert len(k15) == 16 and b"dv:f:0" in k15 and len(set(k15)) >= 3
    bound = 1024 + 1024 + twin.paf_twin_fixed_bound()
    assert twin.paf_twin_fixed_bound() == 170 and max(len(l) for l in exp) <= bound
    # all lines one slice; a few lines a slice; one line a slice
    for piece, n_slices in [(1 << 30, 1), (4 * bound, None), (1, len(exp))]:
        rc, got, ends, st = run_twin(twin, case, piece)
        assert rc == 0 and int(st[0]) == 0 and int(st[3]) == len(exp)
        assert got == text, "first differing line: %r" % next(((a, b) for a, b in zip(got.split(b"\n"), text.split(b"\n")) if a != b), None)
        assert n_slices is None or len(ends) == n_slices
        assert ends[-1] == len(text) and all(got[e - 1:e] == b"\n" for e in ends) and all(b - a <= max(piece, bound) for a, b in zip([0] + ends, ends))
        if piece == 4 * bound:
            assert len(ends) == -(-len(exp) // 4)
    assert [len(l) for l in exp] == np.diff([0] + run_twin(twin, case, 1)[2]).tolist()


def test_formatter_refusals(twin, case):
    from lrge_amd import _ffi
    import copy
    c = copy.copy(case)
    c.recs = case.recs[:3].copy()
    c.recs[1]["target"] = len(case.t_names)
    assert run_twin(twin, c, 1 << 20)[0] == _ffi.ERR_INVALID
    c.recs = case.recs[:0].copy()
    assert run_twin(twin, c, 1 << 20)[:3] == (0, b"", [])


# ------------------------------------------------------------------------------------------
# the same under the host sanitizers, as a program of its own
# ------------------------------------------------------------------------------------------
def case_blob(c, piece):
    qb, qo = table(c.q_names)
    tb, to = table(c.t_names)
    text = b"".join(c.expected())
    head = struct.pack("<QIIQQQQ", len(c.recs), len(c.q_names), len(c.t_names), piece, len(qb), len(tb), len(text))
    return b"".join([head, np.ascontiguousarray(c.recs).tobytes(), c.q_lens.tobytes(), c.t_lens.tobytes(), qo.tobytes(), to.tobytes(), qb, tb,
                     c.rl.tobytes(), c.ss.tobytes(), c.nk.tobytes(), text])


def test_sanitized_standalone_program(tmp_path, case):
    """tools/paf_check.cpp: the formatter cases above (written to a file, every array handed over in a heap block of its exact size)
    and the dv cases (generated inside the program, against printf), built with AddressSanitizer and UBSan as a program of its own."""
    exe = str(tmp_path / "paf_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "lrge_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "paf_check.cpp")])
    bound = 2048 + 170
    cases = [case_blob(case, p) for p in (1 << 30, 4 * bound, 1)]
    path = tmp_path / "cases.bin"
    path.write_bytes(b"PAFC" + struct.pack("<I", len(cases)) + b"".join(cases))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "paf_check: ok" in r.stdout
