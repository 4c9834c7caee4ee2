"""The sampled ingest of unaligned CRAM without a GPU (lrge_amd/csrc/cram_round.h cram_sampled): the host twin
runs the four calls -- census, selected open, census with a map, mapped open -- over the walk, the stream heads and the rounds the
device runs, with a backend of the device's shape: every round is decoded into a heap block of exactly the round's raw size and
the chosen reads' ranges are copied from there to a store of exactly the chosen bases.  The reference is the host reader
(lrge_hip_read_records) on the same bytes; the mapped statistics are counted by the test from the walk."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cram_corpus as K
import cram_writer as CW
from conftest import ROOT
from test_cram_twin import STAT_KEYS, STAT_NAMES, damage_cases, load_twin
from test_gpu_ingest import read_host

CENSUS, SELECTED, CENSUS_MAP, MAPPED = 0, 1, 2, 3
OK, UNPROVEN, ORDINAL, OTHER_INPUT, MISFIT, OVER_CAP, NOT_ASCENDING = 0, 1, 2, 3, 4, 5, -2
NONE = (1 << 64) - 1


def bind(L):
    """the prototypes of the twin's sampled entries (the GPU suite binds them too)"""
    L.cram_twin_sampled.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64 * 4)]
    for f in (L.cram_twin_kept, L.cram_twin_kept_name_bytes, L.cram_twin_map_points, L.cram_twin_walk_recs, L.cram_twin_walk_slices):
        f.restype = C.c_uint64
    L.cram_twin_sampled_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64 * 4), C.POINTER(C.c_uint64 * 4)]
    L.cram_twin_sampled_stats.restype = None
    L.cram_twin_kept_table.argtypes = [C.c_void_p] * 6
    L.cram_twin_kept_table.restype = None
    L.cram_twin_map.argtypes = [C.POINTER(C.c_uint64 * 5)]
    L.cram_twin_map.restype = None
    L.cram_twin_map_points.argtypes = [C.c_void_p] * 4 + [C.c_uint64]
    L.cram_twin_walk_recs.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.cram_twin_walk_slices.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    return L


@pytest.fixture(scope="module")
def twin():
    from lrge_amd import build as B
    return bind(load_twin(B.build_cram_twin()))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """file bytes -> the host reader's [(name, bases)], computed once per file"""
    d = tmp_path_factory.mktemp("cram_select_host")
    seen = {}

    def run(data):
        if data not in seen:
            p = d / "in.cram"
            p.write_bytes(data)
            rc, rec, msg = read_host(p)
            assert rc == 0, msg
            seen[data] = rec
        return seen[data]
    return run


def sampled(L, what, data, sel=(), round_bytes=0, min_blocks=0, cap=0):
    """-> (verdict, counts [records, bases, bases, 0] or the reason) of one call of the twin"""
    a = np.ascontiguousarray(sel, dtype=np.uint32)
    out = (C.c_uint64 * 4)()
    rc = L.cram_twin_sampled(what, data, len(data), a.ctypes.data if a.size else None, a.size, round_bytes, min_blocks, cap, C.byref(out))
    return rc, (list(out) if rc == OK else L.cram_twin_why().decode())


def stats(L):
    """(cram stats, seek stats, {store bytes, largest scratch, copies, round size}) of the call that just ended"""
    st, seek, mem = (C.c_uint64 * len(STAT_NAMES))(), (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
    L.cram_twin_sampled_stats(st, C.byref(seek), C.byref(mem))
    return dict(zip(STAT_NAMES, list(st))), tuple(seek), dict(zip(("store", "scratch", "copies", "round"), list(mem)))


def kept(L, sel):
    """[(name, bases)] of the call that just ended, the store dense: read j lies directly behind read j - 1"""
    a = np.ascontiguousarray(sel, dtype=np.uint32)
    k, nb = L.cram_twin_kept(), L.cram_twin_kept_name_bytes()
    assert k == a.size
    _, _, mem = stats(L)
    lens, noff, boff = np.zeros(max(1, k), np.uint32), np.zeros(k + 1, np.uint64), np.zeros(max(1, k), np.uint64)
    names, store = C.create_string_buffer(max(1, nb)), C.create_string_buffer(max(1, mem["store"]))
    L.cram_twin_kept_table(a.ctypes.data if k else None, lens.ctypes.data, noff.ctypes.data, names, boff.ctypes.data, store)
    nm, bs = names.raw[:nb], store.raw[:mem["store"]]
    at = 0
    for j in range(k):
        assert int(boff[j]) == at
        at += int(lens[j])
    assert at == mem["store"]                                            # store bytes equal chosen bases
    return [(nm[int(noff[j]):int(noff[j + 1])], bs[int(boff[j]):int(boff[j]) + int(lens[j])]) for j in range(k)]


def walk(L):
    """(slice of every record, length of every record, compressed bytes of every slice's BA block or None, raw bytes)"""
    n = L.cram_twin_walk_recs(None, None, 0)
    sl, ln = np.zeros(max(1, n), np.uint32), np.zeros(max(1, n), np.uint32)
    L.cram_twin_walk_recs(sl.ctypes.data, ln.ctypes.data, n)
    m = L.cram_twin_walk_slices(None, None, 0)
    comp, raw = np.zeros(max(1, m), np.uint64), np.zeros(max(1, m), np.uint64)
    L.cram_twin_walk_slices(comp.ctypes.data, raw.ctypes.data, m)
    return sl[:n].tolist(), ln[:n].tolist(), [None if c == NONE else c for c in comp[:m].tolist()], raw[:m].tolist()


def map_points(L):
    out = (C.c_uint64 * 5)()
    L.cram_twin_map(C.byref(out))
    k = out[1]
    a = [np.zeros(max(1, k), np.uint64) for _ in range(4)]
    L.cram_twin_map_points(*[x.ctypes.data for x in a], k)
    return list(out), list(zip(*[x[:k].tolist() for x in a]))


def selections(rec_h, slices):
    """the selections of one file whose record i lies in slice slices[i]"""
    n = len(rec_h)
    sels = {"empty": [], "all": list(range(n))}
    if n:
        sels["first"], sels["last"] = [0], [n - 1]
        first_of = [i for i in range(n) if not i or slices[i] != slices[i - 1]]
        sels["one per slice"] = first_of
        sels["every read of one slice"] = [i for i in range(n) if slices[i] == slices[n // 2]]
        sels["every third"] = list(range(0, n, 3))
    zero = [i for i, (_, s) in enumerate(rec_h) if not s]
    if zero:
        sels["a read of length 0"] = zero[:1]
        sels["a read of length 0 and its neighbour"] = sorted({zero[0], min(n - 1, zero[0] + 1)})
    star = [i for i, (nm, _) in enumerate(rec_h) if not nm]
    if star:
        sels["a * name"] = star[:1]
    return sels


def expected_seek(sel, slices, lens, comp, raw):
    """what a mapped open of `sel` decodes, counted from the walk: the slices that hold a chosen read with bases"""
    touched = sorted({slices[i] for i in sel if lens[i]})
    assert all(comp[s] is not None for s in touched)
    runs = sum(1 for j, s in enumerate(touched) if not j or touched[j - 1] + 1 != s)
    return (runs, sum(raw[s] for s in touched), sum(comp[s] for s in touched), len(touched)), touched


@pytest.mark.parametrize("round_bytes", [1, 0])
def test_four_calls_equal_the_host_reader(twin, host, round_bytes):
    """every file of the corpus, every block a round and the default: the census counts, every selection's names, lengths and
    bases, the map's points, and the mapped open -- which decodes exactly the slices that hold a chosen read with bases"""
    n_sel = n_partial = 0
    for name, data in K.file_cases():
        rec_h = host(data)
        bases = sum(len(s) for _, s in rec_h)
        rc, out = sampled(twin, CENSUS, data, round_bytes=round_bytes)
        assert rc == OK and out == [len(rec_h), bases, bases, 0], (name, rc, out)
        assert twin.cram_twin_kept() == 0 and twin.cram_twin_kept_name_bytes() == 0       # the census keeps no identifier and no base
        st_c, seek, mem = stats(twin)
        slices, lens, comp, raw = walk(twin)
        blocks = [s for s in range(len(comp)) if comp[s] is not None]
        assert mem["store"] == 0 and seek == (0, 0, 0, 0) and lens == [len(s) for _, s in rec_h]
        assert st_c["raw_bytes"] == bases and st_c["comp_bytes"] == sum(comp[s] for s in blocks) and st_c["rounds"] == (len(blocks) if round_bytes else min(1, len(blocks))), (name, st_c)
        assert mem["scratch"] == (max([raw[s] for s in blocks], default=0) if round_bytes else bases), (name, mem)     # round scratch: the largest round
        rc, out_m = sampled(twin, CENSUS_MAP, data, round_bytes=round_bytes)
        assert rc == OK and out_m == out
        head, pts = map_points(twin)
        assert head == [len(rec_h), len(pts), len(comp), bases, len(data)], (name, head)
        first_of = [i for i in range(len(rec_h)) if not i or slices[i] != slices[i - 1]]
        assert [(o, s) for o, _, _, s in pts] == [(i, slices[i]) for i in first_of], name
        for o, off, c_off, s in pts:
            assert off == sum(raw[:s]), (name, s)
            if comp[s] is not None and comp[s]:
                assert 26 < c_off < len(data) and c_off + comp[s] <= len(data), (name, s, c_off)
        for kind, sel in selections(rec_h, slices).items():
            want = [rec_h[i] for i in sel]
            rc, out = sampled(twin, SELECTED, data, sel, round_bytes=round_bytes)
            assert rc == OK and out == out_m, (name, kind, rc, out)
            assert kept(twin, sel) == want, (name, kind)
            st, seek, mem = stats(twin)
            assert [st[k] for k in STAT_KEYS] == [st_c[k] for k in STAT_KEYS] and seek == (0, 0, 0, 0), (name, kind)     # the selected open proves the file
            assert mem["store"] == sum(len(s) for _, s in want) and mem["scratch"] <= (max(raw, default=0) if round_bytes else bases)
            assert twin.cram_twin_kept_name_bytes() == sum(len(nm) for nm, _ in want)                                     # identifiers: the sample's
            rc, out = sampled(twin, MAPPED, data, sel, round_bytes=round_bytes)
            assert rc == OK and out == out_m, (name, kind, rc, out)
            assert kept(twin, sel) == want, (name, kind, "mapped")
            st, seek, mem = stats(twin)
            want_seek, touched = expected_seek(sel, slices, lens, comp, raw)
            assert seek == want_seek, (name, kind, seek, want_seek)
            assert (st["containers"], st["slices"], st["records"]) == (st_c["containers"], st_c["slices"], st_c["records"])
            assert st["ba_raw"] + st["ba_rans4x8"] + st["ba_ransnx16"] == len(touched) and st["raw_bytes"] == want_seek[1] and st["comp_bytes"] == want_seek[2], (name, kind, st)
            assert st["rounds"] == (len(touched) if round_bytes else min(1, len(touched)))
            assert mem["scratch"] == (max([raw[s] for s in touched], default=0) if round_bytes else want_seek[1])
            n_sel += 1
            n_partial += 0 < len(touched) < len(blocks)
    assert n_sel > 200 and n_partial > 80                                # (not vacuous: many mapped opens decode some slices and not others)


def test_refusals_stay_in_step(twin, host):
    """what the walk and the stream heads refuse is refused with its reason by the census, the census with a map and the selected
    open; the mapped open finds a refused head only in a block it touches"""
    for name, data, reason in K.refused_files():
        for what in (CENSUS, CENSUS_MAP, SELECTED):
            rc, why = sampled(twin, what, data, [0] if what == SELECTED else [])
            assert rc == UNPROVEN and (reason or "compression format") in why, (name, what, why)
            assert twin.cram_twin_kept() == 0
    # as refused_files()'s gzip_ba, but in the second slice only: the method byte of that slice's BA block says gzip (the walk never
    # opens a BA block, so the file walks as before); the first slice is good
    R = K.reads(14, 3, 1, 200)
    good = CW.write_cram(R, method="gzip", records_per_slice=7, method_for={"BA": "rans0"})
    plain1 = b"".join(s for _, s in R[7:])
    blk = next(b for b in (CW.block("rans0", 4, cid, plain1) for cid in range(64)) if good.count(b) == 1)
    assert blk[0] == CW.METHODS["rans0"]
    at = good.index(blk)
    bad = good[:at] + bytes([CW.METHODS["gzip"]]) + good[at + 1:]
    rec_h = host(good)
    for what in (CENSUS, CENSUS_MAP, SELECTED):                          # the census and the selected open find a refused head in any block
        rc, why = sampled(twin, what, bad, [0] if what == SELECTED else [])
        assert rc == UNPROVEN and "a BA block in gzip" in why, (what, why)
    assert sampled(twin, CENSUS_MAP, good)[0] == OK                      # (the same length, records, bases and slices: the map fits either file)
    rc, out = sampled(twin, MAPPED, bad, [0, 3])                         # slice 0 only: the bad block is not touched
    assert rc == OK and kept(twin, [0, 3]) == [rec_h[0], rec_h[3]]
    rc, why = sampled(twin, MAPPED, bad, [0, 9])                         # slice 1 is touched
    assert rc == UNPROVEN and "a BA block in gzip" in why and twin.cram_twin_kept() == 0, why
    # CRAM_MIN_BLOCKS is tested against the file's BA blocks in all four calls
    for what in (CENSUS, CENSUS_MAP, SELECTED, MAPPED):
        if what == MAPPED:
            assert sampled(twin, CENSUS_MAP, good)[0] == OK              # (a refused census leaves no map)
        rc, why = sampled(twin, what, good, [0] if what in (SELECTED, MAPPED) else [], min_blocks=3)
        assert rc == UNPROVEN and "fewer BA blocks than CRAM_MIN_BLOCKS" in why, (what, why)
    assert sampled(twin, MAPPED, good, [0], min_blocks=2)[0] == OK


def test_maps_of_other_files_and_bad_selections(twin, host):
    data, other = K.by_name("ba_rans1"), K.by_name("ba_rans0")
    n = len(host(data))
    assert sampled(twin, CENSUS_MAP, data)[0] == OK
    assert sampled(twin, MAPPED, other, [0])[0] == OTHER_INPUT           # another file length
    assert sampled(twin, MAPPED, data + b"\0", [0])[0] == OTHER_INPUT
    # the same length and counts, other slices: 23 reads at 7 a slice against the same at 6 and 8 a slice is another length; the
    # same bytes with one read moved between slices cannot be written, so the points are compared on a map of the twin's own
    assert sampled(twin, MAPPED, data, [0, n - 1])[0] == OK
    for sel in ([n], [0, n - 1, n]):
        assert sampled(twin, SELECTED, data, sel)[0] == ORDINAL and sampled(twin, MAPPED, data, sel)[0] == ORDINAL, sel
    for sel in ([5, 3], [0, 4, 4, 9]):
        assert sampled(twin, SELECTED, data, sel)[0] == NOT_ASCENDING and sampled(twin, MAPPED, data, sel)[0] == NOT_ASCENDING, sel
    assert twin.cram_twin_kept() == 0
    # an empty file: an empty census, an empty map, empty handles
    empty = K.by_name("empty")
    assert sampled(twin, CENSUS_MAP, empty) == (OK, [0, 0, 0, 0]) and map_points(twin)[1] == []
    assert sampled(twin, SELECTED, empty, []) == (OK, [0, 0, 0, 0]) and sampled(twin, MAPPED, empty, []) == (OK, [0, 0, 0, 0])
    assert sampled(twin, SELECTED, empty, [0])[0] == ORDINAL


def test_damage_is_a_status_or_the_host_readers_bytes(twin, tmp_path):
    """a flipped byte in a BA body: the census and the selected open refuse, or the kept reads are the host reader's"""
    refused = same = 0
    for name, data in damage_cases()[::2]:
        p = tmp_path / "damaged.cram"
        p.write_bytes(data)
        rc_h, rec_h, _ = read_host(p)
        rc_c, _ = sampled(twin, CENSUS, data)
        sel = [0, 4, 8]
        rc, _ = sampled(twin, SELECTED, data, sel)
        assert rc == rc_c, name                                          # the census proves what the selected open proves
        if rc:
            refused += 1
            assert twin.cram_twin_kept() == 0
            continue
        assert rc_h == 0 and kept(twin, sel) == [rec_h[i] for i in sel], name     # never different bytes
        same += 1
    assert refused >= 10 and same >= 1, (refused, same)


def test_budget(twin, host):
    """INGEST_MAX_BYTES bounds the chosen bases plus the largest round: at the file's bases -- where the full open is refused -- two
    reads fit, because the rounds shrink until one fits; below chosen bases plus the largest single block nothing does"""
    data = K.by_name("ba_rans1")
    rec_h = host(data)
    bases = sum(len(s) for _, s in rec_h)
    sel = [2, 17]
    chosen = sum(len(rec_h[i][1]) for i in sel)
    assert sampled(twin, CENSUS, data)[0] == OK
    slices, lens, comp, raw = walk(twin)
    pad = lambda c: (c + 3) & ~3   # noqa: E731  (a block's compressed bytes go up padded to words)
    block = max(pad(c) + r for c, r in zip(comp, raw))                    # the largest single block, compressed and raw
    assert chosen + block <= bases < bases + sum(comp)                   # (the full open needs the bases and a round: refused at this cap)
    for what in (SELECTED, MAPPED):
        if what == MAPPED:
            assert sampled(twin, CENSUS_MAP, data)[0] == OK
        rc, out = sampled(twin, what, data, sel, cap=bases)
        assert rc == OK and kept(twin, sel) == [rec_h[i] for i in sel], (what, rc, out)
        st, seek, mem = stats(twin)
        assert mem["store"] == chosen and mem["store"] + mem["scratch"] + max(pad(c) for c in comp) <= bases, (what, mem, st)
        assert what == MAPPED or st["rounds"] > 1                        # (every block in one round would not fit: the rounds shrank)
        touched_block = max(pad(comp[s]) + raw[s] for s in ({slices[i] for i in sel} if what == MAPPED else range(len(comp))))
        assert sampled(twin, what, data, sel, cap=chosen + touched_block)[0] == OK
        assert sampled(twin, what, data, sel, cap=chosen + touched_block - 1)[0] == OVER_CAP, what
        assert twin.cram_twin_kept() == 0
    assert sampled(twin, CENSUS, data, cap=block)[0] == OK and sampled(twin, CENSUS, data, cap=block - 1)[0] == OVER_CAP


def test_abi_has_both_flags():
    from lrge_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "lrge_hip.h")).read()
    shim = open(os.path.join(ROOT, "integration", "liblrge_hip_shim.rs")).read()
    for name, bit in (("SELECT_SAM", 4096), ("SELECT_CRAM", 8192)):
        assert re.search(r"#define\s+LRGE_GPU_INGEST_%s\s+%d\b" % (name, bit), hdr) and getattr(_ffi, "GPU_INGEST_" + name) == bit
        assert re.search(r"LRGE_GPU_INGEST_%s: c_int = %d;" % (name, bit), shim)
        assert "LRGE_GPU_INGEST_" + name in open(os.path.join(ROOT, "include", "lrge_hip.hpp")).read()
        assert "LRGE_GPU_INGEST_" + name in open(os.path.join(ROOT, "tools", "lrge_hip_cli.cpp")).read()
    flags = [v for k, v in vars(_ffi).items() if k.startswith(("GPU_INGEST_", "GPU_INFLATE_")) and isinstance(v, int)]
    assert len(flags) == len(set(flags)) and all(v & (v - 1) == 0 for v in flags)         # one bit each, none shared
