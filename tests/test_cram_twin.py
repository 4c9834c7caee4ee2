"""CPU: the host twin of the CRAM device ingest (lrge_amd/csrc/cram_twin.cpp: the walk, the stream heads, the rounds and the block
decode the device runs) against the writer's plain bytes and against the host reader (lrge_hip_read_records), every refusal by its
reason, single-byte damage, the header pins.  tests/test_gpu_cram.py holds the device to the same cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cram_corpus as K
import cram_writer as CW
from conftest import ROOT
from test_gpu_ingest import read_host

STAT_KEYS = ["containers", "slices", "records", "ba_raw", "ba_rans4x8", "ba_ransnx16", "order1_blocks", "global_table_blocks", "comp_bytes", "raw_bytes", "rounds"]
STAT_NAMES = STAT_KEYS + ["walk_us", "decode_us"]
STATUS = {"ok": 0, "exhausted": 1, "state": 2, "end": 3, "no_table": 4, "runs": 5, "head": 16}


class Stream(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("length", C.c_uint32), ("raw_size", C.c_uint32), ("method", C.c_uint32), ("status", C.c_uint32)]


def load_twin(path):
    L = C.CDLL(path)
    L.cram_twin_why.restype = C.c_char_p
    L.cram_twin_rans_decode.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(Stream), C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    L.cram_twin_open.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    for f in (L.cram_twin_count, L.cram_twin_name_bytes, L.cram_twin_base_bytes):
        f.restype = C.c_uint64
    L.cram_twin_table.argtypes = [C.c_void_p] * 5
    L.cram_twin_table.restype = None
    return L


@pytest.fixture(scope="module")
def twin():
    from lrge_amd import build as B
    return load_twin(B.build_cram_twin())


def pack_streams(items):
    """items: [(method, bytes, raw size)] -> (the bytes back to back, Stream array)"""
    comp, arr = bytearray(), (Stream * max(1, len(items)))()
    for i, (method, body, raw) in enumerate(items):
        arr[i] = Stream(len(comp), len(body), raw, method, 0xFFFF)
        comp += body
    return bytes(comp), arr


def twin_decode(L, items, round_bytes=0):
    """-> (output bytes, [status], stats dict, first refusal text)"""
    comp, arr = pack_streams(items)
    total = sum(r for _, _, r in items)
    out = C.create_string_buffer(max(1, total))
    st = (C.c_uint64 * len(STAT_NAMES))()
    assert L.cram_twin_rans_decode(comp, len(comp), arr, len(items), out, total, round_bytes, st) == 0
    return out.raw[:total], [arr[i].status for i in range(len(items))], dict(zip(STAT_NAMES, list(st))), L.cram_twin_why().decode()


def twin_open(L, data, round_bytes=0, min_blocks=0):
    """-> (0, records [(name, bases)], stats) or (1, reason, None)"""
    st = (C.c_uint64 * len(STAT_NAMES))()
    if L.cram_twin_open(data, len(data), round_bytes, min_blocks, st):
        return 1, L.cram_twin_why().decode(), None
    n, nb, bb = L.cram_twin_count(), L.cram_twin_name_bytes(), L.cram_twin_base_bytes()
    lens, noff, boff = np.zeros(max(1, n), np.uint32), np.zeros(n + 1, np.uint64), np.zeros(max(1, n), np.uint64)
    names, bases = C.create_string_buffer(max(1, nb)), C.create_string_buffer(max(1, bb))
    L.cram_twin_table(lens.ctypes.data, noff.ctypes.data, names, boff.ctypes.data, bases)
    nm, bs = names.raw[:nb], bases.raw[:bb]
    recs = [(nm[int(noff[i]):int(noff[i + 1])], bs[int(boff[i]):int(boff[i]) + int(lens[i])]) for i in range(n)]
    return 0, recs, dict(zip(STAT_NAMES, list(st)))


def test_streams_equal_the_writers_plain_bytes(twin):
    cases = K.stream_cases()
    names = {c[0] for c in cases}
    assert len(cases) > 500 and {"rans1_n3_a4", "nx16_o1x32_n31_a4", "nx16_o1x32_n33_a5", "nx16_o1_n4097_a256", "nx16_packrle_n70001_a4", "rans0_freq1"} <= names
    items = [(m, comp, len(plain)) for _, m, comp, plain in cases]
    out, status, st, why = twin_decode(twin, items)                      # one batch of all
    assert status == [0] * len(cases), [(cases[i][0], s) for i, s in enumerate(status) if s][:5] + [why]
    o = 0
    for name, _, _, plain in cases:
        assert out[o:o + len(plain)] == plain, name
        o += len(plain)
    assert st["rounds"] == 1 and st["ba_raw"] == 2 and st["ba_rans4x8"] + st["ba_ransnx16"] == len(cases) - 2
    assert st["global_table_blocks"] >= 3 and st["order1_blocks"] > 100 and st["raw_bytes"] == len(out)
    for name, m, comp, plain in cases[::7]:                              # one block a call
        out1, status1, st1, _ = twin_decode(twin, [(m, comp, len(plain))])
        assert status1 == [0] and out1 == plain and st1["rounds"] == 1, name
    out2, status2, st2, _ = twin_decode(twin, items[:40], round_bytes=1)  # every block a round of its own
    assert status2 == [0] * 40 and st2["rounds"] == 40 and out2 == b"".join(c[3] for c in cases[:40])


def test_refused_stream_heads_name_their_reason(twin):
    good = K.stream_cases()[100]
    for name, method, body, raw, reason in K.refused_streams():
        out, status, st, why = twin_decode(twin, [(good[1], good[2], len(good[3])), (method, body, raw), (good[1], good[2], len(good[3]))])
        assert status == [0, STATUS["head"], 0] and reason in why, (name, status, why)
        assert out[:len(good[3])] == good[3] and out[len(good[3]) + raw:] == good[3], name
    short, plain = K.short_table_stream()
    assert len(short) == len(CW.rans4x8(plain, 0))


def test_walker_gives_the_host_readers_records(twin, tmp_path):
    files = K.file_cases()
    assert len(files) >= 30
    for name, data in files:
        p = tmp_path / (name + ".cram")
        p.write_bytes(data)
        rc_h, rec_h, msg = read_host(p)
        assert rc_h == 0, (name, msg)
        for round_bytes in (0, 1):
            rc, rec, st = twin_open(twin, data, round_bytes)
            assert rc == 0, (name, rec)
            assert rec == rec_h, name
            blocks = st["ba_raw"] + st["ba_rans4x8"] + st["ba_ransnx16"]
            assert st["records"] == len(rec_h) and st["raw_bytes"] == sum(len(s) for _, s in rec_h) and st["rounds"] == (blocks if round_bytes else min(1, blocks)), (name, st)
    rc, rec, st = twin_open(twin, K.by_name("external_stop_q1_t1_spc3"))
    assert (st["containers"], st["slices"], st["ba_rans4x8"], st["order1_blocks"]) == (2, 4, 4, 4) and b"" in [n for n, _ in rec] and b"" in [s for _, s in rec], st
    rc, rec, st = twin_open(twin, K.by_name("empty"))
    assert rc == 0 and rec == [] and st["slices"] <= 1
    rc, why, _ = twin_open(twin, K.by_name("ba_rans0"), min_blocks=5)
    assert rc == 1 and "fewer BA blocks than CRAM_MIN_BLOCKS" in why


def test_every_unproven_reason_by_name(twin, tmp_path):
    cases = K.refused_files()
    assert {"stripe_ba", "gzip_ba", "mapped", "shared_ba_id", "lengths_do_not_add_up", "short_table"} <= {c[0] for c in cases}
    for name, data, reason in cases:
        rc, why, _ = twin_open(twin, data)
        assert rc == 1 and (reason or "compression format") in why, (name, why)
        if name in ("stripe_ba", "gzip_ba", "shared_ba_id", "short_table"):       # the host reader takes these
            p = tmp_path / (name + ".cram")
            p.write_bytes(data)
            assert read_host(p)[0] == 0, name


def damage_cases():
    """(name, damaged file): fixed single-byte flips inside the BA body of one-slice files"""
    out = []
    for method in ("rans0", "rans1", "nx16_o0", "nx16_o1", "nx16_packrle", "nx16_rle_cm", "nx16_cat"):
        R = K.reads(9, 17, 40, 300)
        data = CW.write_cram(R, method="raw", minor=1, method_for={"BA": method})
        a, e = K.ba_body_span(data, b"".join(s for _, s in R), method)
        for k, bit in ((1, 1), (9, 0x40), (12, 1), (20, 0x80), (33, 2), ((e - a) // 2, 4), (e - a - 30, 1), (e - a - 9, 0x10), (e - a - 2, 1), (e - a - 1, 0x80)):
            at = a + k
            out.append(("%s_%d_%x" % (method, k, bit), data[:at] + bytes([data[at] ^ bit]) + data[at + 1:]))
    return out


def test_damage_is_a_status_or_the_host_readers_bytes(twin, tmp_path):
    refused = same = 0
    for name, data in damage_cases():
        p = tmp_path / "damaged.cram"
        p.write_bytes(data)
        rc_h, rec_h, _ = read_host(p)
        rc, rec, _ = twin_open(twin, data)
        if rc:
            refused += 1
            continue
        assert rc_h == 0 and rec == rec_h, name                          # never different bytes
        same += 1
    assert refused >= 20 and same >= 3, (refused, same)


def test_header_pins():
    from lrge_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "lrge_hip.h")).read()
    shim = open(os.path.join(ROOT, "integration", "liblrge_hip_shim.rs")).read()
    assert re.search(r"#define\s+LRGE_GPU_INGEST_CRAM\s+512\b", hdr) and _ffi.GPU_INGEST_CRAM == 512
    assert re.search(r"pub const LRGE_GPU_INGEST_CRAM: c_int = 512;", shim)
    assert {"lrge_hip_rans_decode", "lrge_hip_reads_cram_stats"} <= set(_ffi.EXPORTS)
    assert "fn lrge_hip_rans_decode" in shim and "fn lrge_hip_reads_cram_stats" in shim
    m = re.search(r"typedef struct lrge_hip_cram_stats \{(.*?)\}", hdr, flags=re.S)
    assert re.findall(r"uint64_t\s+([a-z_0-9]+);", m.group(1)) == _ffi.CRAM_STAT_NAMES == STAT_NAMES


def test_sanitizer_program(tmp_path):
    """tools/cram_check.cpp, a stand-alone program with its own main: the twin and the walker over the corpus dumped to files, built
    with AddressSanitizer and UBSan and run here (nothing loaded into Python is run under a sanitizer)"""
    exe = tmp_path / "cram_check"
    src = os.path.join(ROOT, "tools", "cram_check.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), src, "-lz", "-ldl"])
    d = tmp_path / "corpus"
    d.mkdir()
    cases = K.stream_cases()
    pick = [c for c in cases if c[0].endswith(("_n0_a4", "_n3_a4", "_n33_a5", "_n4097_a17", "_n4097_a256")) or "long_runs" in c[0] or "symbols" in c[0] or "freq1" in c[0]]
    for name, m, comp, plain in pick:
        (d / ("s_%d_%s.in" % (m, name))).write_bytes(comp)
        (d / ("s_%d_%s.out" % (m, name))).write_bytes(plain)
    for name, data in K.file_cases()[::3] + [(n, f) for n, f, _ in K.refused_files()] + damage_cases()[::2]:
        (d / ("f_%s.cram" % name)).write_bytes(data)
    r = subprocess.run([str(exe), str(d)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "streams ok" in r.stdout and "files walked" in r.stdout
