"""The sliding mode of the block-parallel Zstandard decode without a GPU: the host twin
(lrge_amd/csrc/zs_twin.cpp) run with a work text [history | round] per round -- a heap block of exactly that size -- instead of the
whole text, against libzstd and against the twin that keeps the whole text; the memory claim as conditions on the run's
statistics; frames written by hand at the edges of the history rule; XXH64 taken in parts (zs_xxh64_part); the sanitizer
program tools/zstd_slide_check.cpp.  The largest text is 600 KB."""
import ctypes as C
import os
import random
import struct
import subprocess

import pytest

import zstd_corpus as Z
import zstd_writer as ZW
from test_zstd_twin import E_CHECKSUM, E_OFFSET, ROOT, STAT_KEYS, all_cases, load_twin, not_accepted_cases, run

BLOCK_MAX = 1 << 17
ROUNDS = [1, 2, 3, 0]


def load_slide_twin(path):
    L = load_twin(path)
    u64p = C.POINTER(C.c_uint64)
    L.zs_twin_inflate_sliding.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_int, u64p, u64p, u64p]
    L.zs_twin_xxh64_parts.argtypes = [C.c_char_p, C.c_uint64, u64p, C.c_uint64]
    L.zs_twin_xxh64_parts.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def ztwin():
    from lrge_amd import build as B
    return load_slide_twin(B.build_zstd_twin())


def run_sliding(L, data, round_blocks=0, checksum=1):
    """(rc, bytes, stats, byte offset, slide stats): as test_zstd_twin.run; slide stats = (rounds, largest history, largest work
    text, bytes of history moved)"""
    st, sl = (C.c_uint64 * 9)(), (C.c_uint64 * 4)()
    bad = C.c_uint64()
    rc = L.zs_twin_inflate_sliding(data, len(data), round_blocks, checksum, st, C.byref(bad), sl)
    n = L.zs_twin_result(None)
    buf = C.create_string_buffer(max(1, n))
    L.zs_twin_result(buf)
    return rc, buf.raw[:n], dict(zip(STAT_KEYS, list(st))), bad.value, tuple(sl)


def small_window_text():
    return Z.fastq(24_000, 71) * 3


_SMALL = None


def small_window_cases():
    """the 72 000-byte text in one libzstd frame with a window of 1, 4 and 16 KiB: 71, 18 and 5 blocks, all but the last full"""
    global _SMALL
    if _SMALL is None:
        text = small_window_text()
        assert len(text) == 72_000
        _SMALL = [("window_log_%d" % w, Z.compress(text, 3, window_log=w), text) for w in (10, 12, 14)]
        assert [Z.walk(c)["per_frame"] for _, c, _ in _SMALL] == [[71], [18], [5]]
    return _SMALL


def frames_of(data):
    """[(window, [upper bound of every block's text: Block_Maximum_Size, for raw and RLE blocks their size])] from the headers"""
    out, p = [], 0
    while p < len(data):
        magic, = struct.unpack_from("<I", data, p)
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            p += 8 + struct.unpack_from("<I", data, p + 4)[0]
            continue
        fhd = data[p + 4]
        single, did, flag = (fhd >> 5) & 1, fhd & 3, fhd >> 6
        q = p + 5
        window = 0
        if not single:
            wd = data[q]
            q += 1
            window = (1 << (10 + (wd >> 3))) + ((1 << (10 + (wd >> 3))) >> 3) * (wd & 7)
        q += 4 if did == 3 else did
        n = single if flag == 0 else 1 << flag
        fcs = int.from_bytes(data[q:q + n], "little") + (256 if n == 2 else 0)
        q += n
        if single:
            window = fcs
        bmax, blocks = min(window, BLOCK_MAX), []
        while True:
            bh = int.from_bytes(data[q:q + 3], "little")
            q += 3
            last, typ, size = bh & 1, (bh >> 1) & 3, bh >> 3
            blocks.append(bmax if typ == 2 else size)
            q += 1 if typ == 1 else size
            if last:
                break
        p = q + (4 if fhd & 4 else 0)
        out.append((window, blocks))
    return out


def largest_round_bound(data, round_blocks):
    """no round's text is larger: rounds are runs of consecutive blocks, across frames"""
    ub = [b for _, blocks in frames_of(data) for b in blocks]
    k = round_blocks or 4096
    return max(sum(ub[i:i + k]) for i in range(0, len(ub), k))


@pytest.mark.parametrize("round_blocks", ROUNDS)
def test_streams_equal_libzstd_and_the_whole_text_twin(ztwin, round_blocks):
    for name, comp, plain in all_cases() + small_window_cases():
        rc, out, st, bad, sl = run_sliding(ztwin, comp, round_blocks)
        assert rc == 0 and out == plain == Z.decompress(comp), (name, rc, bad, st)
        rc_w, out_w, st_w, _ = run(ztwin, comp, round_blocks)
        assert rc_w == 0 and st == st_w, (name, st, st_w)
        assert sl[0] == st["rounds"], (name, sl, st)
        # the memory claim: the history is never more than a frame's window, the work text never more than history plus one round
        assert sl[1] <= max(w for w, _ in frames_of(comp)), (name, sl)
        assert sl[2] <= sl[1] + largest_round_bound(comp, round_blocks), (name, sl)
        assert sl[2] <= sl[1] + len(plain) and sl[3] <= sl[1] * max(0, sl[0] - 1), (name, sl)


@pytest.mark.parametrize("round_blocks", [1, 2, 3])
def test_small_windows_keep_a_window_and_a_round(ztwin, round_blocks):
    """every block but the last is full, so the largest round's text is known exactly: history of one window, then the round"""
    for (name, comp, plain), w in zip(small_window_cases(), (10, 12, 14)):
        _, _, st, _, sl = run_sliding(ztwin, comp, round_blocks)
        window = 1 << w
        work, at = 0, 0
        while at < len(plain):
            size = min(round_blocks * window, len(plain) - at)
            work, at = max(work, min(window, at) + size), at + size
        assert sl[1] == window and sl[2] == work and sl[3] == window * (st["rounds"] - 1), (name, sl, work)


def frame(**kw):
    kw.setdefault("window_log", 10)
    return ZW.Frame(**kw)


def edge_cases():
    """(name, bytes, text, what the run at one block per round must show: {slide stat index: value})"""
    out = []
    d = ZW._dna(400, 70)
    # an offset of exactly the window, at the block's first byte: the source is the first byte of the carried history
    f = frame()
    f.raw(ZW._dna(1000, 71))
    f.raw(ZW._dna(1000, 72))
    f.compressed(ZW.literals("raw", d), d, [(0, 30, 1024 + 3), (10, 40, 1024 + 3)])
    out.append(("offset_equals_the_window", f.bytes(), bytes(f.text), {1: 1024}))
    # 200 bytes at offset 1 from the block's first byte: the source is the last byte of the history
    f = frame()
    f.raw(ZW._dna(700, 73) + b"Q")
    f.compressed(ZW.literals("raw", d), d, [(0, 200, 1 + 3), (5, 9, 100 + 3)])
    out.append(("offset_1_from_the_last_history_byte", f.bytes(), bytes(f.text), {1: 701}))
    # a frame that ends with a round, then a second frame: it starts with no history, and its matches stay inside it
    a, b = frame(), frame()
    a.raw(ZW._dna(900, 74))
    a.compressed(ZW.literals("raw", d), d, [(3, 50, 800 + 3)])
    b.raw(ZW._dna(300, 75))
    b.compressed(ZW.literals("raw", d), d, [(0, 64, 300 + 3), (7, 100, 2 + 3)])
    out.append(("frame_ends_with_the_round", a.bytes() + b.bytes(), bytes(a.text + b.text), {1: 900}))
    # three frames, a skippable frame between them
    fs = []
    for i in range(3):
        g = frame(checksum=i != 1, content_size=i != 2)
        g.raw(ZW._dna(500 + 37 * i, 76 + i))
        g.compressed(ZW.literals("raw", d), d, [(4, 90, 400 + 3)])
        g.rle(ord("N"), 45)
        fs.append(g)
    out.append(("three_frames_skippable_between", fs[0].bytes() + Z.skippable(b"gap", 4) + fs[1].bytes() + Z.skippable(b"", 9) + fs[2].bytes(),
                b"".join(bytes(g.text) for g in fs), {}))
    # no content size: the window is the header's, the frame's length is known only at its end
    f = frame(content_size=False)
    for i in range(4):
        f.raw(ZW._dna(600, 80 + i))
    f.compressed(ZW.literals("raw", d), d, [(0, 100, 1000 + 3), (20, 300, 3 + 3)])
    out.append(("no_content_size", f.bytes(), bytes(f.text), {1: 1024}))
    return out


def test_edge_frames_at_one_block_per_round(ztwin):
    for name, comp, plain, want in edge_cases():
        assert Z.decompress(comp) == plain, name
        for round_blocks in (1, 2):
            rc, out, st, bad, sl = run_sliding(ztwin, comp, round_blocks)
            assert rc == 0 and out == plain, (name, round_blocks, rc, bad)
            assert run(ztwin, comp, round_blocks)[2] == st, (name, round_blocks)
        _, _, st, _, sl = run_sliding(ztwin, comp, 1)
        assert sl[0] == st["blocks"], (name, sl, st)
        for i, v in want.items():
            assert sl[i] == v, (name, sl, want)


def test_offset_beyond_the_window_is_refused_where_the_whole_text_twin_refuses_it(ztwin):
    d = ZW._dna(400, 90)
    f = frame()
    f.raw(ZW._dna(1000, 91))
    f.raw(ZW._dna(1000, 92))
    f.compressed(ZW.literals("raw", d), d, [(0, 30, 1025 + 3)])
    data = f.bytes()
    for round_blocks in ROUNDS:
        rc, _, _, bad, _ = run_sliding(ztwin, data, round_blocks)
        rc_w, _, _, bad_w = run(ztwin, data, round_blocks)
        assert (rc, bad) == (rc_w, bad_w) == (E_OFFSET, 10 + 2 * 1003 + 3), (round_blocks, rc, bad, rc_w, bad_w)
    for name, data, status, at, _ in not_accepted_cases():
        for round_blocks in (1, 0):
            rc, _, _, bad, _ = run_sliding(ztwin, data, round_blocks)
            assert rc == status and (at is None or bad == at), (name, round_blocks, rc, bad)


def parts(L, text, cuts):
    a = (C.c_uint64 * max(1, len(cuts)))(*cuts)
    return L.zs_twin_xxh64_parts(text, len(text), a, len(cuts))


def test_xxh64_in_parts(ztwin):
    rng = random.Random(26)
    for n in list(range(101)) + [1023, 1024, 1025]:
        text = bytes(rng.getrandbits(8) for _ in range(n))
        want = ZW.xxh64(text)
        assert parts(ztwin, text, []) == want, n
        for a in range(n + 1):                                    # every split into two parts
            assert parts(ztwin, text, [a]) == want, (n, a)
        for _ in range(40):                                       # three parts
            a = rng.randint(0, n)
            b = rng.randint(a, n)
            assert parts(ztwin, text, [a, b]) == want, (n, a, b)


def stripe_frames():
    """frames of raw blocks of 100 bytes (a round at one block per round ends inside a stripe of 32) whose lengths are 0, 1 and 31
    modulo 32, and one below 32 bytes in two blocks: (bytes, text, where the last block's content starts)"""
    out = []
    for total in (640, 641, 671, 31):
        f = frame()
        text = ZW._dna(total, 100 + total)
        sizes = [100] * (total // 100) + ([total % 100] if total % 100 else []) if total > 100 else [20, total - 20]
        at = 0
        for s in sizes:
            f.raw(text[at:at + s])
            at += s
        data = f.bytes()
        out.append((data, text, len(data) - 4 - sizes[-1]))
    return out


def test_checksum_of_a_frame_whose_rounds_end_inside_a_stripe(ztwin):
    for data, text, last_at in stripe_frames():
        assert len(text) % 32 in (0, 1, 31) and Z.decompress(data) == text
        for round_blocks in (1, 2, 3):
            rc, out, st, _, sl = run_sliding(ztwin, data, round_blocks)
            assert rc == 0 and out == text and st["checksums_checked"] == 1, (len(text), round_blocks, rc)
        flipped = bytearray(data)
        flipped[last_at + 3] ^= 0x20
        for round_blocks in (1, 2, 3, 0):
            rc, _, _, bad, _ = run_sliding(ztwin, bytes(flipped), round_blocks)
            assert (rc, bad) == (E_CHECKSUM, len(data) - 4), (len(text), round_blocks, rc, bad)
        assert run_sliding(ztwin, bytes(flipped), 1, checksum=0)[0] == 0


def test_public_surface():
    import re
    from lrge_amd import _ffi, engine
    hdr = open(os.path.join(ROOT, "include", "lrge_hip.h")).read()
    assert re.search(r"#define\s+LRGE_GPU_INGEST_WINDOWED_ZSTD\s+2048\b", hdr) and _ffi.GPU_INGEST_WINDOWED_ZSTD == 2048
    assert "lrge_hip_reads_zstd_stats" in _ffi.EXPORTS and re.search(r"\blrge_hip_reads_zstd_stats\s*\(", hdr)
    assert hasattr(engine.DeviceReads, "zstd_stats")
    assert "LRGE_GPU_INGEST_WINDOWED_ZSTD" in open(os.path.join(ROOT, "include", "lrge_hip.hpp")).read()
    assert "LRGE_GPU_INGEST_WINDOWED_ZSTD" in open(os.path.join(ROOT, "tools", "lrge_hip_cli.cpp")).read()
    assert re.search(r"LRGE_GPU_INGEST_WINDOWED_ZSTD: c_int = 2048;", open(os.path.join(ROOT, "integration", "liblrge_hip_shim.rs")).read())


def test_sanitized_standalone_program(tmp_path):
    """tools/zstd_slide_check.cpp: the corpus, the writer's streams, the small-window and the edge frames, the refusals and a few
    hundred edited streams through the sliding twin, built with AddressSanitizer and UBSan as a program of its own and run as a
    child process: a read in front of a round's history is a heap overflow there."""
    exe = str(tmp_path / "zstd_slide_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "lrge_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "zstd_slide_check.cpp")])
    d = tmp_path / "cases"
    d.mkdir()
    accepted = all_cases() + small_window_cases() + [c[:3] for c in edge_cases()] + [("stripe_%d" % len(t), c, t) for c, t, _ in stripe_frames()]
    for name, comp, plain in accepted:
        (d / (name + ".zst")).write_bytes(comp)
        (d / (name + ".plain")).write_bytes(plain)
    for name, data, status, _, _ in not_accepted_cases():
        (d / ("refused_" + name + ".zst")).write_bytes(data)
        (d / ("refused_" + name + ".status")).write_text(str(status))
    rng = random.Random(4)
    pool = [c[1] for c in accepted if len(c[1]) < 20_000]
    for i in range(300):
        e = bytearray(rng.choice(pool))
        e[rng.randrange(len(e))] ^= 1 << rng.randrange(8)
        (d / ("%03d.edit" % i)).write_bytes(bytes(e))
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert "zstd_slide_check: ok" in r.stdout
