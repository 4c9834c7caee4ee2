"""Block-parallel Zstandard decoding without a GPU: the host twin (lrge_amd/csrc/zs_twin.cpp, which runs zs_round.h's walk, rounds
and scan over the loops of zs_core.h, with the 64 lanes of every copy step) against libzstd over the corpus of
tests/zstd_corpus.py and the streams of tests/zstd_writer.py; the repeat-offset transfer function against a plain walk; what is
not accepted, beside what the host reader does with it; a seeded campaign of single-byte edits; the public surface."""
import ctypes as C
import os
import random
import re
import struct

import pytest

import zstd_corpus as Z
import zstd_writer as ZW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT_KEYS = ("frames", "skippable_frames", "blocks", "raw_blocks", "rle_blocks", "sequences", "checksums_checked", "rounds", "bytes_out")
# zs_core.h
(E_MAGIC, E_INPUT, E_RESERVED, E_DICT, E_WINDOW, E_BLOCK_TYPE, E_BLOCK_SIZE, E_LIT_HEADER, E_ACCURACY, E_FSE, E_WEIGHTS, E_BITSTREAM, E_NO_TABLE, E_SYMBOL,
 E_LITERALS, E_OFFSET, E_CONTENT_SIZE, E_CHECKSUM, E_SEQ_HEADER, E_TOO_BIG) = range(1, 21)


@pytest.fixture(scope="module")
def ztwin():
    from lrge_amd import build as B
    return load_twin(B.build_zstd_twin())


def load_twin(path):
    L = C.CDLL(path)
    L.zs_twin_inflate.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.zs_twin_result.argtypes = [C.c_void_p]
    L.zs_twin_result.restype = C.c_uint64
    u32p = C.POINTER(C.c_uint32)
    L.zs_twin_rep.argtypes = [u32p, u32p, C.c_uint64, C.c_uint64, u32p, u32p, u32p]
    return L


def run(L, data, round_blocks=0, checksum=1, budget=0):
    """(rc, bytes, stats, byte offset): rc 0 decoded, > 0 the ZS_E_* status"""
    st = (C.c_uint64 * 9)()
    bad = C.c_uint64()
    rc = L.zs_twin_inflate(data, len(data), round_blocks, checksum, budget, st, C.byref(bad))
    n = L.zs_twin_result(None)
    buf = C.create_string_buffer(max(1, n))
    L.zs_twin_result(buf)
    return rc, buf.raw[:n], dict(zip(STAT_KEYS, list(st))), bad.value


def all_cases():
    return Z.cases() + ZW.cases()


@pytest.mark.parametrize("round_blocks", [0, 1, 2])
def test_corpus_and_writer_streams_equal_libzstd(ztwin, round_blocks):
    for name, comp, plain in all_cases():
        assert Z.decompress(comp) == plain, name
        rc, out, st, bad = run(ztwin, comp, round_blocks)
        assert rc == 0 and out == plain, (name, rc, bad, st)
        want = Z.stats_of(comp)
        assert {k: st[k] for k in want} == want and st["bytes_out"] == len(plain), (name, st, want)
        assert st["checksums_checked"] == Z.walk(comp)["checksums"], (name, st)
        # a round is a run of consecutive blocks, across frames
        assert st["rounds"] == (-(-st["blocks"] // round_blocks) if round_blocks else 1), (name, st)


def test_checksum_option(ztwin):
    name, comp, plain = Z.by_name("fastq_l3")
    flipped = comp[:-1] + bytes([comp[-1] ^ 1])
    rc, _, _, bad = run(ztwin, flipped)
    assert (rc, bad) == (E_CHECKSUM, len(comp) - 4)
    rc, out, st, _ = run(ztwin, flipped, checksum=0)
    assert rc == 0 and out == plain and st["checksums_checked"] == 0


def test_budget(ztwin):
    name, comp, plain = Z.by_name("fastq_l3")
    assert run(ztwin, comp, 1, budget=len(plain))[0] == 0
    assert run(ztwin, comp, 1, budget=len(plain) - 1)[0] == E_TOO_BIG


def test_writer_keeps_its_streams():
    """libzstd decodes what the writer writes to the text it intended: at most two streams dropped, twenty or more kept"""
    assert len(ZW.dropped()) <= 2, ZW.dropped()
    assert len(ZW.cases()) >= 20
    names = {c[0] for c in ZW.cases()}
    for must in ("rle_literals", "direct_weights_1_stream", "direct_weights_4_streams", "rle_mode_ll", "rle_mode_of", "rle_mode_ml", "repeat_offsets_all_six",
                 "r1_minus_1_in_a_row", "nseq_127", "nseq_128", "nseq_three_bytes", "short_offsets_step_edges", "largest_length_codes",
                 "repeat_mode_after_predefined", "repeat_mode_after_rle", "treeless_two_blocks_behind", "no_content_size", "empty_frame",
                 "skippable_before_between_behind", "matches_over_block_fronts"):
        assert must in names, must
    shapes = {name: Z.walk(comp) for name, comp, _ in ZW.cases()}
    assert ("rle", 1) in shapes["rle_literals"]["lit"] and shapes["direct_weights_4_streams"]["weights"] == {"direct"}
    for t in ("ll", "of", "ml"):
        assert (t, "rle") in shapes["rle_mode_" + t]["modes"]
    assert shapes["nseq_three_bytes"]["nseq"] == [0x7F00 + 5] and shapes["nseq_127"]["nseq"] == [127] and shapes["nseq_128"]["nseq"] == [128]
    assert ("treeless", 4) in shapes["treeless_two_blocks_behind"]["lit"] and ("treeless", 1) in shapes["treeless_two_blocks_behind"]["lit"]
    assert shapes["treeless_two_blocks_behind"]["types"] == ["compressed", "raw", "compressed", "compressed"]
    assert ("of", "repeat") in shapes["repeat_mode_after_rle"]["modes"] and ("ll", "repeat") in shapes["repeat_mode_after_predefined"]["modes"]
    assert shapes["skippable_before_between_behind"]["skippable_frames"] == 3


def test_xxh64_of_the_writer():
    """the writer's XXH64 on the published vectors of the empty input and of "a" (seed 0)"""
    assert ZW.xxh64(b"") == 0xEF46DB3751D8E999 and ZW.xxh64(b"a") == 0xD24EC4F1A98C6E5B


def test_repeat_offset_function_equals_the_walk(ztwin):
    rng = random.Random(20)
    refused = agreed = 0
    for trial in range(400):
        n = rng.randint(1, 60)
        ofv = [rng.choice((1, 2, 3, 1, 2, 3, rng.randint(4, 40), rng.randint(4, 1 << 20))) for _ in range(n)]
        ll = [rng.choice((0, 0, 1, 5)) for _ in range(n)]
        start = [rng.randint(1, 50) for _ in range(3)] if trial % 3 else [1, 4, 8]
        a, b = (C.c_uint32 * n)(*ofv), (C.c_uint32 * n)(*ll)
        for piece in (0, 1, 7):
            by_fn, by_walk = (C.c_uint32 * 3)(), (C.c_uint32 * 3)()
            rc = ztwin.zs_twin_rep(a, b, n, piece, (C.c_uint32 * 3)(*start), by_fn, by_walk)
            if rc & 2:                       # the walk met an offset of 0: the function may or may not have seen it (the execution does)
                refused += 1
                continue
            assert rc == 0 and list(by_fn) == list(by_walk), (trial, piece, ofv, ll, start, list(by_fn), list(by_walk))
            agreed += 1
    assert agreed > 600 and refused > 10, (agreed, refused)


# ---- what is not accepted ----
def _frame(**kw):
    kw.setdefault("window_log", 10)
    kw.setdefault("content_size", False)
    kw.setdefault("checksum", False)
    return ZW.Frame(**kw)


def not_accepted_cases():
    """(name, bytes, status, byte offset, what the host reader does: "error" or "accepts")"""
    d = ZW._dna(400, 50)
    out = []
    ok = Z.by_name("fastq_l3")[1]
    single = ZW._frame_plain(ZW._dna(100, 51)).bytes()                       # magic, descriptor, one-byte content size, block

    def frame_case(name, status, host, build, at=9):
        f = _frame()
        build(f)
        out.append((name, f.bytes(), status, at, host))
    out.append(("dictionary_id", Z.MAGIC + bytes([0x21, 5, 3, 0x19, 0, 0]) + b"abc", E_DICT, 0, "error"))
    out.append(("reserved_bit", single[:4] + bytes([single[4] | 8]) + single[5:], E_RESERVED, 0, "error"))
    out.append(("block_type_3", single[:6] + bytes([single[6] | 6]) + single[7:], E_BLOCK_TYPE, 6, "error"))
    frame_case("block_above_maximum", E_BLOCK_SIZE, "error", lambda f: f.raw(ZW._dna(2000, 52)), at=6)
    frame_case("output_above_maximum", E_BLOCK_SIZE, "error", lambda f: f.compressed(ZW.literals("rle", b"A" * 1000), b"A" * 1000, [(1000, 100, 4)]))
    out.append(("window_log_28", Z.MAGIC + bytes([0, 18 << 3, 1, 0, 0]), E_WINDOW, 0, "error"))
    frame_case("accuracy_log", E_ACCURACY, "error", lambda f: f.body(b"\x00\x01\x80\x0f\xff\xff\xff\x01"))
    frame_case("weights_not_a_power_of_two", E_WEIGHTS, "error", lambda f: f.body(ZW.lit_header(2, 10, 3, 1) + bytes([129, 0x31, 0x01]) + b"\x00"))
    stream = ZW.DNA.description() + ZW.DNA.stream(d[:10])
    frame_case("bitstream_not_consumed", E_BITSTREAM, "error", lambda f: f.body(ZW.lit_header(2, 9, len(stream), 1) + stream + b"\x00"))
    frame_case("treeless_first", E_NO_TABLE, "error", lambda f: f.compressed(ZW.literals("treeless", d, ZW.DNA, 1), d))

    def repeat_first(f):
        f.prev = dict(ZW.PREDEFINED)
        f.compressed(ZW.literals("raw", d), d, [(20, 5, 8)], ("repeat", "predefined", "predefined"))
    frame_case("repeat_mode_first", E_NO_TABLE, "error", repeat_first)
    frame_case("too_few_literals", E_LITERALS, "error", lambda f: f.compressed(ZW.literals("raw", b"ACGT"), b"ACGT", [(10, 3, 4)], lenient=True))

    def offset_zero(f):
        f.raw(d[:20])
        f.compressed(ZW.literals("raw", d), d, [(0, 3, 3)], lenient=True)
    frame_case("offset_zero", E_OFFSET, "accepts", offset_zero, at=32)
    frame_case("offset_beyond_the_frame", E_OFFSET, "error", lambda f: f.compressed(ZW.literals("raw", d), d, [(5, 3, 100 + 3)], lenient=True))

    def beyond_window(f):
        for i in range(3):
            f.raw(ZW._dna(1000, 60 + i))
        f.compressed(ZW.literals("raw", d), d, [(5, 30, 2000 + 3)])
    frame_case("offset_beyond_the_window", E_OFFSET, "accepts", beyond_window, at=6 + 3 * 1003 + 3)
    out.append(("content_size_mismatch", single[:5] + bytes([single[5] + 1]) + single[6:], E_CONTENT_SIZE, 0, "error"))
    out.append(("wrong_checksum", ok[:-2] + bytes([ok[-2] ^ 0x10]) + ok[-1:], E_CHECKSUM, len(ok) - 4, "error"))
    out.append(("truncated_in_a_block", ok[:len(ok) // 2], E_INPUT, None, "error"))
    out.append(("truncated_checksum", ok[:-2], E_INPUT, len(ok) - 4, "error"))
    out.append(("bytes_behind_the_last_frame", ok + b"junk", E_MAGIC, len(ok), "error"))
    out.append(("one_byte_behind_the_last_frame", ok + b"\x00", E_INPUT, len(ok), "error"))
    return out


def test_not_accepted(ztwin):
    for name, data, status, at, host in not_accepted_cases():
        rc, _, _, bad = run(ztwin, data)
        assert rc == status, (name, rc, status, bad)
        if at is not None:
            assert bad == at, (name, bad, at)
        got = Z.decompress(data)
        assert ("accepts" if got is not None else "error") == host, (name, host)


def test_single_byte_edits(ztwin):
    """whenever the twin accepts an edited stream, libzstd accepts it and gives the same bytes; the twin may refuse more"""
    rng = random.Random(77)
    pool = [c for c in all_cases() if c[0] in ("small_100", "small_900", "all_bytes", "direct_weights_1_stream", "rle_mode_of", "repeat_offsets_all_six",
                                               "treeless_two_blocks_behind", "repeat_mode_after_rle", "matches_over_block_fronts", "skippable_before_between_behind")]
    pool.append(("fastq_small", Z.compress(Z.fastq(20_000, 9), 19), Z.fastq(20_000, 9)))
    accepted = refused = 0
    for name, comp, plain in pool:
        assert run(ztwin, comp)[0] == 0, name
        for _ in range(120):
            i = rng.randrange(len(comp))
            e = bytearray(comp)
            e[i] ^= 1 << rng.randrange(8)
            e = bytes(e)
            for ck in (1, 0):
                rc, out, _, _ = run(ztwin, e, rng.choice((0, 1, 2)), ck)
                if rc != 0:
                    refused += 1
                    continue
                accepted += 1
                if ck:
                    assert Z.decompress(e) == out, (name, i)
                else:                               # libzstd always checks the checksum: compare where it accepts
                    got = Z.decompress(e)
                    assert got is None or got == out, (name, i)
    assert accepted > 20 and refused > 500, (accepted, refused)


def test_public_surface():
    from lrge_amd import _ffi, build as B, engine
    hdr = open(os.path.join(ROOT, "include", "lrge_hip.h")).read()
    assert re.search(r"#define\s+LRGE_GPU_INFLATE_ZSTD\s+128\b", hdr) and _ffi.GPU_INFLATE_ZSTD == 128
    assert "lrge_hip_zstd_inflate" in _ffi.EXPORTS and re.search(r"\blrge_hip_zstd_inflate\s*\(", hdr)
    fields = re.search(r"typedef struct lrge_hip_zstd_stats \{(.*?)\}", hdr, re.S).group(1)
    assert re.findall(r"uint64_t\s+(\w+);", fields) == _ffi.ZSTD_STAT_NAMES and tuple(_ffi.ZSTD_STAT_NAMES[:9]) == STAT_KEYS
    assert hasattr(engine.Context, "zstd_inflate") and hasattr(B, "build_zstd_twin")
    assert "--gpu-zstd" in open(os.path.join(ROOT, "tools", "lrge_hip_cli.cpp")).read()
    assert "LRGE_GPU_INFLATE_ZSTD" in open(os.path.join(ROOT, "include", "lrge_hip.hpp")).read()
    assert re.search(r"LRGE_GPU_INFLATE_ZSTD: c_int = 128;", open(os.path.join(ROOT, "integration", "liblrge_hip_shim.rs")).read())


def test_sanitized_standalone_program(tmp_path):
    """tools/zstd_check.cpp: the corpus, the writer's streams, the refusals and a few hundred edited streams over the same twin,
    built with AddressSanitizer and UBSan as a program of its own and run as a child process."""
    import subprocess
    exe = str(tmp_path / "zstd_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "lrge_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "zstd_check.cpp")])
    d = tmp_path / "cases"
    d.mkdir()
    for name, comp, plain in all_cases():
        (d / (name + ".zst")).write_bytes(comp)
        (d / (name + ".plain")).write_bytes(plain)
    for name, data, status, _, _ in not_accepted_cases():
        (d / ("refused_" + name + ".zst")).write_bytes(data)
        (d / ("refused_" + name + ".status")).write_text(str(status))
    rng = random.Random(3)
    pool = [c[1] for c in all_cases() if len(c[1]) < 20_000]
    for i in range(300):
        e = bytearray(rng.choice(pool))
        e[rng.randrange(len(e))] ^= 1 << rng.randrange(8)
        (d / ("%03d.edit" % i)).write_bytes(bytes(e))
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "zstd_check: ok" in r.stdout
