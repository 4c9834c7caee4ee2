"""The seek map of plain and multi-member gzip without a GPU (lrge_amd/csrc/fx_seek.h FX_SEEK_GZIP, gzip_round.h GzSeekRec,
gzip_core.h GzSeedEnv): the host twin runs the census with the recorder the device uses, decodes every entry
alone from its seed with the environment the kernel uses, plans with the planner the device uses and runs the mapped pass over
the sub-text the seeded decodes give.  The reference is zlib and the text itself."""
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest

import deflate_writer as DW
import fastx_corpus as F
import gzip_corpus as G
from deflate_corpus import member
from test_fastx_select_twin import OK, UNPROVEN, INVALID, selected, selections, window_records
from test_fastx_select_twin import twin as _select_twin   # noqa: F401  (fixture)
from test_fastx_seek_twin import bind as bind_seek, mapped as _mapped_plain, seek_plan   # noqa: F401
from test_gzip_twin import gtwin as _gtwin   # noqa: F401  (fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WIN = 32768
CHUNKS = [64, 1024, 16384]


def bind(L):
    """the prototypes of the twin's gzip map entries (the GPU suite binds them too)"""
    bind_seek(L)
    L.fastx_twin_gz_census_map.argtypes = [C.c_char_p] + [C.c_uint64] * 9 + [C.POINTER(C.c_uint64 * 4)]
    L.fastx_twin_gz_text.argtypes = [C.c_char_p]
    L.fastx_twin_gz_text.restype = C.c_uint64
    L.fastx_twin_gz_ring.restype = C.c_uint32
    L.fastx_twin_gz_entries.argtypes = [C.c_void_p, C.c_uint64]
    L.fastx_twin_gz_entries.restype = C.c_uint64
    L.fastx_twin_gz_window.argtypes = [C.c_uint64, C.c_char_p]
    L.fastx_twin_gz_poke_window.argtypes = [C.c_uint64, C.c_uint32, C.c_uint8]
    L.fastx_twin_gz_point_entries.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.fastx_twin_gz_point_entries.restype = C.c_uint64
    L.fastx_twin_gz_entry.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_char_p]
    L.fastx_twin_gz_mapped.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    L.fastx_twin_plan_stats.argtypes = [C.POINTER(C.c_uint64 * 4)]
    return L


@pytest.fixture(scope="module")
def twin(_select_twin):
    return bind(_select_twin)


@pytest.fixture(scope="module")
def gtwin(_gtwin):
    L = _gtwin
    L.gzip_twin_inflate_rec.argtypes = [C.c_char_p] + [C.c_uint64] * 5 + [C.POINTER(C.c_uint64)] * 3
    return L


def census(L, data, chunk, spacing, window=20000, stride=512, tile=64):
    """(verdict, counts, entries [(bit, off, len, crc, valid, in_member)], text) of the twin's census with a map on gzip bytes;
    the entries and the text are there whether or not the text is FASTA / FASTQ"""
    out = (C.c_uint64 * 4)()
    rc = L.fastx_twin_gz_census_map(data, len(data), chunk, 256 << 20, 64, spacing, tile, window, 4096, stride, C.byref(out))
    k = L.fastx_twin_gz_entries(None, 0)
    e = np.zeros((max(1, k), 6), dtype=np.uint64)
    L.fastx_twin_gz_entries(e.ctypes.data, k)
    text = C.create_string_buffer(max(1, L.fastx_twin_gz_text(None)))
    n = L.fastx_twin_gz_text(text)
    return rc, list(out), [tuple(int(x) for x in r) for r in e[:k]], text.raw[:n]


def entry(L, data, i, length, skew=0):
    """(status, text) of entry i decoded alone from its seed"""
    buf = C.create_string_buffer(max(1, length))
    rc = L.fastx_twin_gz_entry(data, len(data), i, skew, buf)
    return rc, buf.raw[:length] if rc == 0 else None


def window_of(L, i):
    buf = C.create_string_buffer(WIN)
    L.fastx_twin_gz_window(i, buf)
    return buf.raw


def boundaries(gtwin, data):
    bits, kind = (C.c_uint32 * 400000)(), (C.c_uint32 * 400000)()
    nb = gtwin.gzip_twin_boundaries(data, len(data), bits, kind, 400000)
    assert 0 < nb < 400000
    return set(bits[:nb])


def check_entries(L, data, text, ents, bounds, what):
    assert ents and ents[0][:2] == (0, 0), what
    for i, (bit, off, ln, crc, valid, in_member) in enumerate(ents):
        nxt = ents[i + 1] if i + 1 < len(ents) else (8 * len(data), len(text))
        assert bit < nxt[0] and (off < nxt[1] or i + 1 == len(ents)), (what, i)
        assert bounds is None or bit in bounds, (what, i, bit)
        assert ln == nxt[1] - off and crc == zlib.crc32(text[off:nxt[1]]), (what, i)
        assert valid <= min(off, WIN) and (in_member or not valid), (what, i)
        if i:
            assert window_of(L, i) == (b"\0" * WIN + text[:off])[-WIN:], (what, i)
        rc, got = entry(L, data, i, ln, skew=i & 3)
        assert rc == 0 and got == text[off:nxt[1]], (what, i, rc)


def corpus():
    out = [(n, d, t) for n, d, t in G.cases()]
    for name, text in F.well_formed():
        if name in ("fq_big", "fa_big_w60_crlf", "fq_lf_nl", "fq_ids"):
            out.append(("fx_" + name, G.gz(text, 6), text))
    return out


def test_entries_and_seeded_decode(twin, gtwin):
    """every case, chunk size and spacing: entry 0 is bit 0, the bits are true boundaries and ascend with the offsets, the window is
    the 32 KiB of text in front, length and CRC are the text's up to the next entry -- and every entry decoded alone from its seed is
    its slice of the text, at every staging skew.  Multi-member files put member headers and trailers inside entries, level 0
    stored blocks, Z_FIXED fixed ones, the flushed files empty stored blocks"""
    n_entries = n_inside = 0
    for name, data, text in corpus():
        bounds = boundaries(gtwin, data)
        for chunk in CHUNKS:
            for spacing in (1, 4096, len(text) + 1):
                what = (name, chunk, spacing)
                rc, out, ents, got = census(twin, data, chunk, spacing, window=1 << 30, stride=65536, tile=4096)
                assert rc in (OK, UNPROVEN) and got == text, what       # (UNPROVEN: the record scan of a text that is no FASTA / FASTQ)
                check_entries(twin, data, text, ents, bounds, what)
                assert all(b[1] - a[1] >= spacing for a, b in zip(ents, ents[1:])), what
                assert spacing <= len(text) or len(ents) == 1, what
                n_entries += len(ents)
                n_inside += sum(1 for e in ents if e[5])
    assert n_entries > 5000 and n_inside > 4000, (n_entries, n_inside)


def test_members_inside_an_entry(twin):
    """a spacing above the members: one entry holds several member headers and trailers, and decodes from its seed across them"""
    fq = G.fastq(600)
    data = b"".join(G.gz(fq[i:i + 3000], 1 + i % 9) for i in range(0, len(fq), 3000)) + G.gz(b"")
    rc, out, ents, text = census(twin, data, 1024, 20000)
    assert rc == OK and text == fq and 3 < len(ents) < len(fq) // 3000 / 3
    check_entries(twin, data, text, ents, None, "members")
    assert any(e[5] for e in ents[1:]) or any(not e[5] for e in ents[1:])


def built_stream():
    """a member whose non-final dynamic blocks each start with a match that reads the window's far end (distance 32768, the first
    byte of a preloaded window) or its near end (distance 1, length 258): wherever an entry falls on a block start, the match
    crosses it.  Returns (gzip bytes, text, text offsets of the block starts)"""
    rng = np.random.default_rng(11)
    d = DW.Deflate()
    d.dynamic(list(rng.integers(0, 256, WIN, dtype=np.uint8).tobytes()))
    starts = []
    for k in range(60):
        starts.append(len(d.out))
        first = (100, WIN) if k % 2 == 0 else (258, 1)
        d.dynamic([first] + list(rng.integers(65, 91, 700, dtype=np.uint8).tobytes()) + [(3, WIN), (258, WIN)])
    d.dynamic([(258, 1)], final=True)
    raw, plain = d.finish(), d.plain()
    assert zlib.decompress(raw, -15) == plain
    return member(raw, plain), plain, starts


def test_matches_across_an_entry_start(twin):
    data, text, starts = built_stream()
    far = near = 0
    for chunk in (64, 256, 1024):
        rc, out, ents, got = census(twin, data, chunk, 1)
        assert got == text
        check_entries(twin, data, text, ents, None, ("built", chunk))
        at = {e[1] for e in ents[1:]} & set(starts)
        far += sum(1 for o in at if starts.index(o) % 2 == 0)
        near += sum(1 for o in at if starts.index(o) % 2 == 1)
    assert far >= 5 and near >= 5, (far, near)


def test_entry_lengths_around_the_ring(twin):
    """members of one block each, so that every member is a link and, at spacing 1, an entry: text lengths 1, ring / 2 +- 1,
    ring +- 1 and 3 ring + 5 (and ring / 2 and ring themselves), each decoded at the four skews -- the halves that leave the ring
    start and end at every residue"""
    R = twin.fastx_twin_gz_ring()
    assert R == 65536
    want = [1, R // 2 - 1, R // 2, R // 2 + 1, R - 1, R, R + 1, 3 * R + 5, 7]
    unit = b"ACGTTGCAAC"
    parts = [(unit * (n // 10 + 1))[:n] for n in want]
    # (a file name of 150 bytes keeps two member headers out of one 64-byte chunk: every header is its chunk's candidate)
    data, text = b"".join(G.gz_header(p, fname=b"x" * 150, level=9) for p in parts), b"".join(parts)
    rc, out, ents, got = census(twin, data, 64, 1)
    assert got == text
    assert [e[2] for e in ents] == want, [e[2] for e in ents]
    for i, e in enumerate(ents):
        for skew in range(4):
            rc, t = entry(twin, data, i, e[2], skew)
            assert rc == 0 and t == text[e[1]:e[1] + e[2]], (i, skew, rc)
    # one entry for the lot: 6 ring of text through one ring, members starting inside it
    rc, out, ents, got = census(twin, data, 64, len(text) + 1)
    assert len(ents) == 1 and entry(twin, data, 0, len(text), 3) == (0, text)
    # a stored block longer than half the ring, entered at its start
    noise = np.random.default_rng(2).integers(0, 256, 3 * R, dtype=np.uint8).tobytes()
    data = G.gz(b"A" * 100, 9) + G.gz(noise, 0)
    rc, out, ents, got = census(twin, data, 64, 1)
    check_entries(twin, data, got, ents, None, "stored")
    assert got == b"A" * 100 + noise and max(e[2] for e in ents) > R // 2


FX_CASES = ["fq_lf_nl", "fa_lf_nl", "fq_crlf_nonl", "fa_crlf_nl", "fq_lead_trail_lf", "fa_w1_lf", "fq_ids", "fa_ids", "fq_empty_seqs", "fa_blank_lines_inside",
            "fq_single", "fa_header_only", "fq_size_4097", "fa_size_4095", "fq_big", "fa_big_w60_crlf", "fa_big_one_line", "size_0", "blank_only"]


def gz_mapped(L, data, text, window, piece, sel, tile=64):
    a = np.ascontiguousarray(sel, dtype=np.uint32)
    rc = L.fastx_twin_gz_mapped(data, len(data), tile, window, piece, a.ctypes.data if a.size else None, a.size)
    if rc != OK:
        return rc, None, None
    st = (C.c_uint64 * 4)()
    L.fastx_twin_plan_stats(C.byref(st))
    # the result reads as fastx_twin_selected's: the accessor of the select-twin test, without running anything again
    from test_fastx_select_twin import FxRec
    n = L.fastx_twin_windowed_count()
    tab = (FxRec * max(1, n))()
    L.fastx_twin_windowed_table(tab)
    buf = C.create_string_buffer(max(1, max((tab[i].seq_len for i in range(n)), default=0)))
    recs = []
    for i in range(n):
        assert L.fastx_twin_windowed_seq(i, buf) == tab[i].seq_len
        recs.append((text[tab[i].name_off:tab[i].name_off + tab[i].name_len], buf.raw[:tab[i].seq_len]))
    ss = (C.c_uint64 * 4)()
    L.fastx_twin_select_stats(C.byref(ss))
    return rc, recs, (tuple(st), list(ss))


def test_mapped_pass_equals_the_selected_twin(twin):
    """well-formed FASTA / FASTQ at levels 1 and 9 and as two members: every selection through the map gives the selected twin's
    reads and the planner's statistics; zero sub-texts are unproven"""
    cases = dict(F.well_formed())
    n_sel = n_skip = 0
    for name in FX_CASES:
        text = cases[name]
        half = len(text) // 2
        # (zlib closes a block every 16 Ki symbols or so: the texts of the corpus give one to three entries.  The flushed file has a
        # block, hence at chunk 64 an entry, every 1500 bytes of text)
        for how, data in (("l1", G.gz(text, 1)), ("l9", G.gz(text, 9)), ("two", G.gz(text[:half], 6) + G.gz(text[half:], 6)),
                          ("flushed", G.gz_flushed(text, zlib.Z_SYNC_FLUSH, 1500))):
            for chunk, spacing, stride, window in ((64, 1, 64, 3001), (64, 700, 1, 64), (1024, 4096, 3000, 20000), (16384, 1, len(text) + 1, len(text) + 1)):
                what = (name, how, chunk, spacing, stride)
                rc, out, ents, got = census(twin, data, chunk, spacing, window=window, stride=stride)
                assert rc == OK and got == text, what
                n = out[0]
                for kind, sel in selections(n, [n]).items():
                    rc, want, store, ss = selected(twin, text, window, 4096, sel)
                    assert rc == OK
                    rc, plan_st, _, _ = seek_plan(twin, sel)
                    assert rc == OK
                    rc, recs, st = gz_mapped(twin, data, text, window, 4096, sel)
                    assert rc == OK, (what, kind, rc)                # a condition, not a hope
                    assert recs == want and st[1] == ss, (what, kind)
                    assert st[0] == plan_st and st[0][3] <= len(ents) and st[0][2] <= len(data), (what, kind, st, plan_st)
                    if sel and len(ents) > 4 and kind in ("first", "last"):
                        assert st[0][3] < len(ents) and st[0][2] < len(data), (what, kind, st)
                        n_skip += 1
                    n_sel += 1
    assert n_sel > 1000 and n_skip > 20, (n_sel, n_skip)


def test_points_name_their_entry(twin):
    text = dict(F.well_formed())["fq_big"]
    data = G.gz_flushed(text, zlib.Z_SYNC_FLUSH, 5000)
    rc, out, ents, got = census(twin, data, 1024, 1, stride=512)
    assert rc == OK and len(ents) > 10
    k = twin.fastx_twin_map_points(None, None, 0)
    o, t = np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.uint64)
    twin.fastx_twin_map_points(o.ctypes.data, t.ctypes.data, k)
    c, b = np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.uint64)
    assert twin.fastx_twin_gz_point_entries(c.ctypes.data, b.ctypes.data, k) == k
    for off, c_off, blk in zip(t.tolist(), c.tolist(), b.tolist()):
        e = ents[blk]
        assert e[1] <= off < e[1] + e[2] and c_off == e[0] >> 3


def test_damage_after_the_census(twin):
    """a flipped bit in a needed entry's compressed range, a flipped window byte that a match reads, a truncated file: UNPROVEN or
    INVALID, or -- where the damage does not reach the chosen records' entry -- the same records; never other records"""
    text = dict(F.well_formed())["fq_big"]
    data = G.gz_flushed(text, zlib.Z_SYNC_FLUSH, 5000)
    rc, out, ents, got = census(twin, data, 1024, 1, window=20000, stride=512)
    assert rc == OK and len(ents) > 10
    n = out[0]
    rc, want, _, _ = selected(twin, text, 20000, 4096, [n // 2])
    rc, recs, st = gz_mapped(twin, data, text, 20000, 4096, [n // 2])
    assert rc == OK and recs == want and st[0][3] <= 2
    # which entry the record's run needs: the one whose decode the planner counts
    k = twin.fastx_twin_map_points(None, None, 0)
    o, t = np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.uint64)
    twin.fastx_twin_map_points(o.ctypes.data, t.ctypes.data, k)
    p = int(np.searchsorted(o, n // 2, side="right")) - 1
    i = max(j for j, e in enumerate(ents) if e[1] <= int(t[p]))
    lo, hi = ents[i][0] // 8 + 1, ents[i + 1][0] // 8 - 1
    n_bad = 0
    for byte in range(lo, hi, max(1, (hi - lo) // 12)):
        for bit in (0, 5):
            bad = bytearray(data)
            bad[byte] ^= 1 << bit
            rc = entry(twin, bytes(bad), i, ents[i][2])[0]
            assert rc > 0, (byte, bit)                           # a status, and no byte outside the entry's place was written
            assert gz_mapped(twin, bytes(bad), text, 20000, 4096, [n // 2])[0] == UNPROVEN
            n_bad += 1
    assert n_bad >= 20
    # a window byte that a match reads: the entry's text depends on its window (a FASTQ of 60 reads repeats its qualities)
    ok = entry(twin, data, i, ents[i][2])
    assert ok[0] == 0
    read = 0
    for j in range(WIN - 1, WIN - 4000, -97):
        old = window_of(twin, i)[j]
        twin.fastx_twin_gz_poke_window(i, j, old ^ 0x55)
        rc, txt = entry(twin, data, i, ents[i][2])
        if rc:                                                   # the byte was read: the CRC-32 says so
            read += 1
            assert rc == 15 and gz_mapped(twin, data, text, 20000, 4096, [n // 2])[0] == UNPROVEN
        else:
            assert txt == ok[1]
        twin.fastx_twin_gz_poke_window(i, j, old)
    assert read >= 1
    assert gz_mapped(twin, data, text, 20000, 4096, [n // 2])[1] == want
    # a truncated file, and one a byte longer: the map is of another input
    assert gz_mapped(twin, data[:-9], text, 20000, 4096, [n // 2])[0] == INVALID
    assert gz_mapped(twin, data + b"\0", text, 20000, 4096, [n // 2])[0] == INVALID
    # the last entry of a file cut inside it, offered at the map's length by padding: its decode ends early
    cut = data[:len(data) - 40] + b"\0" * 40
    assert entry(twin, cut, len(ents) - 1, ents[-1][2])[0] > 0
    # a distance that reaches before the member's first byte is a status, never a read of what the ring held before
    d = DW.Deflate()
    d.dynamic([65, 66, 67, (3, 3)], final=True)
    good = member(d.finish(), d.plain())
    d = DW.Deflate(history=b"xyz")
    d.dynamic([65, 66, 67, (3, 6)], final=True)
    far = member(d.finish(), d.plain())
    rc, out, ents, got = census(twin, good, 64, 1)
    assert got == b"ABCABC" and len(far) == len(good)
    assert entry(twin, far, 0, 6)[0] == 5                         # INF_E_DIST


def test_recorder_changes_nothing(gtwin):
    """gzip_twin_inflate returns identical bytes and statistics with and without a recorder"""
    for name, data, text in G.cases():
        for chunk in CHUNKS if len(data) < 70000 else CHUNKS[1:]:       # (the finder at 64 bytes a chunk is the slow part of the twin)
            st0, st1, bad0, bad1, ne = (C.c_uint64 * 7)(), (C.c_uint64 * 7)(), C.c_uint64(), C.c_uint64(), C.c_uint64()
            rc0 = gtwin.gzip_twin_inflate(data, len(data), chunk, 256 << 20, 64, st0, C.byref(bad0))
            out0 = C.create_string_buffer(max(1, gtwin.gzip_twin_result(None)))
            n0 = gtwin.gzip_twin_result(out0)
            rc1 = gtwin.gzip_twin_inflate_rec(data, len(data), chunk, 256 << 20, 64, 4096, st1, C.byref(bad1), C.byref(ne))
            out1 = C.create_string_buffer(max(1, gtwin.gzip_twin_result(None)))
            n1 = gtwin.gzip_twin_result(out1)
            assert rc0 == rc1 == 0 and list(st0) == list(st1) and bad0.value == bad1.value, (name, chunk)
            assert out0.raw[:n0] == out1.raw[:n1] == text and ne.value >= 1, (name, chunk)


def test_a_sole_entry_over_several_chunks_is_not_entered(twin):
    """fx_gz_enterable: a spacing above the text in a file of several chunks leaves nothing to skip; one chunk is entered"""
    twin.fastx_twin_gz_enterable.restype = C.c_int
    text = dict(F.well_formed())["fq_big"]
    data = G.gz_flushed(text, zlib.Z_FULL_FLUSH, 3000)
    for chunk, spacing, want in ((512, 1 << 20, 0), (512, 1, 1), (512, 4096, 1), (1 << 20, 1 << 20, 1), (1 << 20, 1, 1)):
        rc, out, ents, got = census(twin, data, chunk, spacing)
        assert rc == OK and (len(ents) == 1) == (spacing > len(text) or chunk > len(data)), (chunk, spacing, len(ents))
        assert twin.fastx_twin_gz_enterable() == want, (chunk, spacing)


def test_abi_has_the_entries():
    from lrge_amd import _ffi
    L = _ffi.lib()
    hdr = open(os.path.join(ROOT, "include", "lrge_hip.h")).read()
    s = "lrge_hip_read_map_entries"
    assert s in _ffi.EXPORTS and hasattr(L, s) and re.search(r"\b%s\s*\(" % s, hdr)
    assert "DESIGN section 28" in hdr and "INGEST_SEEK_GZIP_BYTES" in hdr


def test_entry_kernel_resources(tmp_path):
    """k_gz_entry: no scratch, no spills, the ring and the tables in LDS with room for two workgroups on a CU; k_gz_win_pick no LDS"""
    import subprocess
    src = tmp_path / "k.hip"
    src.write_text('#include "%s"\n' % os.path.join(ROOT, "lrge_amd", "csrc", "k_gzip.h"))
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-o", str(tmp_path / "k.o"), str(src),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    txt = r.stderr
    for k, lds in (("k_gz_entry", 80 << 10), ("k_gz_win_pick", 0)):
        i = txt.index("Function Name: _Z%d%s" % (len(k), k))
        block = txt[i:i + 2000]
        val = lambda key: int(re.search(key + r": (\d+)", block).group(1))   # noqa: E731
        assert val(r"ScratchSize \[bytes/lane\]") == 0, k
        assert val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0, k
        assert val(r"LDS Size \[bytes/block\]") <= lds, k
