"""Unaligned BAM through the windows of the windowed ingest without a GPU (lrge_amd/csrc/fx_window.h, bam_round.h's tail mode,
DESIGN section 18): the host twin runs the window driver over its passes (bam_twin_windowed) with the segment, the window and
the appended piece as parameters, against the host parser (lrge_hip_read_records) on the same bytes.  A windowed scan gives the
host's records or the unproven verdict, never other records, and never keeps a record of a call it refuses; the store holds the
packed bytes of every record, dense, in file order."""
import ctypes as C
import math
import random
import struct

import pytest

import bam_corpus as B
from test_bam_twin import OK, UNPROVEN, STAT_NAMES, FxRec, host_records, load_twin, twin_records

SEGMENTS = [64, 257, 4096]
WINDOWS = [64, 257, 3001, 20000]


@pytest.fixture(scope="module")
def twin():
    L = load_twin()
    L.bam_twin_windowed.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]
    L.bam_twin_windowed_count.restype = C.c_uint64
    L.bam_twin_windowed_table.argtypes = [C.c_void_p]
    L.bam_twin_windowed_stats.argtypes = [C.POINTER(C.c_uint64 * 5)]
    L.bam_twin_windowed_bam_stats.argtypes = [C.c_void_p]
    L.bam_twin_windowed_store.argtypes = [C.c_char_p]
    L.bam_twin_windowed_store.restype = C.c_uint64
    L.bam_twin_windowed_seq.argtypes = [C.c_uint64, C.c_uint32, C.c_char_p]
    L.bam_twin_windowed_seq.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """text -> (rc, [(name, sequence)], message) of the host parser, computed once per text"""
    d = tmp_path_factory.mktemp("bam_window_host")
    seen = {}

    def run(text):
        if text not in seen:
            seen[text] = host_records(d, text)
        return seen[text]
    return run


def scans(L):
    st = (C.c_uint64 * 5)()
    L.bam_twin_windowed_stats(C.byref(st))
    return int(st[4])


def scan_bound(n, window, cuts):
    """between two cuts the block is scanned at `window` bytes and then each time it has doubled, so at most 1 + log2(n / window)
    times; `cuts` cuts, the stretch behind the last of them and the scan when the input ends"""
    return (cuts + 1) * (1 + math.ceil(math.log2(max(2, n / window)))) + 1


def windowed(L, data, S, window, piece):
    """(verdict, [(name, sequence)], (windows, store bytes, largest window, carried), summed BamStats, store)"""
    rc = L.bam_twin_windowed(data, len(data), S, window, piece)
    if rc != OK:
        assert L.bam_twin_windowed_count() == 0            # (a refused call keeps no record of an earlier window)
        return rc, None, None, None, None
    n = L.bam_twin_windowed_count()
    tab = (FxRec * max(1, n))()
    L.bam_twin_windowed_table(tab)
    st = (C.c_uint64 * 5)()
    L.bam_twin_windowed_stats(C.byref(st))
    store = C.create_string_buffer(max(1, L.bam_twin_windowed_store(None)))
    n_store = L.bam_twin_windowed_store(store)
    out, at = [], 0
    buf = C.create_string_buffer(max(1, max((tab[i].seq_len for i in range(n)), default=0)))
    for i in range(n):
        r = tab[i]
        assert r.name_off + r.name_len <= len(data) and r.seq_off == at and r.seq_span == (r.seq_len + 1) // 2     # dense, in file order
        assert L.bam_twin_windowed_seq(i, i % 4, buf) == r.seq_len
        out.append((data[r.name_off:r.name_off + r.name_len], buf.raw[:r.seq_len]))
        at += r.seq_span
    assert n_store == at and st[1] == (at if st[0] else 0)
    a = (C.c_uint64 * len(STAT_NAMES))()
    L.bam_twin_windowed_bam_stats(a)
    return rc, out, tuple(int(x) for x in st[:4]), dict(zip(STAT_NAMES, [int(x) for x in a])), store.raw[:n_store]


def pieces_for(text, window):
    return sorted({1, 61, window, max(1, len(text))})


@pytest.mark.parametrize("S", SEGMENTS)
def test_corpus_equals_host_parser(twin, host, S):
    """every well-formed case and bait at every window and piece: proven, with the host's records; zero fall-backs"""
    cases = B.well_formed()
    assert {n for n, _ in B.baits()} <= {n for n, _ in cases}
    n_rec = n_windowed = 0
    for name, data in cases:
        rc_h, rec_h, msg = host(data)
        assert rc_h == 0, (name, msg)
        for window in WINDOWS:
            for piece in pieces_for(data, window):
                rc, rec, st, _, _ = windowed(twin, data, S, window, piece)
                assert rc == OK, (name, S, window, piece, rc)
                assert rec == rec_h, (name, S, window, piece)
                n_rec += len(rec)
                n_windowed += st[0] > 1
    # (not vacuous: at windows 64 and 257 every case of more than two windows is cut at least once for the three small pieces)
    assert n_rec > 30000 and n_windowed > 100


def test_every_window_of_the_small_cases(twin, host):
    """every window size from 4 bytes up to the text, so that a block ends at every offset of a record and of the header"""
    cases = dict(B.well_formed())
    n_multi = 0
    for name in ("empty", "empty_no_text", "one_record", "names", "all_codes", "tags", "cigar_unmapped", "flags_with_4", "lengths"):
        data = cases[name]
        for window in range(4, len(data) + 1):
            piece = 1 if len(data) < 400 else window if window % 2 else 61
            rc, rec, st, _, _ = windowed(twin, data, 64, window, piece)
            assert rc == OK and rec == host(data)[1], (name, window, piece)
            n_multi += st[0] > 1
    assert n_multi > 2000


def test_unproven_list(twin):
    """what the resident scan leaves to the host is unproven at every window and piece"""
    for name, data in B.unproven():
        for window in [4, 17] + WINDOWS:
            for piece in (1, 61, window):
                for S in (64, 4096):
                    assert twin.bam_twin_windowed(data, len(data), S, window, piece) == UNPROVEN, (name, window, piece, S)
                    assert twin.bam_twin_windowed_count() == 0


def small_big_small():
    rng = random.Random(51)
    big = B._seq(rng, 40001, b"ACGTN")
    recs = [B.record(b"s", b"AC"), B.record(b"big", big), B.record(b"t", b"GGA")]
    return B.bam(recs), recs


def test_a_record_of_several_windows(twin, host):
    data = dict(B.well_formed())["long_record"]
    for window, piece in ((64, 61), (257, 257), (3001, 1000)):
        rc, rec, st, _, _ = windowed(twin, data, 64, window, piece)
        assert rc == OK and rec == host(data)[1]
        assert st[0] >= 2 and st[2] > 8 * window and st[2] >= 4 + 32 + 5 + 10001 + 20001, (window, st)      # the largest window held the record


def test_small_record_in_front_of_a_large_one(twin, host):
    """the cut lies a few bytes into the block and the tail behind it is far longer"""
    data, recs = small_big_small()
    rc, rec, st, _, _ = windowed(twin, data, 64, 64, 3001)
    assert rc == OK and rec == host(data)[1] and [len(s) for _, s in rec] == [2, 40001, 3]
    first_cut = len(B.header()) + len(recs[0])
    assert st[0] >= 2 and st[2] > len(recs[1]) and st[3] >= 3001 - first_cut > first_cut, st


def test_header_longer_than_the_window(twin, host):
    """the header fails only for lack of bytes: no cut, the block doubles until it holds the 100 KB header"""
    small = dict(B.well_formed())["header_refs_100k"]
    hdr = len(small) - sum(len(B.record(n, s)) for n, s in host(small)[1])
    assert hdr > 100000
    # (behind the 100 KB header as many bytes of records again: the block that has doubled past the header is flushed before the input ends)
    data = small[:hdr] + b"".join(B.record(n, s) for n, s in B.big_reads())
    assert len(data) > 2 * 65536 * 1.5
    for window, piece in ((64, 61), (257, 257), (3001, 1), (20000, 20000)):
        rc, rec, st, _, _ = windowed(twin, data, 257, window, piece)
        assert rc == OK and rec == host(data)[1] and len(rec) == 60
        assert st[0] >= 2 and st[2] >= hdr, (window, st)
        assert scans(twin) <= scan_bound(len(data), window, 61), (window, scans(twin))


def test_header_that_ends_the_text(twin, host):
    for hdr in (B.header(), B.header(b""), B.header(refs=[(b"chr1", 1000)])):
        assert host(hdr)[:2] == (0, [])
        for window in (4, 8, len(hdr) - 1, len(hdr) + 1):       # never whole before the input ends: scanned resident
            rc, rec, st, bs, _ = windowed(twin, hdr, 64, window, 1)
            assert rc == OK and rec == [] and st == (0, 0, 0, 0) and bs["segments"] == 0, window
        rc, rec, st, _, _ = windowed(twin, hdr, 64, len(hdr), len(hdr))     # whole in a window that is not the last: a cut at its end
        assert rc == OK and rec == [] and st == (1, 0, len(hdr), 0)


def test_record_ending_at_the_block_end_and_tails_of_1_2_3(twin, host):
    """cut = len with nothing carried; then 1, 2 and 3 bytes of the next record's block size in the tail"""
    rng = random.Random(52)
    recs = [B.record(b"r%d" % i, B._seq(rng, 10 + i)) for i in range(6)]
    data = B.bam(recs)
    edge = len(B.header()) + sum(len(r) for r in recs[:3])
    assert 2 * edge > len(data) > edge + 3
    for k in (0, 1, 2, 3):
        rc, rec, st, _, _ = windowed(twin, data, 64, edge + k, edge + k)
        assert rc == OK and rec == host(data)[1] and len(rec) == 6
        assert st == (2, sum((10 + i + 1) // 2 for i in range(6)), edge + k, k), (k, st)


def test_odd_and_zero_lengths_side_by_side_in_the_store(twin, host):
    """every record starts on a byte of the store; an odd length keeps its pad nibble, an empty sequence takes nothing"""
    seqs = [b"ACG", b"", b"T", b"", b"", b"GA", b"NACGT", b"", b"C"]
    data = B.bam([B.record(b"o%d" % i, s) for i, s in enumerate(seqs)])
    for window in (64, 100, 257):
        rc, rec, st, _, store = windowed(twin, data, 64, window, 61)
        assert rc == OK and rec == host(data)[1] and [s for _, s in rec] == seqs
        assert store == b"".join(B.pack_seq(s) for s in seqs) and st[1] == len(store) == 2 + 1 + 1 + 3 + 1
        assert st[0] >= 2


def test_mapped_record_in_the_third_window(twin, host):
    """two windows are flushed before the mapped record's bytes arrive: the whole call is unproven, no earlier record is kept"""
    rng = random.Random(53)
    recs = [B.record(b"m%d" % i, B._seq(rng, 30)) for i in range(12)]
    window = 200
    k = next(i for i in range(12) if len(B.header()) + sum(len(r) for r in recs[:i]) > 2 * window)
    good = B.bam(recs)
    rc, rec, st, _, _ = windowed(twin, good, 64, window, window)
    assert rc == OK and len(rec) == 12 and st[0] >= 3
    bad = B.bam(recs[:k] + [B.record(b"mapped", B._seq(rng, 30), flag=0)] + recs[k:])
    assert host(bad)[0] != 0
    assert twin.bam_twin_windowed(bad, len(bad), 64, window, window) == UNPROVEN
    assert twin.bam_twin_windowed_count() == 0 and twin.bam_twin_windowed_store(None) == 0
    assert scans(twin) >= 3                                 # (the refusal came from the third scan or a later one)


def test_bait_chain_across_a_cut(twin, host):
    """blocks that end at every offset of records whose tags and qualities spell record chains"""
    n_multi = 0
    for name, data in B.baits():
        rc_h, rec_h, _ = host(data)
        starts, o = [], len(B.header())
        for n, s in rec_h[:4]:
            starts.append(o)
            o += 4 + struct.unpack_from("<i", data, o)[0]
        short = data[:o]
        rc_s, rec_s, _ = host(short)
        assert rc_s == 0 and rec_s == rec_h[:4]
        for window in range(starts[1] - 8, o):
            for S in (64, 257):
                rc, rec, st, _, _ = windowed(twin, short, S, window, window)
                assert rc == OK and rec == rec_s, (name, window, S)
                n_multi += st[0] > 1
    assert n_multi > 300


def test_bad_block_size_on_the_proven_chain(twin, host):
    """a block size below 32 is refused as soon as its four bytes are there; one of 2^31 - 1 looks incomplete until the input
    ends, and the block is scanned a logarithmic number of times on the way"""
    rng = random.Random(54)
    recs = [B.record(b"b%d" % i, B._seq(rng, 20)) for i in range(3)]
    more = b"".join(B.record(b"c%d" % i, B._seq(rng, 20)) for i in range(40))
    for block, junk in ((31, bytes(31)), (0, b""), (-5, b""), (2 ** 31 - 1, bytes(100))):
        data = B.bam(recs) + struct.pack("<i", block) + junk + more
        assert host(data)[0] != 0
        for window, piece in ((64, 1), (64, 61), (257, 257)):
            assert twin.bam_twin_windowed(data, len(data), 64, window, piece) == UNPROVEN, (block, window)
            assert twin.bam_twin_windowed_count() == 0
            assert scans(twin) <= scan_bound(len(data), window, 4), (block, window, scans(twin))       # (the header and three records)
        if block < 32:                                     # refused in a window that is not the last: before the rest has arrived
            assert twin.bam_twin_windowed(data, len(data), 64, 64, 61) == UNPROVEN and scans(twin) <= 5


def test_single_byte_mutations(twin, tmp_path):
    """a few hundred single-byte edits of a well-formed file at one small window: each ends in the unproven verdict or in exactly
    the host's records"""
    base = dict(B.well_formed())["bait_quality"]
    assert twin.bam_twin_parse(base, len(base), 4096) == OK
    tab = (FxRec * twin.bam_twin_count())()
    twin.bam_twin_table(tab)
    starts = [r.name_off - 36 for r in tab]
    rng = random.Random(55)
    proven = unproven = 0
    for k in range(300):
        m = bytearray(base)
        pos = rng.choice(starts) + rng.randrange(36) if k % 2 else rng.randrange(len(B.header())) if k % 6 == 0 else rng.randrange(len(m))
        m[pos] = rng.randrange(256) if k % 4 < 2 else m[pos] ^ (1 << rng.randrange(8))
        m = bytes(m)
        S = SEGMENTS[k % 3]
        rc, rec, _, _, _ = windowed(twin, m, S, 257, (61, 257, 1000)[k % 3])
        rc_h, rec_h, msg = host_records(tmp_path, m)
        if rc == OK:
            assert rc_h == 0 and rec == rec_h, (k, pos, S, msg)
            proven += 1
        else:
            assert rc == UNPROVEN, (k, pos, S)
            unproven += 1
    assert proven >= 30 and unproven >= 30, (proven, unproven)


def test_resident_equivalence(twin):
    """a window larger than the text: nothing is flushed, and records and counts are those of the resident twin"""
    for name, data in B.well_formed():
        for S in SEGMENTS:
            rc, rec, st, bs, _ = windowed(twin, data, S, len(data) + 1, 61)
            assert rc == OK and st == (0, 0, 0, 0), (name, S)
            rc2, rec2, bs2 = twin_records(twin, data, S)
            assert rc2 == OK and rec == rec2 and bs == bs2, (name, S)


def test_arguments(twin):
    data = B.header()
    assert twin.bam_twin_windowed(data, len(data), 63, 64, 1) == -1             # a segment has 64 bytes or more
    assert twin.bam_twin_windowed(data, len(data), 64, 64, 0) == -1             # a piece has bytes


def test_abi_has_the_flag():
    import os
    import re
    from lrge_amd import _ffi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert re.search(r"#define\s+LRGE_GPU_INGEST_WINDOWED_ALN\s+64\b", open(os.path.join(root, "include", "lrge_hip.h")).read()) and _ffi.GPU_INGEST_WINDOWED_ALN == 64
    assert re.search(r"LRGE_GPU_INGEST_WINDOWED_ALN: c_int = 64;", open(os.path.join(root, "integration", "liblrge_hip_shim.rs")).read())
    assert "LRGE_GPU_INGEST_WINDOWED_ALN" in open(os.path.join(root, "include", "lrge_hip.hpp")).read()
    assert "LRGE_GPU_INGEST_WINDOWED_ALN" in open(os.path.join(root, "tools", "lrge_hip_cli.cpp")).read()


def test_k_bam_store_resources(tmp_path):
    """no scratch, no LDS, no spill, from the compiler's own report"""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "k.hip"
    src.write_text('#include "%s"\n' % os.path.join(root, "lrge_amd", "csrc", "k_bam.h"))
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-o", str(tmp_path / "k.o"), str(src),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    txt = r.stderr
    for k in ("k_bam_spans", "k_bam_store"):
        i = txt.index("Function Name: _Z%d%s" % (len(k), k))
        block = txt[i:i + 2000]
        val = lambda key: int(re.search(key + r": (\d+)", block).group(1))   # noqa: E731
        assert val(r"ScratchSize \[bytes/lane\]") == 0, k
        assert val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0, k
        assert val(r"LDS Size \[bytes/block\]") == 0, k
