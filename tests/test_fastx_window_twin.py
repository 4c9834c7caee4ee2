"""The windowed ingest without a GPU (lrge_amd/csrc/fx_window.h): the host twin runs the window driver over
its passes (fastx_twin_windowed) with the window and the appended piece as parameters, against the host parser
(lrge_hip_read_records) on the same bytes.  A windowed scan gives the host's records or the unproven verdict, never other
records; the well-formed corpus is proven at every window and piece; cuts at every offset of the hard cases; the window counts;
the store kernel's resources from the compiler; the new ABI symbols."""
import ctypes as C
import os
import re
import subprocess

import pytest

import fastx_corpus as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OK, UNPROVEN = 0, 1
PIECES = [1, 7, 61, 4096]
CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_char), C.c_uint64, C.POINTER(C.c_char), C.c_uint64)


def windows_for(text):
    n = len(text)
    return sorted({1, 17, 64, 257, 1000, 4096, max(1, n - 1), max(1, n), n + 1})


class FxRec(C.Structure):
    _fields_ = [("name_off", C.c_uint64), ("seq_off", C.c_uint64), ("seq_span", C.c_uint64), ("name_len", C.c_uint32), ("seq_len", C.c_uint32)]


@pytest.fixture(scope="module")
def twin():
    from lrge_amd import build as B
    L = C.CDLL(B.build_fastx_twin())
    L.fastx_twin_windowed.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]
    L.fastx_twin_windowed_count.restype = C.c_uint64
    L.fastx_twin_windowed_table.argtypes = [C.c_void_p]
    L.fastx_twin_windowed_stats.argtypes = [C.POINTER(C.c_uint64 * 4)]
    L.fastx_twin_windowed_seq.argtypes = [C.c_uint64, C.c_char_p]
    L.fastx_twin_windowed_seq.restype = C.c_uint64
    return L


def windowed(L, text, window, piece, tile=64):
    """(verdict, [(name, sequence)], stats) of the windowed twin"""
    rc = L.fastx_twin_windowed(text, len(text), tile, window, piece)
    if rc != OK:
        return rc, None, None
    n = L.fastx_twin_windowed_count()
    tab = (FxRec * max(1, n))()
    L.fastx_twin_windowed_table(tab)
    st = (C.c_uint64 * 4)()
    L.fastx_twin_windowed_stats(C.byref(st))
    out, at, buf = [], 0, C.create_string_buffer(max(1, max((tab[i].seq_len for i in range(n)), default=0)))
    for i in range(n):
        r = tab[i]
        assert r.name_off + r.name_len <= len(text) and r.seq_off == at and r.seq_span == r.seq_len     # dense, in file order
        assert L.fastx_twin_windowed_seq(i, buf) == r.seq_len
        out.append((text[r.name_off:r.name_off + r.name_len], buf.raw[:r.seq_len]))
        at += r.seq_len
    assert st[1] == at
    return rc, out, list(st)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """text -> (rc, [(name, sequence)], message) of the host parser, computed once per text"""
    from lrge_amd import _ffi
    L = _ffi.lib()
    L.lrge_hip_read_records.argtypes = [C.c_char_p, CB, C.c_void_p, C.c_char_p, C.c_uint64]
    p = tmp_path_factory.mktemp("host") / "in.txt"
    seen = {}

    def run(text):
        if text not in seen:
            p.write_bytes(text)
            out = []
            cb = CB(lambda u, n, nl, b, bl: out.append((C.string_at(n, nl), C.string_at(b, bl))))
            err = C.create_string_buffer(512)
            rc = L.lrge_hip_read_records(os.fsencode(str(p)), cb, None, err, 512)
            seen[text] = (rc, out, err.value.decode())
        return seen[text]
    return run


def check_invariant(L, host, text, window, piece, what):
    """the invariant of DESIGN section 17: the host's records, or the unproven verdict"""
    rc, rec, st = windowed(L, text, window, piece)
    assert rc in (OK, UNPROVEN), (what, window, piece, rc)
    if rc == OK:
        rc_h, rec_h, msg = host(text)
        assert rc_h == 0 and rec == rec_h, (what, window, piece, msg)
    return rc, st


@pytest.mark.parametrize("piece", PIECES)
def test_corpus_equals_host_parser(twin, host, piece):
    """every well-formed case at every window: proven, with the host's records; zero fallbacks"""
    cases = F.well_formed()
    assert len(cases) > 40
    n_rec = n_windowed = 0
    for name, text in cases:
        rc_h, rec_h, msg = host(text)
        assert rc_h == 0, (name, msg)
        for window in windows_for(text):
            rc, rec, st = windowed(twin, text, window, piece)
            assert rc == OK, (name, window, piece, rc)
            assert rec == rec_h, (name, window, piece)
            n_rec += len(rec)
            n_windowed += st[0] > 1
    assert n_rec > 4000 and n_windowed > 100          # (not vacuous: most runs really went through several windows)


def test_tiles_of_the_device(twin, host):
    """the big cases once more at the device's tile"""
    cases = dict(F.well_formed())
    for name in ("fq_big", "fa_big_w60_crlf", "fa_big_one_line", "fq_lead_trail_crlf", "fq_size_4097", "fa_size_4096"):
        for window in (3001, 4097, 20000):
            rc, rec, st = windowed(twin, cases[name], window, 3000, tile=4096)
            assert rc == OK and rec == host(cases[name])[1], (name, window)


def test_unproven_list(twin, host):
    """the inputs the resident scan leaves to the host: unproven here too, or proven with the host's records"""
    for name, text in F.unproven():
        for window in windows_for(text):
            for piece in (1, 7, 4096):
                rc, _ = check_invariant(twin, host, text, window, piece, name)
                if name in ("sam_header", "bam_magic"):
                    assert rc == UNPROVEN, (name, window, piece)


def every_window(twin, host, text, what, proven):
    n_multi = 0
    for window in range(1, len(text) + 2):
        rc, st = check_invariant(twin, host, text, window, 1, what)
        if proven:
            assert rc == OK, (what, window)
            n_multi += st[0] > 1
    return n_multi


def test_cut_never_between_cr_and_lf(twin, host):
    """CRLF text with one byte appended per step: blocks end between the CR and the LF at every line"""
    recs = [(b"r%d x" % i, b"ACGT" * (1 + i % 3)) for i in range(5)]
    assert every_window(twin, host, F.fastq_text(recs, b"\r\n"), "fq_crlf", True) > 20
    assert every_window(twin, host, F.fasta_text(recs, 5, b"\r\n"), "fa_crlf", True) > 20
    assert every_window(twin, host, F.fastq_text(recs, b"\r\n", final=False), "fq_crlf_nonl", True) > 20


def test_empty_sequence_and_quality_at_every_cut(twin, host):
    """records whose sequence and quality lines are empty, at every position relative to a cut; empty lines in front and behind"""
    recs = [(b"e0", b""), (b"n1", b"ACGT"), (b"e2", b""), (b"e3", b""), (b"n4", b"GG"), (b"e5", b"")]
    for eol in (b"\n", b"\r\n"):
        assert every_window(twin, host, F.fastq_text(recs, eol), "fq_empty", True) > 20
        assert every_window(twin, host, F.fastq_text(recs, eol, lead=2, trail=6), "fq_empty_lead_trail", True) > 20
        assert every_window(twin, host, F.fasta_text(recs, 3, eol, lead=1, trail=3), "fa_empty", True) > 10
    assert every_window(twin, host, F.fastq_text(recs[:1]), "fq_one_empty", True) == 0        # (one record: nothing to cut)


def test_sam_like_names_start_a_later_window(twin, host):
    """reads named HD1, SQ2 and RG3: the sniff for SAM belongs to the first window only"""
    recs = [(b"r0", b"ACGT"), (b"HD1", b"AC"), (b"SQ2 x", b"GGTT"), (b"RG3", b"T")]
    text = F.fastq_text(recs)
    first = len(F.fastq_text(recs[:1]))
    rc, rec, st = windowed(twin, text, first, 1)
    # (the first flush comes with exactly the first record in the block: the second window starts with "@HD1")
    assert rc == OK and st[0] >= 3 and [n for n, _ in rec] == [b"r0", b"HD1", b"SQ2", b"RG3"]
    assert every_window(twin, host, text, "fq_sam_like", True) > 20
    # the same names first in the file are the host's SAM sniff: unproven at every window
    for window in (1, 5, 16, 1000):
        assert windowed(twin, F.fastq_text(recs[1:]), window, 1)[0] == UNPROVEN


def test_fastq_followed_by_fasta(twin, host):
    text = F.fastq_text([(b"a", b"ACGT"), (b"b", b"GG")]) + b">x\nAC\n"
    assert host(text)[0] != 0                                                   # the host reports it
    for window in range(1, len(text) + 2):
        for piece in (1, 7):
            assert windowed(twin, text, window, piece)[0] == UNPROVEN, (window, piece)
    every_window(twin, host, F.fasta_text([(b"a", b"ACGT")], None) + b"@x\nAC\n+\nII\n", "fa_then_fq", False)


def test_a_record_longer_than_eight_windows(twin, host):
    """no cut inside a record: the window grows until the record is whole"""
    big = b"ACGTN" * 2000
    around = [(b"s", b"AC"), (b"big", big), (b"t", b"GG")]
    for text, alone in ((F.fastq_text(around), False), (F.fasta_text(around, 60), False), (F.fasta_text(around, None, b"\r\n"), False),
                        (F.fasta_text([(b"big", big)], None), True), (F.fastq_text([(b"big", big)]), True)):
        for window in (64, 1000):
            for piece in (61, 4096):
                rc, rec, st = windowed(twin, text, window, piece)
                assert rc == OK and rec == host(text)[1]
                if alone:
                    assert st[0] == 0                                            # never a cut: scanned whole when the input ends
                else:
                    assert st[0] >= 2 and st[2] > 8 * window                     # the largest window held the record


def test_window_counts(twin):
    text = dict(F.well_formed())["fq_big"]
    rc, rec, st = windowed(twin, text, 4096, 4096)
    assert rc == OK and len(rec) == 60 and st[0] >= 10 and st[2] >= 4096 and st[3] > 0
    for window in (len(text) + 1, 1 << 30):
        rc, rec, st = windowed(twin, text, window, 4096)
        assert rc == OK and len(rec) == 60 and st[0] == 0 and st[3] == 0


def test_arguments(twin):
    assert twin.fastx_twin_windowed(b">a\nA\n", 5, 100, 64, 1) == -1            # the tile is a multiple of 16
    assert twin.fastx_twin_windowed(b">a\nA\n", 5, 64, 64, 0) == -1             # a piece has bytes


def test_abi_has_the_windowed_ingest():
    from lrge_amd import _ffi
    L = _ffi.lib()
    hdr = open(os.path.join(ROOT, "include", "lrge_hip.h")).read()
    assert re.search(r"#define\s+LRGE_GPU_INGEST_WINDOWED\s+32\b", hdr) and _ffi.GPU_INGEST_WINDOWED == 32
    assert re.search(r"LRGE_GPU_INGEST_WINDOWED: c_int = 32;", open(os.path.join(ROOT, "integration", "liblrge_hip_shim.rs")).read())
    assert "LRGE_GPU_INGEST_WINDOWED" in open(os.path.join(ROOT, "include", "lrge_hip.hpp")).read()
    s = "lrge_hip_reads_window_stats"
    assert s in _ffi.EXPORTS and hasattr(L, s) and re.search(r"\b%s\s*\(" % s, hdr)


def test_k_fx_store_resources(tmp_path):
    src = tmp_path / "k.hip"
    src.write_text('#include "%s"\n' % os.path.join(ROOT, "lrge_amd", "csrc", "k_fastx.h"))
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-o", str(tmp_path / "k.o"), str(src),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    txt = r.stderr
    for k in ("k_fx_store", "k_fx_gather"):
        i = txt.index("Function Name: _Z%d%s" % (len(k), k))
        block = txt[i:i + 2000]
        val = lambda key: int(re.search(key + r": (\d+)", block).group(1))   # noqa: E731
        assert val(r"ScratchSize \[bytes/lane\]") == 0, k
        assert val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0, k
        assert val(r"LDS Size \[bytes/block\]") <= 4096, k
