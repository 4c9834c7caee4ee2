"""The device record scan without a GPU: the host twin (lrge_amd/csrc/fastx_twin.cpp, which runs the passes of k_fastx.h over
the core of fastx_core.h tile by tile on the CPU) against the host parser (lrge_hip_read_records) over the corpus of
tests/fastx_corpus.py at several tile sizes; the explicit list of inputs the device leaves to the host; the new ABI symbols;
the kernels' resources from the compiler."""
import ctypes as C
import os
import re
import subprocess

import pytest

import fastx_corpus as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TILES = [64, 4096, 1 << 20]
OK, UNPROVEN, TOO_MANY = 0, 1, 2
CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_char), C.c_uint64, C.POINTER(C.c_char), C.c_uint64)


class FxRec(C.Structure):
    _fields_ = [("name_off", C.c_uint64), ("seq_off", C.c_uint64), ("seq_span", C.c_uint64), ("name_len", C.c_uint32), ("seq_len", C.c_uint32)]


@pytest.fixture(scope="module")
def twin():
    from lrge_amd import build as B
    L = C.CDLL(B.build_fastx_twin())
    L.fastx_twin_parse.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64]
    L.fastx_twin_count.restype = C.c_uint64
    L.fastx_twin_table.argtypes = [C.c_void_p]
    L.fastx_twin_seq.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_char_p]
    L.fastx_twin_seq.restype = C.c_uint64
    return L


def twin_records(L, text, tile):
    """(verdict, [(name, sequence)]) rebuilt from the twin's record table"""
    rc = L.fastx_twin_parse(text, len(text), tile)
    if rc != OK:
        return rc, None
    n = L.fastx_twin_count()
    tab = (FxRec * max(1, n))()
    L.fastx_twin_table(tab)
    out = []
    for i in range(n):
        r = tab[i]
        assert r.name_off + r.name_len <= len(text) and r.seq_off + r.seq_span <= len(text) and r.seq_len <= r.seq_span
        buf = C.create_string_buffer(max(1, r.seq_len))
        assert L.fastx_twin_seq(text, len(text), i, buf) == r.seq_len
        out.append((text[r.name_off:r.name_off + r.name_len], buf.raw[:r.seq_len]))
    return rc, out


def host_records(tmp_path, text):
    """(rc, [(name, sequence)], message) of the host parser on the same bytes"""
    from lrge_amd import _ffi
    L = _ffi.lib()
    p = tmp_path / "in.txt"
    p.write_bytes(text)
    out = []
    cb = CB(lambda u, n, nl, b, bl: out.append((C.string_at(n, nl), C.string_at(b, bl))))
    err = C.create_string_buffer(512)
    L.lrge_hip_read_records.argtypes = [C.c_char_p, CB, C.c_void_p, C.c_char_p, C.c_uint64]
    rc = L.lrge_hip_read_records(os.fsencode(str(p)), cb, None, err, 512)
    return rc, out, err.value.decode()


@pytest.mark.parametrize("tile", TILES)
def test_corpus_equals_host_parser(twin, tmp_path, tile):
    """every well-formed case: the host parser accepts it, the twin proves it, and the records are the same; zero fallbacks"""
    cases = F.well_formed()
    assert len(cases) > 40
    n_rec = 0
    for name, text in cases:
        rc_h, rec_h, msg = host_records(tmp_path, text)
        assert rc_h == 0, (name, msg)
        rc, rec = twin_records(twin, text, tile)
        assert rc == OK, (name, tile, rc)
        assert rec == rec_h, (name, tile)
        n_rec += len(rec)
    assert n_rec > 500                  # (the corpus is not vacuous)


def test_records_straddle_tiles(twin):
    """at 64-byte tiles nearly every record of the big cases crosses a tile edge, and lines do too"""
    text = dict(F.well_formed())["fa_big_w60_crlf"]
    assert twin.fastx_twin_parse(text, len(text), 64) == OK
    n = twin.fastx_twin_count()
    tab = (FxRec * n)()
    twin.fastx_twin_table(tab)
    assert sum(1 for r in tab if r.seq_off // 64 != (r.seq_off + r.seq_span) // 64) > n // 2


def test_unproven_list(twin, tmp_path):
    """the only inputs that may fall back, listed explicitly: the twin gives the unproven verdict at every tile size, and the
    behaviour -- records or the reference's message -- is the host parser's, recorded here"""
    host = {}
    for name, text in F.unproven():
        for tile in TILES:
            assert twin.fastx_twin_parse(text, len(text), tile) == UNPROVEN, (name, tile)
        rc_h, rec_h, msg = host_records(tmp_path, text)
        host[name] = ([n for n, _ in rec_h], msg) if rc_h == 0 else msg
    assert host == {
        "fq_empty_line_between_records": ([b"a", b"b", b"c"], ""),          # the host skips empty lines between records
        "fq_three_line_tail": "truncated FASTQ record",
        "fq_plus_missing": "malformed FASTQ record: a",
        "fq_fifth_line_not_at": "malformed FASTQ record after a",
        "first_byte_other": "unrecognised sequence file",
        "sam_header": ([b"r0"], ""),                                        # parsed as SAM on the host
        "bam_magic": ([], ""),                                              # an empty BAM on the host: no header text, no records
        "fq_empty_quality_line_missing": "truncated FASTQ record",
    }


def test_tile_must_be_a_multiple_of_16(twin):
    assert twin.fastx_twin_parse(b">a\nA\n", 5, 100) == -1


def test_abi_has_the_ingest_entry_points():
    from lrge_amd import _ffi
    L = _ffi.lib()
    hdr = open(os.path.join(ROOT, "include", "lrge_hip.h")).read()
    assert re.search(r"#define\s+LRGE_ERR_UNPROVEN\s+-10\b", hdr)
    for s in ("lrge_hip_reads_open", "lrge_hip_reads_open_mem", "lrge_hip_reads_count", "lrge_hip_reads_name_bytes", "lrge_hip_reads_table",
              "lrge_hip_seqset_from_reads", "lrge_hip_reads_free"):
        assert s in _ffi.EXPORTS and hasattr(L, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    assert _ffi.ERR_UNPROVEN == -10 and issubclass(_ffi.UnprovenInput, _ffi.LrgeHipError)


def test_k_fastx_resources(tmp_path):
    src = tmp_path / "k.hip"
    src.write_text('#include "%s"\n' % os.path.join(ROOT, "lrge_amd", "csrc", "k_fastx.h"))
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-o", str(tmp_path / "k.o"), str(src),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    txt = r.stderr
    for k in ("k_fx_census", "k_fx_summary", "k_fx_scatter", "k_fx_records", "k_fx_names", "k_fx_gather"):
        i = txt.index("Function Name: _Z%d%s" % (len(k), k))
        block = txt[i:i + 2000]
        val = lambda key: int(re.search(key + r": (\d+)", block).group(1))   # noqa: E731
        assert val(r"ScratchSize \[bytes/lane\]") == 0, k
        assert val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0, k
        assert val(r"LDS Size \[bytes/block\]") <= 4096, k
