"""The device SAM record scan without a GPU: the host twin (lrge_amd/csrc/sam_twin.cpp, which runs the passes of k_sam.h over the
core of sam_core.h on the CPU, in the same 1 KiB steps of 64 sixteen-byte groups) against the host parser (lrge_hip_read_records)
over the corpus of tests/sam_corpus.py; the explicit list of inputs the device leaves to the host; single-byte mutations; the flag
constant; the kernels' resources from the compiler."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import sam_corpus as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OK, UNPROVEN, TOO_MANY = 0, 1, 2
CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_char), C.c_uint64, C.POINTER(C.c_char), C.c_uint64)


class FxRec(C.Structure):
    _fields_ = [("name_off", C.c_uint64), ("seq_off", C.c_uint64), ("seq_span", C.c_uint64), ("name_len", C.c_uint32), ("seq_len", C.c_uint32)]


def load_twin():
    from lrge_amd import build as Bd
    L = C.CDLL(Bd.build_sam_twin())
    L.sam_twin_parse.argtypes = [C.c_char_p, C.c_uint64]
    L.sam_twin_count.restype = C.c_uint64
    L.sam_twin_table.argtypes = [C.c_void_p]
    return L


@pytest.fixture(scope="module")
def twin():
    return load_twin()


def twin_records(L, data):
    """(verdict, [(name, sequence)]) rebuilt from the twin's record table"""
    rc = L.sam_twin_parse(data, len(data))
    if rc != OK:
        return rc, None
    n = L.sam_twin_count()
    tab = (FxRec * max(1, n))()
    L.sam_twin_table(tab)
    out = []
    for i in range(n):
        r = tab[i]
        assert r.name_off + r.name_len <= len(data) and r.seq_off + r.seq_span <= len(data) and r.seq_span == r.seq_len
        out.append((data[r.name_off:r.name_off + r.name_len], data[r.seq_off:r.seq_off + r.seq_len]))
    return rc, out


_host_lib = None


def host_records(tmp_path, data):
    """(rc, [(name, sequence)], message) of the host parser on the same bytes"""
    global _host_lib
    if _host_lib is None:
        from lrge_amd import _ffi
        _host_lib = _ffi.lib()
        _host_lib.lrge_hip_read_records.argtypes = [C.c_char_p, CB, C.c_void_p, C.c_char_p, C.c_uint64]
    p = tmp_path / "in.sam"
    p.write_bytes(data)
    out = []
    cb = CB(lambda u, n, nl, b, bl: out.append((C.string_at(n, nl), C.string_at(b, bl))))
    err = C.create_string_buffer(512)
    rc = _host_lib.lrge_hip_read_records(os.fsencode(str(p)), cb, None, err, 512)
    return rc, out, err.value.decode()


def test_corpus_equals_host_parser(twin, tmp_path):
    """every well-formed case: the host parser accepts it, the twin proves it -- no fall-back -- and names and sequences are the same"""
    cases = S.well_formed()
    assert len(cases) >= 20 and len(dict(cases)) == len(cases)
    n_rec = 0
    host = {}
    for name, data in cases:
        rc_h, rec_h, msg = host_records(tmp_path, data)
        assert rc_h == 0, (name, msg)
        rc, rec = twin_records(twin, data)
        assert rc == OK, (name, rc)
        assert rec == rec_h, name
        host[name] = rec_h
        n_rec += len(rec)
    assert n_rec > 3200                 # (the corpus is not vacuous)
    assert host["header_only"] == [] and host["header_no_lf"] == [] and len(host["short_3000"]) == 3000
    names = [n for n, _ in host["names"]]
    assert names == [b"", b"", b"n" * 254, b"with blanks  inside ", b" lead", b"nul\0inside", b"**", b"*x", b""]
    assert [s for _, s in host["star_star_sequence"]] == [b"**", b"", b"*A"]
    assert [len(s) for _, s in host["lengths"]] == [0, 0] + S.LENGTHS
    assert max(len(s) for _, s in host["long_200k"]) == 200000
    # line starts at every alignment, the tenth tab at every offset of a group and on both sides of a step
    starts = set()
    for k in range(16):
        data = dict(cases)["shift_%d" % k]
        starts.add(data.index(b"star\t") % 16)
    assert starts == set(range(16))


def test_unproven_list(twin, tmp_path):
    """the inputs that fall back, listed explicitly: the twin gives the unproven verdict, and what the host parser does with each is
    what the corpus records beside it"""
    cases = S.unproven()
    assert len(cases) >= 16
    for name, data, host in cases:
        assert twin.sam_twin_parse(data, len(data)) == UNPROVEN, name
        rc_h, rec_h, msg = host_records(tmp_path, data)
        assert (len(rec_h) if rc_h == 0 else msg) == host, (name, rc_h, msg)


def test_flag_constant():
    from lrge_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "lrge_hip.h")).read()
    assert re.search(r"#define\s+LRGE_GPU_INGEST_SAM\s+8\b", hdr) and _ffi.GPU_INGEST_SAM == 8
    shim = open(os.path.join(ROOT, "integration", "liblrge_hip_shim.rs")).read()
    assert re.search(r"LRGE_GPU_INGEST_SAM: c_int = 8;", shim)


def test_single_byte_mutations(twin, tmp_path):
    """single-byte edits of three well-formed files whose reads have 100 bases or more: each ends in the unproven verdict, or the
    host accepts the file and the records are identical.  Structural bytes (tabs, flags, line ends, the magic) are about a tenth
    of such lines, so at least half of the edits must end proven."""
    rng = random.Random(44)
    proven = unproven = total = 0
    for name, base in S.mutation_bases():
        rc, rec = twin_records(twin, base)
        assert rc == OK and rec and min(len(s) for _, s in rec) >= 100, name
        tabs = [i for i, c in enumerate(base) if c in b"\t\n\r"]
        for k in range(700):
            m = bytearray(base)
            # one edit in four at a tab or a line end or right beside one, the rest anywhere
            pos = min(len(m) - 1, max(0, rng.choice(tabs) + rng.randrange(-1, 2))) if k % 4 == 0 else rng.randrange(len(m))
            m[pos] = rng.choice(b"\t\n\r@*4 0") if k % 8 == 1 else rng.randrange(256) if k % 2 else m[pos] ^ (1 << rng.randrange(8))
            m = bytes(m)
            rc, rec = twin_records(twin, m)
            total += 1
            if rc == OK:
                rc_h, rec_h, msg = host_records(tmp_path, m)
                assert rc_h == 0 and rec == rec_h, (name, k, pos, msg)
                proven += 1
            else:
                assert rc == UNPROVEN, (name, k, pos)
                unproven += 1
    assert total >= 2000 and proven >= total // 2 and unproven >= 30, (proven, unproven)


def test_k_sam_resources(tmp_path):
    src = tmp_path / "k.hip"
    src.write_text('#include "%s"\n' % os.path.join(ROOT, "lrge_amd", "csrc", "k_sam.h"))
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-o", str(tmp_path / "k.o"), str(src),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    txt = r.stderr
    for k in ("k_sam_mark", "k_sam_records"):
        i = txt.index("Function Name: _Z%d%s" % (len(k), k))
        block = txt[i:i + 2000]
        val = lambda key: int(re.search(key + r": (\d+)", block).group(1))   # noqa: E731
        assert val(r"ScratchSize \[bytes/lane\]") == 0, k
        assert val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0, k
        assert val(r"LDS Size \[bytes/block\]") == 0, k
