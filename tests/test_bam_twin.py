"""The device BAM record scan without a GPU: the host twin (lrge_amd/csrc/bam_twin.cpp, which runs the passes of k_bam.h over the
core of bam_core.h segment by segment on the CPU) against the host parser (lrge_hip_read_records) over the corpus of
tests/bam_corpus.py at several segment sizes; the nibble gather at every destination alignment; the explicit list of inputs the
device leaves to the host; that the speculation is exercised; single-byte mutations; the kernels' resources from the compiler."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import bam_corpus as B

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEGMENTS = [64, 257, 4096, 1 << 20]
OK, UNPROVEN, TOO_MANY = 0, 1, 2
CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_char), C.c_uint64, C.POINTER(C.c_char), C.c_uint64)
STAT_NAMES = ["segments", "empty_segments", "speculative_starts", "rejected_starts", "repair_rounds", "rewalked_segments"]


class FxRec(C.Structure):
    _fields_ = [("name_off", C.c_uint64), ("seq_off", C.c_uint64), ("seq_span", C.c_uint64), ("name_len", C.c_uint32), ("seq_len", C.c_uint32)]


def load_twin():
    from lrge_amd import build as Bd
    L = C.CDLL(Bd.build_bam_twin())
    L.bam_twin_parse.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64]
    L.bam_twin_count.restype = C.c_uint64
    L.bam_twin_table.argtypes = [C.c_void_p]
    L.bam_twin_stats.argtypes = [C.c_void_p]
    L.bam_twin_seq.argtypes = [C.c_uint64, C.c_uint32, C.c_char_p]
    L.bam_twin_seq.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def twin():
    return load_twin()


def twin_stats(L):
    a = (C.c_uint64 * len(STAT_NAMES))()
    L.bam_twin_stats(a)
    return dict(zip(STAT_NAMES, [int(x) for x in a]))


def twin_records(L, data, S, misalign=None):
    """(verdict, [(name, sequence)], stats) rebuilt from the twin's record table; the sequences through bam_twin_seq"""
    rc = L.bam_twin_parse(data, len(data), S)
    if rc != OK:
        return rc, None, None
    n = L.bam_twin_count()
    tab = (FxRec * max(1, n))()
    L.bam_twin_table(tab)
    out = []
    for i in range(n):
        r = tab[i]
        assert r.name_off + r.name_len <= len(data) and r.seq_off + r.seq_span <= len(data) and r.seq_span == (r.seq_len + 1) // 2
        buf = C.create_string_buffer(max(1, r.seq_len))
        assert L.bam_twin_seq(i, i % 4 if misalign is None else misalign, buf) == r.seq_len
        out.append((data[r.name_off:r.name_off + r.name_len], buf.raw[:r.seq_len]))
    return rc, out, twin_stats(L)


def host_records(tmp_path, data):
    """(rc, [(name, sequence)], message) of the host parser on the same bytes"""
    from lrge_amd import _ffi
    L = _ffi.lib()
    p = tmp_path / "in.bam"
    p.write_bytes(data)
    out = []
    cb = CB(lambda u, n, nl, b, bl: out.append((C.string_at(n, nl), C.string_at(b, bl))))
    err = C.create_string_buffer(512)
    L.lrge_hip_read_records.argtypes = [C.c_char_p, CB, C.c_void_p, C.c_char_p, C.c_uint64]
    rc = L.lrge_hip_read_records(os.fsencode(str(p)), cb, None, err, 512)
    return rc, out, err.value.decode()


@pytest.fixture(scope="module")
def host_corpus(tmp_path_factory):
    """the host parser's records of every well-formed case, computed once"""
    d = tmp_path_factory.mktemp("bam_host")
    out = {}
    for name, data in B.well_formed():
        rc, rec, msg = host_records(d, data)
        assert rc == 0, (name, msg)
        out[name] = rec
    return out


@pytest.mark.parametrize("S", SEGMENTS)
def test_corpus_equals_host_parser(twin, host_corpus, S):
    """every well-formed case: the host parser accepts it, the twin proves it, and names and sequences are the same"""
    cases = B.well_formed()
    assert len(cases) >= 18
    n_rec = 0
    for name, data in cases:
        rc, rec, st = twin_records(twin, data, S)
        assert rc == OK, (name, S, rc)
        assert rec == host_corpus[name], (name, S)
        assert (st["segments"] == 0) == name.startswith("empty"), (name, st)
        n_rec += len(rec)
    assert n_rec > 3200                 # (the corpus is not vacuous)
    assert host_corpus["empty"] == [] and host_corpus["names"][0][0] == b"" and host_corpus["names"][5][0] == b"nul\0inside"


def test_gather_at_every_alignment(twin, host_corpus):
    """bam_twin_seq forms the bases as k_bam_gather does -- single bases to the word boundary, groups of eight, single bases --
    and gives the host's sequence for a destination at each of the four alignments"""
    for name in ("lengths", "all_codes", "big_60", "plain_40"):
        data = dict(B.well_formed())[name]
        for mis in range(4):
            rc, rec, _ = twin_records(twin, data, 4096, misalign=mis)
            assert rc == OK and [s for _, s in rec] == [s for _, s in host_corpus[name]], (name, mis)
    assert dict(host_corpus["all_codes"])[b"codes"] == B.NT16


def test_unproven_list(twin, tmp_path):
    """the inputs that fall back, listed explicitly: the twin gives the unproven verdict at every segment size, and the
    behaviour -- here always the reference's message -- is the host parser's, recorded here"""
    host = {}
    for name, data in B.unproven():
        for S in SEGMENTS:
            assert twin.bam_twin_parse(data, len(data), S) == UNPROVEN, (name, S)
        rc_h, rec_h, msg = host_records(tmp_path, data)
        host[name] = ([n for n, _ in rec_h], msg) if rc_h == 0 else msg
    mapped = "Mapped records are not supported. Only unaligned BAM/CRAM/SAM is allowed."
    assert host == {
        "mapped_first": mapped,
        "mapped_middle": mapped,
        "mapped_last": mapped,
        "block_below_32": "invalid BAM record",
        "negative_l_seq": "invalid BAM record",
        "seq_does_not_fit": "invalid BAM record",
        "last_record_cut": "truncated BAM file",
        "trailing_1": "truncated BAM file",
        "trailing_2": "truncated BAM file",
        "trailing_3": "truncated BAM file",
        "negative_l_text": "invalid BAM header",
        "header_cut_in_references": "truncated BAM file",
    }


def test_no_well_formed_case_is_unproven(twin):
    for name, data in B.well_formed():
        for S in SEGMENTS:
            assert twin.bam_twin_parse(data, len(data), S) == OK, (name, S)


def test_speculation_is_exercised(twin):
    """the baits make the finder err and the chain logic repair it; on dense short records nearly every segment starts from a
    candidate"""
    tot = dict.fromkeys(STAT_NAMES, 0)
    for name, data in B.baits():
        for S in SEGMENTS:
            assert twin.bam_twin_parse(data, len(data), S) == OK, (name, S)
            for k, v in twin_stats(twin).items():
                tot[k] += v
    assert tot["rejected_starts"] >= 1 and tot["repair_rounds"] >= 1, tot
    data = dict(B.well_formed())["short_3000"]
    assert twin.bam_twin_parse(data, len(data), 64) == OK
    st = twin_stats(twin)
    assert st["segments"] > 1500 and st["speculative_starts"] >= 0.9 * (st["segments"] - 1), st
    # a record that spans segments leaves them empty; unaligned records that carry a position give the finder nothing
    data = dict(B.well_formed())["long_record"]
    assert twin.bam_twin_parse(data, len(data), 4096) == OK and twin_stats(twin)["empty_segments"] >= 5
    data = dict(B.well_formed())["unmapped_with_pos"]
    assert twin.bam_twin_parse(data, len(data), 64) == OK
    st = twin_stats(twin)
    assert st["speculative_starts"] == 0 and st["repair_rounds"] >= 1 and st["rewalked_segments"] >= 1, st


def test_segment_below_64_is_refused(twin):
    data = B.header()
    assert twin.bam_twin_parse(data, len(data), 63) == -1


def test_single_byte_mutations(twin, tmp_path):
    """a few hundred single-byte edits of a well-formed file: each ends in the unproven verdict or in exactly the host's records"""
    base = dict(B.well_formed())["bait_quality"]
    assert twin.bam_twin_parse(base, len(base), 4096) == OK
    tab = (FxRec * twin.bam_twin_count())()
    twin.bam_twin_table(tab)
    starts = [r.name_off - 36 for r in tab]
    rng = random.Random(34)
    proven = unproven = 0
    for k in range(300):
        m = bytearray(base)
        # every other edit in the fixed fields of a record, one in six in the header, the rest anywhere
        pos = rng.choice(starts) + rng.randrange(36) if k % 2 else rng.randrange(len(B.header())) if k % 6 == 0 else rng.randrange(len(m))
        m[pos] = rng.randrange(256) if k % 4 < 2 else m[pos] ^ (1 << rng.randrange(8))
        m = bytes(m)
        S = SEGMENTS[k % 3]
        rc, rec, _ = twin_records(twin, m, S)
        rc_h, rec_h, msg = host_records(tmp_path, m)
        if rc == OK:
            assert rc_h == 0 and rec == rec_h, (k, pos, S, msg)
            proven += 1
        else:
            assert rc == UNPROVEN, (k, pos, S)
            unproven += 1
    assert proven >= 30 and unproven >= 30, (proven, unproven)      # (both ends were met)


def test_abi_has_the_bam_entry_point():
    from lrge_amd import _ffi
    L = _ffi.lib()
    hdr = open(os.path.join(ROOT, "include", "lrge_hip.h")).read()
    assert re.search(r"#define\s+LRGE_GPU_INGEST_BAM\s+4\b", hdr) and _ffi.GPU_INGEST_BAM == 4
    assert "lrge_hip_reads_bam_stats" in _ffi.EXPORTS and hasattr(L, "lrge_hip_reads_bam_stats") and re.search(r"\blrge_hip_reads_bam_stats\s*\(", hdr)
    fields = re.search(r"typedef struct lrge_hip_bam_stats \{(.*?)\}", hdr, flags=re.S).group(1)
    assert re.findall(r"uint64_t\s+([a-z_]+);", fields) == STAT_NAMES == _ffi.BAM_STAT_NAMES


def test_k_bam_resources(tmp_path):
    src = tmp_path / "k.hip"
    src.write_text('#include "%s"\n' % os.path.join(ROOT, "lrge_amd", "csrc", "k_bam.h"))
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-o", str(tmp_path / "k.o"), str(src),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    txt = r.stderr
    for k in ("k_bam_header", "k_bam_find", "k_bam_walk", "k_bam_records", "k_bam_gather"):
        i = txt.index("Function Name: _Z%d%s" % (len(k), k))
        block = txt[i:i + 2000]
        val = lambda key: int(re.search(key + r": (\d+)", block).group(1))   # noqa: E731
        assert val(r"ScratchSize \[bytes/lane\]") == 0, k
        assert val("VGPRs Spill") == 0 and val("SGPRs Spill") == 0, k
        assert val(r"LDS Size \[bytes/block\]") == 0, k
