"""The seek map of plain and multi-member gzip on the device (k_gz_win_pick, k_gz_entry): the census keeps an
entry table, the mapped open decodes only the entries its runs touch, each from its seed -- against the handle of the selected
open on the same input, the host reader's records, and the twin's entries and plan.  The shapes are small: a FASTQ of 2000 reads in
a handful of deflate blocks at a chunk of 4096 bytes, members of a few hundred bytes whose lengths walk every residue."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import fastx_corpus as F
import gzip_corpus as G
from test_gzip_seek_twin import bind, census
from test_gpu_ingest_selected import Ref, flags
from test_gpu_ingest_seek import same_handle
from test_gpu_ingest_windowed import upload_still_works

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WINDOW = 65536


@pytest.fixture(scope="module")
def twin():
    import ctypes as C
    from lrge_amd import build as Bd
    L = C.CDLL(Bd.build_fastx_twin())
    L.fastx_twin_windowed_count.restype = C.c_uint64
    return bind(L)


def set_knobs(knobs, chunk=4096, spacing=1, window=WINDOW):
    knobs.set("GZIP_CHUNK_BYTES", chunk)
    knobs.set("GZIP_SLOT_RATIO", 64)
    knobs.set("INGEST_SEEK_GZIP_BYTES", spacing)
    knobs.set("INGEST_WINDOW_BYTES", window)


def twin_census(twin, data, chunk=4096, spacing=1, window=WINDOW):
    """the twin's entries of the same file under the same options (stride: the default of INGEST_SEEK_STRIDE_BYTES)"""
    rc, out, ents, text = census(twin, data, chunk, spacing, window=window, stride=65536, tile=4096)
    assert rc == 0
    return out, ents, text


def twin_stats(twin, sel):
    import ctypes as C
    a = np.ascontiguousarray(sel, dtype=np.uint32)
    out = (C.c_uint64 * 4)()
    z = np.zeros(1, dtype=np.uint32)
    assert twin.fastx_twin_seek_plan(z.ctypes.data, z.ctypes.data, 0, 0, a.ctypes.data if a.size else None, a.size, C.byref(out)) == 0
    return tuple(int(x) for x in out)


@pytest.fixture(scope="module")
def fq(ctx, tmp_path_factory):
    text = G.fastq(2000)
    return Ref(ctx, tmp_path_factory.mktemp("seek_gzip") / "in.fq", "fastq2000", text, windows=[WINDOW])


def ordinals(n, k):
    """k seeded ordinals, ordinal 0 and the last among them"""
    if k == 1:
        return [n // 2]
    rng = np.random.default_rng(k)
    return sorted({0, n - 1} | set((1 + rng.permutation(n - 2)[:k - 2]).tolist()))


def check_mapped(ctx, twin, ref, data, src, m, sel, what):
    dr = ctx.open_reads_mapped(src, m, sel, flags())
    ref.check(dr, sel, what)
    other = ctx.open_reads_selected(data, sel, flags())
    same_handle(dr, other, what)
    assert other.seek_stats() == (0, 0, 0, 0), what
    st = dr.seek_stats()
    assert st == twin_stats(twin, sel), (what, st)
    if sel:
        idx = list(range(0, len(sel), 3))
        a, b = dr.seqset(idx), other.seqset(idx)
        (xa, ya), (xb, yb) = a.sketch(0), b.sketch(0)
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb), what
        a.free(); b.free()
    dr.free(); other.free()
    return st


@pytest.mark.parametrize("k", [1, 7, 200])
def test_mapped_open_equals_the_selected_open(ctx, knobs, twin, fq, k):
    """the handle is the selected open's, the statistics the twin planner's, the entries the twin's -- and the route is taken: runs
    are brought, and one chosen read decodes fewer entries than the map holds (on the parent commit gzip brought no run)"""
    set_knobs(knobs)
    data = G.gz(fq.text)
    plain = ctx.census_reads(data, flags())
    counts, m = ctx.census_map_reads(data, flags())
    assert counts == plain and counts[:3] == (fq.n, fq.bases, len(fq.text))
    out, ents, text = twin_census(twin, data)
    assert text == fq.text and len(ents) >= 4
    assert m.entries() == (len(ents), 32768 * len(ents), 4, 1), (m.entries(), len(ents))
    assert all(c == e[0] >> 3 for (_, t, c) in m.points() for e in [max(x for x in ents if x[1] <= t)])
    sel = ordinals(fq.n, k)
    assert len(sel) == k and (k == 1 or (sel[0] == 0 and sel[-1] == fq.n - 1))
    st = check_mapped(ctx, twin, fq, data, data, m, sel, ("mem", k))
    assert st[0] > 0, st
    if k == 1:
        assert 0 < st[3] < m.entries()[0] and st[2] < len(data), (st, m.entries())
    assert ctx.census_reads(data, flags()) == plain            # a census without a map returns what it returned
    m.free()


def test_from_a_path_reads_less_than_the_file(ctx, knobs, twin, fq, tmp_path):
    set_knobs(knobs)
    data = G.gz(fq.text)
    p = tmp_path / "in.fastq.gz"
    p.write_bytes(data)
    counts, m = ctx.census_map_reads(p, flags())
    assert counts[:3] == (fq.n, fq.bases, len(fq.text))
    out, ents, _ = twin_census(twin, data)
    assert m.entries()[0] == len(ents)
    for k in (1, 7):
        st = check_mapped(ctx, twin, fq, data, p, m, ordinals(fq.n, k), ("path", k))
        assert st[0] > 0 and (k > 1 or st[2] < len(data)), st
    m.free()


def test_two_members(ctx, knobs, twin, fq):
    """a member trailer and header inside the file: entries on either side, and a selection on either side of the seam"""
    set_knobs(knobs)
    cut = fq.text.index(b"\n@read01000 ") + 1
    data = G.gz(fq.text[:cut], 6) + G.gz(fq.text[cut:], 9)
    counts, m = ctx.census_map_reads(data, flags())
    out, ents, text = twin_census(twin, data)
    assert text == fq.text and m.entries()[0] == len(ents) and any(not e[5] for e in ents[1:])     # an entry at the second header
    for sel in ([999], [1000], [999, 1000], ordinals(fq.n, 7)):
        st = check_mapped(ctx, twin, fq, data, data, m, sel, ("two members", sel[:3]))
        assert st[0] > 0
    m.free()


def test_file_smaller_than_one_chunk(ctx, knobs, twin, tmp_path):
    text = dict(F.well_formed())["fq_lf_nl"]
    ref = Ref(ctx, tmp_path / "in.fq", "small", text, windows=[WINDOW])
    set_knobs(knobs)
    data = G.gz(text)
    assert len(data) < 4096
    counts, m = ctx.census_map_reads(data, flags())
    twin_census(twin, data)
    assert m.entries()[:3] == (1, 32768, 4)
    for sel in ([0], [ref.n - 1], list(range(ref.n)), []):
        st = check_mapped(ctx, twin, ref, data, data, m, sel, ("small", len(sel)))
        assert st == ((1, len(text), len(data), 1) if sel else (0, 0, 0, 0)), st
    m.free()


def test_a_sole_entry_over_several_chunks_is_not_entered(ctx, knobs, twin, fq):
    """the default spacing of 1 MiB is above this text: at a chunk of 4096 bytes the census walks many chunks and keeps entry 0
    alone, so there is nothing to skip -- the map has the kind "other" and the mapped open is the selected open, 0 runs"""
    set_knobs(knobs)
    knobs.unset("INGEST_SEEK_GZIP_BYTES")
    data = G.gz(fq.text)
    counts, m = ctx.census_map_reads(data, flags())
    assert counts[:3] == (fq.n, fq.bases, len(fq.text)) and m.entries() == (0, 0, 2, 0), m.entries()
    sel = ordinals(fq.n, 7)
    dr = ctx.open_reads_mapped(data, m, sel, flags())
    fq.check(dr, sel, "not entered")
    assert dr.seek_stats() == (0, 0, 0, 0)
    dr.free(); m.free()


def test_alignment_sweep(ctx, knobs, twin, tmp_path):
    """one FASTA record a member, the records' lengths walking 1..23: at a chunk of 64 bytes and spacing 1 every member is an entry,
    so the entries of the one batch start at every offset mod 4 in the staging and have every length mod 4; at spacings 2..40 they
    group differently.  The reads are those of zlib's text"""
    recs = [(b"r%d" % i, (b"ACGTTGCAGGTCATCGATCGGCTA" * 2)[i % 5:i % 5 + 1 + i % 23]) for i in range(96)]
    parts = [F.fasta_text([r], None) for r in recs]
    text = b"".join(parts)
    # (a file name of 150 bytes keeps two member headers out of one 64-byte chunk: every header is its chunk's candidate)
    data = b"".join(G.gz_header(p, fname=b"x" * 150) for p in parts)
    assert zlib.decompress(data, 47) == parts[0] and len(text) < WINDOW
    ref = Ref(ctx, tmp_path / "in.fa", "walk", text, windows=[WINDOW])
    seen = {}
    for spacing in (1, 2, 7, 40):
        set_knobs(knobs, chunk=64, spacing=spacing)
        knobs.set("INGEST_SEEK_STRIDE_BYTES", 1)                 # every record a point: a run a chosen record
        counts, m = ctx.census_map_reads(data, flags())
        rc, out, ents, got = census(twin, data, 64, spacing, window=WINDOW, stride=1, tile=4096)
        assert got == text and m.entries()[0] == len(ents)
        seen[spacing] = ({e[1] % 4 for e in ents}, {e[2] % 4 for e in ents})
        for sel in (list(range(ref.n)), list(range(0, ref.n, 2)), [ref.n - 1]):
            check_mapped(ctx, twin, ref, data, data, m, sel, ("walk", spacing, len(sel)))
        m.free()
    assert len(twin_census(twin, data, chunk=64, spacing=1)[1]) == len(recs)
    assert all(seen[s] == ({0, 1, 2, 3}, {0, 1, 2, 3}) for s in (1, 2, 7)), seen


def test_damaged_range_after_the_census(ctx, knobs, twin, fq):
    """a byte of a needed entry's compressed range changes after the census: the entry fails its checks, the call says that the map
    does not fit the input, and the selected open of the file as it was still delivers the reads"""
    from lrge_amd import _ffi
    set_knobs(knobs)
    data = G.gz(fq.text)
    counts, m = ctx.census_map_reads(data, flags())
    out, ents, _ = twin_census(twin, data)
    sel = [fq.n // 2]
    i = max(j for j, e in enumerate(ents) if e[1] <= fq.text.index(b"\n@read%05d " % sel[0]) + 1)
    assert 0 < i < len(ents) - 1
    bad = bytearray(data)
    bad[(ents[i][0] // 8 + ents[i + 1][0] // 8) // 2] ^= 0x10
    with pytest.raises(_ffi.UnprovenInput) as ei:
        ctx.open_reads_mapped(bytes(bad), m, sel, flags())
    assert ei.value.code == _ffi.ERR_UNPROVEN and "the map does not fit the input" in str(ei.value), str(ei.value)
    upload_still_works(ctx)
    dr = ctx.open_reads_selected(data, sel, flags())
    fq.check(dr, sel, "after the refusal")
    dr.free()
    # a file of another length is refused before any device work
    with pytest.raises(_ffi.LrgeHipError) as ei:
        ctx.open_reads_mapped(data[:-1], m, sel, flags())
    assert ei.value.code == _ffi.ERR_INVALID and "the map is of another input" in str(ei.value)
    st = check_mapped(ctx, twin, fq, data, data, m, sel, "undamaged again")
    assert st[0] == 1
    m.free()


def test_cli_seek_on_gzip_equals_the_sampled_route(tmp_path):
    """lrge-hip x.fastq.gz --gpu-ingest --gpu-sample --gpu-seek prints the estimate it prints without --gpu-seek"""
    from lrge_amd import build as Bd
    import gzip
    fa = gzip.decompress(open(os.path.join(HERE, "golden", "toy_reads.fa.gz"), "rb").read()).decode()
    recs = [(b.split("\n", 1)[0].encode(), "".join(b.split("\n")[1:]).encode()) for b in fa.split(">")[1:]]
    src = tmp_path / "x.fastq.gz"
    src.write_bytes(G.gz(F.fastq_text(recs)))
    cmd = [Bd.CLI_PATH, str(src), "--gpu-ingest", "--gpu-sample", "-T", "50", "-Q", "20", "-s", "1", "-f"]
    a = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    b = subprocess.run(cmd + ["--gpu-seek"], capture_output=True, text=True, timeout=300)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == b.stdout and a.stdout.strip(), (a.stdout, b.stdout)
    assert "gpu-ingest: device (sampled, seek)" in b.stderr and "gpu-ingest: device (sampled)\n" in a.stderr, (a.stderr, b.stderr)
