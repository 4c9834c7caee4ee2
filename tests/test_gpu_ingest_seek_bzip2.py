"""The seek map of bzip2 on the device (k_bz_walk_rec, k_bz_rle_write_rec, k_bz_marks_text): the census keeps a block
table with 64 marks a block, the mapped open decodes only the entries its runs touch and enters every block of them at its marks --
against the handle of the selected open on the same input, the host reader's records, and the twin's blocks, entries and plan.  The
shapes are small: a FASTQ of 2000 reads in blocks of 1500 text bytes from the suite's writer, a level-1 file of libbz2's, and blocks
whose lengths and runs walk every residue of the segment length."""
import bz2
import os
import subprocess

import numpy as np
import pytest

import fastx_corpus as F
import gzip_corpus as G
from test_bzip2_seek_twin import bind, census, filler, stream, seg_of
from test_gpu_ingest_selected import Ref, flags
from test_gpu_ingest_seek import same_handle
from test_gpu_ingest_seek_gzip import ordinals, twin_stats
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


def set_knobs(knobs, spacing=1, window=WINDOW):
    knobs.set("INGEST_SEEK_BZIP2_BYTES", spacing)
    knobs.set("INGEST_WINDOW_BYTES", window)


def twin_census(twin, data, spacing=1, window=WINDOW, stride=65536):
    """the twin's blocks and entries of the same file under the same options (stride: the default of INGEST_SEEK_STRIDE_BYTES)"""
    rc, out, blocks, ents, text = census(twin, data, spacing, window=window, stride=stride, tile=4096)
    assert rc == 0
    return out, blocks, ents, text


@pytest.fixture(scope="module")
def fq(ctx, tmp_path_factory):
    text = G.fastq(2000)
    ref = Ref(ctx, tmp_path_factory.mktemp("seek_bzip2") / "in.fq", "fastq2000", text, windows=[WINDOW])
    ref.data = stream(text, size=1500)
    assert bz2.decompress(ref.data) == text
    return ref


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
    are brought, and one chosen read decodes fewer entries than the map holds (on the parent commit bzip2 brought no run)"""
    set_knobs(knobs)
    data = fq.data
    plain = ctx.census_reads(data, flags())
    counts, m = ctx.census_map_reads(data, flags())
    assert counts == plain and counts[:3] == (fq.n, fq.bases, len(fq.text))
    out, blocks, ents, text = twin_census(twin, data)
    assert text == fq.text and len(ents) == len(blocks) == -(-len(text) // 1500)
    assert m.entries() == (len(ents), 1024 * len(blocks), 5, 1), (m.entries(), len(ents))
    assert all(c == e[4] for (_, t, c) in m.points() for e in [max(x for x in ents if x[2] <= t)])
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
    data = fq.data
    p = tmp_path / "in.fastq.bz2"
    p.write_bytes(data)
    counts, m = ctx.census_map_reads(p, flags())
    assert counts[:3] == (fq.n, fq.bases, len(fq.text))
    out, blocks, ents, _ = twin_census(twin, data)
    assert m.entries()[0] == len(ents)
    for k in (1, 7):
        st = check_mapped(ctx, twin, fq, data, p, m, ordinals(fq.n, k), ("path", k))
        assert st[0] > 0 and st[2] < len(data), st
    m.free()


def sweep_blocks():
    """[(pre, text)] of FASTA records: blocks whose lengths in front of the run-length layer are the issue's (idle lanes, seg 4 and 8,
    1500; the blocks of 1 to 4 bytes cut one record), and runs of 4, 5, 259 and 260 bases, and of 4 with a count of 0 in front of
    another base, that start at every residue of the segment length at seg 4 and seg 8"""
    import random
    import bzip2_writer as BW
    rng = random.Random(31)
    parts, i = [], 0

    def rec(body):
        nonlocal i
        i += 1
        return b">r%d\n" % i + body + b"\n"
    for n in (5, 63, 64, 65, 255, 256, 257, 260, 1500):
        t = rec(filler(rng, n - len(b">r%d\n" % (i + 1)) - 1, b"ACGT"))
        assert BW.rle1(t) == t and len(t) == n
        parts.append((t, t))
    cut, at = rec(filler(rng, 40, b"ACGT")), 0
    for n in (1, 2, 3, 4, len(cut) - 10):
        parts.append((cut[at:at + n], cut[at:at + n]))
        at += n
    for kind, run in (("run4", 4), ("run5", 5), ("run259", 259), ("run260", 260), ("count0", 4)):
        for total in (40, 300):
            seg, at_residue = seg_of(total), set()
            for shift in range(seg):
                head = len(b">r%d\n" % (i + 1))
                t = rec(filler(rng, shift, b"CGT") + b"A" * run + (b"G" if kind == "count0" else b"C") + filler(rng, total - shift - head - 7, b"CGT"))
                pre = BW.rle1(t)
                assert seg_of(len(pre)) == seg and pre[head + shift:head + shift + 4] == b"AAAA"
                at_residue.add((head + shift) % seg)
                parts.append((pre, t))
            assert at_residue == set(range(seg)), (kind, total)
    return parts


def test_block_shape_sweep(ctx, knobs, twin, tmp_path):
    """at stride 1 every record is a point and a run a chosen record: blocks with idle lanes, seg 4 and 8, runs that end on, start at
    and straddle segment ends, a count byte as the first byte of a segment -- the reads are those of the text"""
    parts = sweep_blocks()
    text = b"".join(t for _, t in parts)
    data = stream(parts=parts)
    assert bz2.decompress(data) == text and len(text) < WINDOW
    ref = Ref(ctx, tmp_path / "in.fa", "sweep", text, windows=[WINDOW])
    set_knobs(knobs)
    knobs.set("INGEST_SEEK_STRIDE_BYTES", 1)
    counts, m = ctx.census_map_reads(data, flags())
    rc, out, blocks, ents, got = census(twin, data, 1, window=WINDOW, stride=1, tile=4096)
    assert rc == 0 and got == text and m.entries() == (len(ents), 1024 * len(blocks), 5, 1) and len(blocks) == len(parts)
    states = set()
    for b in range(len(blocks)):
        mk = np.zeros((64, 4), dtype=np.uint32)
        twin.fastx_twin_bz_marks(b, mk.ctypes.data)
        states |= {int(s) >> 16 for s in mk[:-(-blocks[b][4] // seg_of(blocks[b][4])), 1]}
    assert states == {0, 1, 2, 3, 4}, states
    for sel in (list(range(ref.n)), list(range(0, ref.n, 2)), [ref.n - 1], [0]):
        check_mapped(ctx, twin, ref, data, data, m, sel, ("sweep", len(sel)))
    m.free()


def test_libbz2_level_1(ctx, knobs, twin, tmp_path):
    """libbz2's own blocks: about 250 KB at level 1 are three blocks of seg 1564, each an entry at spacing 1; the default spacing of
    512 KiB makes them one entry of three blocks, which is not entered (kind 2)"""
    text = G.fastq(600)[:250000]
    text = text[:text.rindex(b"\n@read") + 1]
    ref = Ref(ctx, tmp_path / "in.fq", "level1", text, windows=[WINDOW])
    data = bz2.compress(text, 1)
    set_knobs(knobs)
    counts, m = ctx.census_map_reads(data, flags())
    out, blocks, ents, got = twin_census(twin, data)
    assert got == text and len(blocks) == 3 and m.entries() == (3, 3072, 5, 1)
    for sel in ([ref.n // 2], ordinals(ref.n, 7), []):
        st = check_mapped(ctx, twin, ref, data, data, m, sel, ("level 1", len(sel)))
        assert (st[0] > 0) == bool(sel) and (len(sel) != 1 or (st[3] < 3 and st[2] < len(data))), st
    m.free()
    knobs.unset("INGEST_SEEK_BZIP2_BYTES")
    counts, m = ctx.census_map_reads(data, flags())
    assert m.entries() == (0, 0, 2, 0), m.entries()
    m.free()


@pytest.fixture(scope="module")
def small(ctx, fq, tmp_path_factory):
    text = fq.text[:130000]
    text = text[:text.rindex(b"\n@read") + 1]
    ref = Ref(ctx, tmp_path_factory.mktemp("seek_bzip2_small") / "in.fq", "fastq130k", text, windows=[WINDOW])
    ref.data = stream(text, size=1500)
    return ref


def test_spacings(ctx, knobs, twin, small):
    """spacings 1, 2000, 7000 and 40000 group the blocks of 130 KB of text as the twin's recorder does; every grouping delivers the reads"""
    text, data, n = small.text, small.data, small.n
    seen = []
    for spacing in (1, 2000, 7000, 40000):
        set_knobs(knobs, spacing=spacing)
        counts, m = ctx.census_map_reads(data, flags())
        out, blocks, ents, got = twin_census(twin, data, spacing=spacing)
        assert got == text and counts[0] == n and m.entries() == (len(ents), 1024 * len(blocks), 5, spacing), (spacing, m.entries())
        seen.append(len(ents))
        for sel in ([n // 2], ordinals(n, 7)):
            st = check_mapped(ctx, twin, small, data, data, m, sel, (spacing, len(sel)))
            assert st[0] > 0, (spacing, st)
        m.free()
    assert seen[0] > seen[1] > seen[2] > seen[3] > 1, seen


def test_default_spacing_on_the_small_file_is_not_entered(ctx, knobs, small):
    """512 KiB is above 130 KB of text in 1500-byte blocks: a sole entry over many blocks could skip nothing -- kind "other", the
    mapped open is the selected open, 0 runs"""
    set_knobs(knobs)
    knobs.unset("INGEST_SEEK_BZIP2_BYTES")
    text, data = small.text, small.data
    counts, m = ctx.census_map_reads(data, flags())
    assert counts[2] == len(text) and m.entries() == (0, 0, 2, 0), m.entries()
    sel = [3, 70]
    dr = ctx.open_reads_mapped(data, m, sel, flags())
    small.check(dr, sel, "not entered")
    assert dr.seek_stats() == (0, 0, 0, 0)
    dr.free(); m.free()


def test_damaged_range_after_the_census(ctx, knobs, twin, fq):
    """a byte of a needed block changes after the census: the block fails its decode or its marks, the call says that the map does not
    fit the input, and the selected open of the file as it was still delivers the reads; the undamaged file maps again.  A file one
    byte shorter is the map of another input, before any device work"""
    from lrge_amd import _ffi
    set_knobs(knobs)
    data = fq.data
    counts, m = ctx.census_map_reads(data, flags())
    out, blocks, ents, _ = twin_census(twin, data)
    sel = [fq.n // 2]
    at = fq.text.index(b"\n@read%05d " % sel[0]) + 1
    e = max(x for x in ents if x[2] <= at)
    bad = bytearray(data)
    bad[(e[4] + e[5]) // 2] ^= 0x10
    with pytest.raises(_ffi.UnprovenInput) as ei:
        ctx.open_reads_mapped(bytes(bad), m, sel, flags())
    assert ei.value.code == _ffi.ERR_UNPROVEN and "the map does not fit the input" in str(ei.value), str(ei.value)
    upload_still_works(ctx)
    dr = ctx.open_reads_selected(data, sel, flags())
    fq.check(dr, sel, "after the refusal")
    dr.free()
    with pytest.raises(_ffi.LrgeHipError) as ei:
        ctx.open_reads_mapped(data[:-1], m, sel, flags())
    assert ei.value.code == _ffi.ERR_INVALID and "the map is of another input" in str(ei.value)
    st = check_mapped(ctx, twin, fq, data, data, m, sel, "undamaged again")
    assert st[0] == 1
    m.free()


def test_cli_seek_on_bzip2_equals_the_sampled_route(tmp_path):
    """lrge-hip x.fastq.bz2 --gpu-ingest --gpu-bzip2 --gpu-sample --gpu-seek prints the estimate it prints without --gpu-seek"""
    from lrge_amd import build as Bd
    import gzip
    fa = gzip.decompress(open(os.path.join(HERE, "golden", "toy_reads.fa.gz"), "rb").read()).decode()
    recs = [(b.split("\n", 1)[0].encode(), "".join(b.split("\n")[1:]).encode()) for b in fa.split(">")[1:]]
    src = tmp_path / "x.fastq.bz2"
    src.write_bytes(bz2.compress(F.fastq_text(recs), 1))
    cmd = [Bd.CLI_PATH, str(src), "--gpu-ingest", "--gpu-bzip2", "--gpu-sample", "-T", "50", "-Q", "20", "-s", "1", "-f"]
    a = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    b = subprocess.run(cmd + ["--gpu-seek"], capture_output=True, text=True, timeout=300)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == b.stdout and a.stdout.strip(), (a.stdout, b.stdout)
    assert "gpu-ingest: device (sampled, seek)" in b.stderr and "gpu-ingest: device (sampled)\n" in a.stderr, (a.stderr, b.stderr)
