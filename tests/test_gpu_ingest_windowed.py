"""Windowed device ingest (LRGE_GPU_INGEST_WINDOWED, fx_window.h, k_fx_store): FASTA / FASTQ text that passes
through HBM in windows while only the bases stay, against the host reader -- raw, in BGZF, in one gzip member, in several and in
bzip2, at windows of a few thousand bytes and with INGEST_MAX_BYTES below the text; the resident path under the flag; the
budget; BAM and SAM, which stay resident; the inputs the device leaves to the host."""
import bz2
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import bam_corpus as B
import bgzf_writer as W
import bzip2_writer as ZW
import fastx_corpus as F
import gzip_corpus as G
import sam_corpus as S
from conftest import to_arrays

pytestmark = pytest.mark.gpu
CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_char), C.c_uint64, C.POINTER(C.c_char), C.c_uint64)
CASES = ["fq_big", "fa_big_w60_crlf", "fa_big_one_line", "fq_lead_trail_crlf", "fq_empty_seqs"] + \
        ["%s_size_%d" % (k, s) for k in ("fq", "fa") for s in (4095, 4096, 4097)]
WRAPS = ["raw", "bgzf", "gzip", "gzip_blocks", "multi", "bzip2"]
WINDOWS = [3001, 4097, 20000]


def flags(extra=0):
    from lrge_amd import _ffi
    return _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INFLATE_BZIP2 | _ffi.GPU_INGEST_WINDOWED | extra


_WRAPPED = {}


def wrap(text, how):
    """gzip: one member as zlib writes it; gzip_blocks: one member with a full flush every 3000 bytes, so that a round's output
    is about 40 KB (a round ends on a deflate block, and zlib's first block of fq_big is 153 127 bytes of text).
    bzip2: blocks of 1500 text bytes from the suite's own writer (libbz2 writes none below 100 KB), so that a round of two
    blocks is a fraction of a window; computed once per text"""
    if (text, how) not in _WRAPPED:
        if how == "raw":
            out = text
        elif how == "bgzf":
            out = W.bgzf_compress(text, block=3000)
        elif how == "gzip":
            out = G.gz(text)
        elif how == "gzip_blocks":                       # one member too, a deflate block every 3000 bytes
            out = G.gz_flushed(text, zlib.Z_FULL_FLUSH, 3000)
        elif how == "bzip2":
            out = ZW.stream(text, size=1500)
        else:
            third = max(1, len(text) // 3)
            out = b"".join(G.gz(text[i:i + third], 1 + k % 9) for k, i in enumerate(range(0, max(1, len(text)), third)))
        _WRAPPED[(text, how)] = out
    return _WRAPPED[(text, how)]


def read_host(path):
    from lrge_amd import _ffi
    L = _ffi.lib()
    out = []
    cb = CB(lambda u, n, nl, b, bl: out.append((C.string_at(n, nl), C.string_at(b, bl))))
    err = C.create_string_buffer(512)
    L.lrge_hip_read_records.argtypes = [C.c_char_p, CB, C.c_void_p, C.c_char_p, C.c_uint64]
    rc = L.lrge_hip_read_records(os.fsencode(str(path)), cb, None, err, 512)
    return rc, out, err.value.decode()


class Ref:
    """the host reader's records of one text and, for three selections of them, the sketches of a host upload under both presets"""

    def __init__(self, ctx, path, name, text):
        path.write_bytes(text)
        rc, rec, msg = read_host(path)
        assert rc == 0, (name, msg)
        self.name, self.text = name, text
        self.names, self.seqs = [n for n, _ in rec], [s for _, s in rec]
        self.lens = np.array([len(s) for s in self.seqs], dtype=np.uint32)
        n, rng = len(rec), np.random.default_rng(7)
        self.sel = {"all": list(range(n)), "shuffled subset": rng.permutation(n)[:max(1, n // 2)].tolist(), "repeats": rng.integers(0, n, size=n + 3).tolist()}
        self.sketches = {}
        for what, idx in self.sel.items():
            sel = [self.seqs[i] for i in idx]
            if sum(len(s) for s in sel):
                H = ctx.upload(*to_arrays(sel))
                self.sketches[what] = [H.sketch(preset) for preset in (0, 1)]
                H.free()

    def check(self, dr, what):
        assert dr.n == len(self.names) and dr.text_bytes == len(self.text), (self.name, what)
        assert dr.names == self.names, (self.name, what)
        assert np.array_equal(dr.lens, self.lens), (self.name, what)
        for kind, idx in self.sel.items():
            s = dr.seqset(idx)
            assert s.n == len(idx) and np.array_equal(s.lens, self.lens[idx]), (self.name, what, kind)
            for preset, (xh, yh) in enumerate(self.sketches.get(kind, [])):
                xd, yd = s.sketch(preset)
                assert np.array_equal(xd, xh) and np.array_equal(yd, yh), (self.name, what, kind, preset)
            s.free()


@pytest.fixture(scope="module")
def refs(ctx, tmp_path_factory):
    p = tmp_path_factory.mktemp("windowed_host") / "in.txt"
    cases = dict(F.well_formed())
    return {name: Ref(ctx, p, name, cases[name]) for name in CASES}


def upload_still_works(ctx):
    s = ctx.upload(*to_arrays([b"ACGTACGTACGTTTGACCA" * 20, b"GGGTTTACACACGT" * 11]))
    x, _ = s.sketch(0)
    assert x.size > 0
    s.free()


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("how", WRAPS)
def test_corpus_against_the_host(ctx, knobs, refs, how, window):
    """Every case through windows of `window` bytes: the host's records, and more than one window wherever the text exceeds two.
    fq_big (178 KB of text, 93 KB of bases) runs with INGEST_MAX_BYTES one byte below its text: resident it would be refused
    (test_gpu_ingest.py::test_memory_cap).  The FASTA cases keep nearly all their text as bases and gain nothing from the store.
    The one exception is fq_big as the gzip member zlib writes: a round of the decoder ends on a deflate block, zlib's first block
    of it holds 153 127 bytes of text, and the block of the windows must take a round's output whole, so block and store need
    153 127 + 88 366 bytes, more than the 177 792 of the text.  No cap below the text can hold that file; it runs at the default
    cap (its largest window is asserted), and the same member with a deflate block every 3000 bytes runs below the text."""
    knobs.set("INGEST_WINDOW_BYTES", window)
    knobs.set("INFLATE_CHUNK_BYTES", 20000)
    knobs.set("GZIP_CHUNK_BYTES", 512)
    knobs.set("GZIP_ROUND_BYTES", 8192)
    knobs.set("GZIP_SLOT_RATIO", 64)
    knobs.set("BZIP2_ROUND_BLOCKS", 2)
    for name in CASES:
        ref = refs[name]
        below = name == "fq_big" and how != "gzip"
        if below:
            knobs.set("INGEST_MAX_BYTES", len(ref.text) - 1)
        dr = ctx.open_reads(wrap(ref.text, how), flags())
        ref.check(dr, (how, window))
        st = dr.window_stats()
        if len(ref.text) > 2 * window:
            assert st[0] > 1, (name, how, window, st)
            assert st[1] == int(ref.lens.sum()) and st[2] >= window and st[3] > 0, (name, how, window, st)
        if name == "fq_big" and how == "gzip":
            assert st[2] >= 153127, st                               # (the first round's output, one deflate block)
        if len(ref.text) < window:                                   # (text of exactly a window may or may not be flushed)
            assert st == (0, 0, 0, 0), (name, how, window, st)
        dr.free()
        if below:
            knobs.unset("INGEST_MAX_BYTES")


def test_bzip2_of_libbz2_at_the_default_round(ctx, knobs, refs):
    """two blocks of 100 KB in one round: all of the text arrives at once, is cut behind its last record and leaves nothing"""
    knobs.set("INGEST_WINDOW_BYTES", 4097)
    ref = refs["fq_big"]
    dr = ctx.open_reads(bz2.compress(ref.text, 1), flags())
    ref.check(dr, "bzip2, one round")
    st = dr.window_stats()
    assert st[0] == 1 and st[1] == int(ref.lens.sum()) and st[2] == len(ref.text) and st[3] == 0, st
    dr.free()


def test_resident_path_under_the_flag(ctx, knobs, refs):
    """a window above the text: no window is flushed, and everything equals a call without the flag"""
    from lrge_amd import _ffi
    ref = refs["fq_big"]
    knobs.set("INGEST_WINDOW_BYTES", len(ref.text) + 1)
    for how in WRAPS:
        data = wrap(ref.text, how)
        a = ctx.open_reads(data, flags())
        b = ctx.open_reads(data, flags() & ~_ffi.GPU_INGEST_WINDOWED)
        assert a.window_stats() == (0, 0, 0, 0) == b.window_stats(), how
        assert a.n == b.n and a.names == b.names and np.array_equal(a.lens, b.lens) and a.text_bytes == b.text_bytes == len(ref.text), how
        ref.check(a, (how, "resident under the flag"))
        a.free(); b.free()


def test_budget(ctx, knobs, refs):
    """INGEST_MAX_BYTES bounds the bases plus the window: below the sum of the bases the call is unproven, whatever the window"""
    from lrge_amd import _ffi
    ref = refs["fq_big"]
    knobs.set("INGEST_WINDOW_BYTES", 3001)
    knobs.set("INGEST_MAX_BYTES", int(ref.lens.sum()) - 1)
    for how in ("raw", "bgzf", "gzip"):
        with pytest.raises(_ffi.UnprovenInput) as ei:
            ctx.open_reads(wrap(ref.text, how), flags())
        assert "INGEST_MAX_BYTES" in str(ei.value), how
        upload_still_works(ctx)
    knobs.unset("INGEST_MAX_BYTES")
    dr = ctx.open_reads(ref.text, flags())
    assert dr.n == 60 and dr.window_stats()[0] > 1
    dr.free()


def test_bam_and_sam_stay_resident(ctx, knobs, tmp_path):
    """with their flags BAM and SAM are not windowed: the same records as without the windowed flag, and the text cap as before"""
    from lrge_amd import _ffi
    reads = B.big_reads()[:12]
    bam = B.bam([B.record(n.split()[0], s) for n, s in reads])
    sam = S.toy_sam([n.split()[0] for n, _ in reads], [s for _, s in reads])
    knobs.set("GZIP_CHUNK_BYTES", 512)                               # (several rounds behind the one that brings the sniff)
    knobs.set("GZIP_ROUND_BYTES", 2048)
    knobs.set("BZIP2_ROUND_BLOCKS", 2)
    for data, extra in ((bam, _ffi.GPU_INGEST_BAM), (sam, _ffi.GPU_INGEST_SAM)):
        assert len(data) > 64 * 8
        for how, window in [(h, 64) for h in ("raw", "bgzf", "gzip", "gzip_blocks", "bzip2")] + [("raw", 2), ("gzip_blocks", 2)]:
            knobs.set("INGEST_WINDOW_BYTES", window)                 # (2: the sniff waits for its four bytes)
            a = ctx.open_reads(wrap(data, how), flags(extra))
            b = ctx.open_reads(wrap(data, how), flags(extra) & ~_ffi.GPU_INGEST_WINDOWED)
            assert a.window_stats() == (0, 0, 0, 0), how
            assert a.n == b.n == len(reads) and a.names == b.names == [n.split()[0] for n, _ in reads] and np.array_equal(a.lens, b.lens), how
            assert a.text_bytes == b.text_bytes == len(data)
            sa, sb = a.seqset(list(range(a.n))), b.seqset(list(range(b.n)))
            for preset in (0, 1):
                (xa, ya), (xb, yb) = sa.sketch(preset), sb.sketch(preset)
                assert np.array_equal(xa, xb) and np.array_equal(ya, yb), (how, preset)
            sa.free(); sb.free(); a.free(); b.free()
        knobs.set("INGEST_MAX_BYTES", len(data) - 1)
        for how in ("raw", "bgzf", "gzip"):
            with pytest.raises(_ffi.UnprovenInput):
                ctx.open_reads(wrap(data, how), flags(extra))
        knobs.unset("INGEST_MAX_BYTES")
        upload_still_works(ctx)


def test_small_record_in_front_of_a_large_one(ctx, knobs, tmp_path):
    """a cut a few bytes into the block with a tail far longer behind it: the tail is carried through a second block"""
    big = (b"ACGTN" * 8000)
    for k, text in enumerate((F.fastq_text([(b"s", b"AC"), (b"big", big), (b"t", b"GG")]), F.fasta_text([(b"s", b"AC"), (b"big", big), (b"t", b"GG")], 60))):
        ref = Ref(ctx, tmp_path / ("in%d.txt" % k), "small_then_big_%d" % k, text)
        for how, window in (("raw", 64), ("raw", 3001), ("bgzf", 64)):    # (gzip shrinks the repetitive record into one round: no tail)
            knobs.set("INGEST_WINDOW_BYTES", window)
            dr = ctx.open_reads(wrap(text, how), flags())
            ref.check(dr, (how, window))
            st = dr.window_stats()
            assert st[0] >= 2 and st[2] > len(big), (how, window, st)
            dr.free()


def test_unproven_corpus(ctx, knobs, tmp_path):
    """the inputs the resident scan leaves to the host, through windows of 64 bytes: unproven, or the host's records"""
    from lrge_amd import _ffi
    knobs.set("INGEST_WINDOW_BYTES", 64)
    p = tmp_path / "in.txt"
    for name, text in F.unproven():
        p.write_bytes(text)
        rc_h, rec_h, _ = read_host(p)
        for how in ("raw", "bgzf", "gzip"):
            try:
                dr = ctx.open_reads(wrap(text, how), flags())
            except _ffi.UnprovenInput as e:
                assert e.code == _ffi.ERR_UNPROVEN, (name, how)
                continue
            assert name not in ("sam_header", "bam_magic"), (name, how)
            assert rc_h == 0 and dr.names == [n for n, _ in rec_h] and dr.lens.tolist() == [len(s) for _, s in rec_h], (name, how)
            s = dr.seqset(list(range(dr.n)))
            H = ctx.upload(*to_arrays([q for _, q in rec_h]))
            assert all(np.array_equal(u, v) for u, v in zip(s.sketch(0), H.sketch(0))), (name, how)
            s.free(); H.free(); dr.free()
    upload_still_works(ctx)
