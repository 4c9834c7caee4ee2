"""The streamed first pass of the device ingest (LRGE_GPU_INGEST_STREAM, option INGEST_STREAM_BYTES, lrge_hip_last_stream_stats;
DESIGN section 30): lrge_hip_reads_open, _census, _open_selected and _census_map of a path read the file in pinned pieces and give
what the whole-file route gives -- the host reader's records and sketches, the census, the seek map, the selected handle, the same
refusals with the same texts --, every file byte of plain and BGZF input read once, the pinned staging independent of the file's
length.  Raw, BGZF blocks of 3000 bytes, one gzip member, one with a full flush every 3000 bytes and three members; windows of 3001
and 20000 bytes; pieces of 509 bytes (below one BGZF member: the slot grows), 4096 (the _size_4095 / 4096 / 4097 cases end one byte
before, on and one byte behind a piece boundary) and above the file."""
import bz2
import os
import shutil
import subprocess

import numpy as np
import pytest

import bgzf_writer as W
import fastx_corpus as F
import gzip_corpus as G
from test_gpu_ingest_refusals import FQ, LENS, RECORD_REFUSALS, bgzf, bgzf_bad_second, flipped
from test_gpu_ingest_windowed import Ref, upload_still_works, wrap
from test_gpu_ingest_windowed_aln import big12

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["fq_big", "fa_big_w60_crlf", "fq_lead_trail_crlf", "fq_empty_seqs"] + ["%s_size_%d" % (k, s) for k in ("fq", "fa") for s in (4095, 4096, 4097)]
WRAPS = ["raw", "bgzf", "gzip", "gzip_blocks", "multi"]
WINDOWS = [3001, 20000]
PIECES = [509, 4096, 1 << 20]
SLACK = 64 << 10


def flags(extra=0, stream=True):
    from lrge_amd import _ffi
    return _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INFLATE_BZIP2 | _ffi.GPU_INGEST_WINDOWED | extra | (_ffi.GPU_INGEST_STREAM if stream else 0)


def set_knobs(knobs, window, piece):
    knobs.set("INGEST_WINDOW_BYTES", window)
    knobs.set("INGEST_STREAM_BYTES", piece)
    knobs.set("INFLATE_CHUNK_BYTES", 20000)
    knobs.set("GZIP_CHUNK_BYTES", 512)
    knobs.set("GZIP_ROUND_BYTES", 8192)
    knobs.set("GZIP_SLOT_RATIO", 64)
    knobs.set("BZIP2_ROUND_BLOCKS", 2)


def largest_member(data, how):
    """the largest member of a writer-made BGZF file (0 for any other wrap)"""
    if how != "bgzf":
        return 0
    at, most = 0, 0
    while at < len(data):
        size = int.from_bytes(data[at + 16:at + 18], "little") + 1
        most, at = max(most, size), at + size
    return most


def pinned_bound(piece, member):
    """two slots, one member of slack: a condition of the design, not a measurement"""
    return 2 * (max(piece, member) + SLACK)


@pytest.fixture(scope="module")
def refs(ctx, tmp_path_factory):
    p = tmp_path_factory.mktemp("stream_host") / "in.txt"
    cases = dict(F.well_formed())
    return {name: Ref(ctx, p, name, cases[name]) for name in CASES}


@pytest.fixture()
def put(tmp_path):
    def write(data, name="in.bin"):
        p = tmp_path / name
        p.write_bytes(data)
        return str(p)
    return write


def outcome(call):
    """("ok", what the call returned) or (code, message)"""
    from lrge_amd import _ffi
    try:
        return "ok", call()
    except _ffi.LrgeHipError as e:
        return e.code, str(e)


@pytest.mark.parametrize("piece", PIECES)
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("how", WRAPS)
def test_corpus_against_the_host(ctx, knobs, refs, put, how, window, piece):
    """the streamed open gives the host reader's names, lengths and text bytes and, for three selections, the sketches of a host
    upload under both presets; it streamed, read every byte of raw and BGZF input once, and held two slots at the most"""
    set_knobs(knobs, window, piece)
    for name in CASES:
        ref = refs[name]
        data = wrap(ref.text, how)
        dr = ctx.open_reads(put(data), flags())
        st = ctx.last_stream_stats()
        ref.check(dr, (how, window, piece))
        dr.free()
        what = (name, how, window, piece, st)
        assert st[3] == 1 and st[0] >= 1, what
        if how in ("raw", "bgzf"):
            assert st[1] == len(data), what
            assert st[2] <= pinned_bound(piece, largest_member(data, how)), what
            if piece < len(data):
                assert st[0] >= 2, what
        else:
            assert st[1] >= len(data), what                  # (the rounds read their overhang again)


@pytest.mark.parametrize("how", ["raw", "bgzf", "gzip_blocks", "multi"])
def test_census_map_and_selected_equal_the_whole_file_route(ctx, knobs, refs, put, how):
    """records, bases and text bytes of the census (the windows flushed may differ); the map's statistics, points and entries; the
    mapped open of that map; the selected open of a seeded subset"""
    for window, piece in ((3001, 509), (20000, 4096)):
        set_knobs(knobs, window, piece)
        knobs.set("INGEST_SEEK_STRIDE_BYTES", 3000)
        knobs.set("INGEST_SEEK_GZIP_BYTES", 6000)
        for name in ("fq_big", "fa_big_w60_crlf", "fq_size_4096"):
            ref = refs[name]
            data = wrap(ref.text, how)
            path = put(data)
            what = (name, how, window, piece)
            whole = ctx.census_reads(path, flags(stream=False))
            assert ctx.last_stream_stats() == (1, len(data), 0, 0), what
            got = ctx.census_reads(path, flags())
            assert ctx.last_stream_stats()[3] == 1, what
            assert got[:3] == whole[:3] == (len(ref.names), int(ref.lens.sum()), len(ref.text)), what
            wc, wm = ctx.census_map_reads(path, flags(stream=False))
            sc, sm = ctx.census_map_reads(path, flags())
            assert sc[:3] == wc[:3] == whole[:3], what
            assert sm.stats() == wm.stats() and sm.points() == wm.points() and sm.entries() == wm.entries(), (what, sm.stats(), wm.stats(), sm.entries(), wm.entries())
            n = len(ref.names)
            sel = sorted(np.random.default_rng(5).permutation(n)[:max(1, n // 3)].tolist())
            a = ctx.open_reads_selected(path, sel, flags())
            assert ctx.last_stream_stats()[3] == 1, what
            b = ctx.open_reads_selected(path, sel, flags(stream=False))
            m = ctx.open_reads_mapped(path, sm, sel, flags())
            for dr in (a, b, m):
                assert dr.names == [ref.names[i] for i in sel] and np.array_equal(dr.lens, ref.lens[sel]) and dr.text_bytes == len(ref.text), what
            assert a.select_stats() == b.select_stats() == m.select_stats(), what
            sa, sb = a.seqset(list(range(len(sel)))), b.seqset(list(range(len(sel))))
            if int(ref.lens[sel].sum()):
                for preset in (0, 1):
                    (xa, ya), (xb, yb) = sa.sketch(preset), sb.sketch(preset)
                    assert np.array_equal(xa, xb) and np.array_equal(ya, yb), (what, preset)
            sa.free(); sb.free(); a.free(); b.free(); m.free(); wm.free(); sm.free()


def test_mapped_open_of_a_map_that_is_not_entered_streams_its_pass(ctx, knobs, refs, put):
    """a gzip text below the spacing gives a map of kind 2: the mapped open runs the full selected pass, streamed under the flag"""
    set_knobs(knobs, 3001, 509)
    ref = refs["fq_big"]
    path = put(wrap(ref.text, "gzip_blocks"))
    _, m = ctx.census_map_reads(path, flags())
    assert m.entries()[2] == 2, m.entries()
    sel = [1, 7, 30]
    dr = ctx.open_reads_mapped(path, m, sel, flags())
    assert ctx.last_stream_stats()[3] == 1
    assert dr.names == [ref.names[i] for i in sel] and np.array_equal(dr.lens, ref.lens[sel])
    dr.free(); m.free()


def test_bam_and_sam(ctx, knobs, put, tmp_path):
    """one unaligned BAM and one SAM, plain, in BGZF and in gzip, with their flags and the flag that windows them, against the host
    reader; without that flag the streamed call is unproven and says which flag is missing"""
    from lrge_amd import _ffi
    bam, sam = big12()
    every = _ffi.GPU_INGEST_BAM | _ffi.GPU_INGEST_SAM | _ffi.GPU_INGEST_WINDOWED_ALN
    for kind, text in (("bam", bam), ("sam", sam)):
        ref = Ref(ctx, tmp_path / ("host." + kind), kind, text)
        for window, piece in ((3001, 509), (20000, 4096)):
            set_knobs(knobs, window, piece)
            for how in ("raw", "bgzf", "gzip_blocks"):
                path = put(wrap(text, how))
                dr = ctx.open_reads(path, flags(every))
                ref.check(dr, (kind, how, window, piece))
                assert ctx.last_stream_stats()[3] == 1 and dr.window_stats()[0] >= 1, (kind, how)
                dr.free()
                with pytest.raises(_ffi.UnprovenInput) as ei:
                    ctx.open_reads(path, flags(every & ~_ffi.GPU_INGEST_WINDOWED_ALN))
                assert ei.value.code == _ffi.ERR_UNPROVEN and "LRGE_GPU_INGEST_STREAM" in str(ei.value) and "LRGE_GPU_INGEST_WINDOWED_ALN" in str(ei.value), (kind, how, str(ei.value))
        upload_still_works(ctx)


def test_stream_statistics(ctx, knobs, refs, put):
    """streamed or whole by the container; bytes read; the pinned bytes do not grow with the file"""
    set_knobs(knobs, 3001, 4096)
    ref = refs["fq_big"]
    dr = ctx.open_reads(put(bz2.compress(ref.text, 1)), flags())
    st = ctx.last_stream_stats()
    assert st[3] == 0 and st[1] >= len(bz2.compress(ref.text, 1)), st
    ref.check(dr, "bzip2, read whole under the flag")
    dr.free()
    for how in ("raw", "bgzf"):
        held = []
        for times in (1, 8):
            data = wrap(ref.text * times, how)
            got = ctx.census_reads(put(data), flags())
            st = ctx.last_stream_stats()
            assert got[:3] == (times * len(ref.names), times * int(ref.lens.sum()), times * len(ref.text)), (how, times)
            assert st[3] == 1 and st[1] == len(data) and st[2] <= pinned_bound(4096, largest_member(data, how)), (how, times, st)
            held.append(st[2])
        assert held[0] == held[1], (how, held)
    dr = ctx.open_reads(put(wrap(ref.text, "gzip_blocks")), flags())
    assert ctx.last_stream_stats()[3] == 1
    dr.free()


def same_verdict(ctx, put, data, fl_extra=0):
    """the whole-file call refuses, and the streamed call returns its code and its message"""
    path = put(data)
    whole = outcome(lambda: ctx.open_reads(path, flags(fl_extra, stream=False)))
    got = outcome(lambda: ctx.open_reads(path, flags(fl_extra)))
    assert whole[0] != "ok", whole
    assert got == whole, (got, whole)
    upload_still_works(ctx)
    return whole


def test_same_verdicts(ctx, knobs, put):
    from lrge_amd import _ffi
    aln = _ffi.GPU_INGEST_WINDOWED_ALN
    # records the scan does not prove, through windows of 64 bytes
    set_knobs(knobs, 64, 509)
    for data, extra, why in RECORD_REFUSALS:
        fl = aln | sum(getattr(_ffi, "GPU_" + n) for n in extra)
        for wrapped in (data, bgzf(data)[0], G.gz(data)):
            code, msg = same_verdict(ctx, put, wrapped, fl)
            assert code == _ffi.ERR_UNPROVEN and why in msg, msg
    # a BGZF block that fails its CRC
    code, msg = same_verdict(ctx, put, bgzf_bad_second(FQ))
    assert code == _ffi.ERR_UNPROVEN and msg.endswith("reads_open: a BGZF block failed its checks"), msg
    # a damaged gzip stream
    gz = G.gz(FQ)
    code, msg = same_verdict(ctx, put, flipped(gz, len(gz) // 2))
    assert code == _ffi.ERR_UNPROVEN and "gzip data not proven on the device" in msg, msg
    # bases and window above the cap
    knobs.set("INGEST_MAX_BYTES", sum(LENS) - 1)
    for data in (FQ, bgzf(FQ)[0]):
        code, msg = same_verdict(ctx, put, data)
        assert code == _ffi.ERR_UNPROVEN and "bases and window above INGEST_MAX_BYTES" in msg, msg
    # text above the cap (a window above the text: the whole-file route would keep it resident)
    set_knobs(knobs, 1 << 20, 509)
    knobs.set("INGEST_MAX_BYTES", len(FQ) - 1)
    for data in (FQ, bgzf(FQ)[0], G.gz(FQ)):
        code, msg = same_verdict(ctx, put, data)
        assert code == _ffi.ERR_UNPROVEN and msg.endswith("reads_open: text above INGEST_MAX_BYTES (%d)" % (len(FQ) - 1)), msg


def test_the_documented_difference(ctx, knobs, put):
    """BGZF blocks followed by a plain gzip member: the whole-file route decodes the file as gzip; the streamed call has delivered
    windows by then and refuses, naming the file offset of the member that is no BGZF block"""
    from lrge_amd import _ffi
    set_knobs(knobs, 3001, 509)
    half = FQ.index(b"@read5\n")
    head = b"".join(W.bgzf_block(FQ[i:min(i + 1000, half)]) for i in range(0, half, 1000))
    data = head + G.gz(FQ[half:])
    path = put(data)
    dr = ctx.open_reads(path, flags(stream=False))
    assert dr.n == len(LENS) and dr.lens.tolist() == LENS
    dr.free()
    for call in (lambda: ctx.open_reads(path, flags()), lambda: ctx.census_reads(path, flags())):
        with pytest.raises(_ffi.UnprovenInput) as ei:
            call()
        assert ei.value.code == _ffi.ERR_UNPROVEN and "file offset %d " % len(head) in str(ei.value) and "without LRGE_GPU_INGEST_STREAM" in str(ei.value), str(ei.value)
    upload_still_works(ctx)


def test_io_and_flag_errors(ctx, knobs, put, tmp_path):
    from lrge_amd import _ffi
    set_knobs(knobs, 3001, 509)
    calls = (lambda p, f: ctx.open_reads(p, f), lambda p, f: ctx.census_reads(p, f), lambda p, f: ctx.open_reads_selected(p, [0], f),
             lambda p, f: ctx.census_map_reads(p, f))
    for path in (str(tmp_path / "there_is_no_such_file.fq"), str(tmp_path)):
        for call in calls:
            code, msg = outcome(lambda: call(path, flags()))
            assert code == _ffi.ERR_IO, (path, code, msg)
    empty = put(b"", "empty.fq")
    for call in calls[:2]:
        a, b = outcome(lambda: call(empty, flags(stream=False))), outcome(lambda: call(empty, flags()))
        if a[0] == "ok" and not isinstance(a[1], tuple):
            assert b[0] == "ok" and a[1].n == b[1].n == 0
            a[1].free(); b[1].free()
        else:
            assert a == b, (a, b)
    path = put(FQ)
    code, msg = outcome(lambda: ctx.open_reads(path, flags() & ~_ffi.GPU_INGEST_WINDOWED))
    assert code == _ffi.ERR_INVALID and "LRGE_GPU_INGEST_STREAM" in msg and "LRGE_GPU_INGEST_WINDOWED" in msg, (code, msg)
    # the _mem forms accept and ignore the flag
    dr = ctx.open_reads(FQ, flags() & ~_ffi.GPU_INGEST_WINDOWED)
    assert dr.n == len(LENS) and dr.window_stats() == (0, 0, 0, 0)
    dr.free()
    assert ctx.census_reads(FQ, flags())[:3] == (len(LENS), sum(LENS), len(FQ))
    upload_still_works(ctx)


@pytest.mark.parametrize("more", [[], ["--gpu-sample", "--gpu-seek"]])
def test_cli_stream_prints_the_same_estimate(tmp_path, more):
    """lrge-hip --gpu-ingest --gpu-stream [--gpu-sample --gpu-seek] prints the estimate that the same line without --gpu-stream prints"""
    from lrge_amd import build as Bd
    src = tmp_path / "toy_reads.fa.gz"
    shutil.copy(os.path.join(HERE, "golden", "toy_reads.fa.gz"), src)
    cmd = [Bd.CLI_PATH, str(src), "-T", "300", "-Q", "100", "-s", "1", "--gpu-ingest"] + more
    a = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    b = subprocess.run(cmd + ["--gpu-stream"], capture_output=True, text=True, timeout=300)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == b.stdout and a.stdout.strip(), (a.stdout, b.stdout)
    info = lambda s: [ln for ln in s.splitlines() if "gpu-ingest:" in ln or ln.startswith("[WARN]")]   # noqa: E731
    assert info(a.stderr) == info(b.stderr) and "gpu-ingest: device" in b.stderr, (a.stderr, b.stderr)


def test_cli_stream_requires_ingest(tmp_path):
    from lrge_amd import build as Bd
    src = tmp_path / "toy_reads.fa.gz"
    shutil.copy(os.path.join(HERE, "golden", "toy_reads.fa.gz"), src)
    r = subprocess.run([Bd.CLI_PATH, str(src), "--gpu-stream"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "error: the argument '--gpu-stream' requires '--gpu-ingest'" in r.stderr, r.stderr
