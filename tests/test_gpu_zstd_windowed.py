"""The windowed and the sampled device ingest of Zstandard (LRGE_GPU_INGEST_WINDOWED_ZSTD; k_zs_xxh64_part, k_zs_slide; DESIGN section
26): the sliding decoder keeps a work text [history | round] instead of the whole text, every finished round passes through the
windows.  Against the resident open, the host reader and the sliding host twin (its statistics field for field); a text above
INGEST_MAX_BYTES that is taken only with the flag; census, selected and mapped opens against the same calls on the plain text;
refusals; the CLI.  The shapes are small: a 72 000-byte text in 71 blocks of 1 KiB (window_log 10) or 18 of 4 KiB (window_log 12),
three frames of 30 KB, blocks of 300 bytes in a 1 KiB window (the history overlaps its destination when it moves)."""
import os
import subprocess

import numpy as np
import pytest

import bgzf_writer as W
import zstd_corpus as Z
import zstd_writer as ZW
from test_gpu_ingest import check_seqset, read_host, upload_still_works
from test_gpu_zstd import inflate_flags, three_frames
from test_zstd_slide_twin import load_slide_twin, run_sliding, small_window_text

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCK_MAX = 1 << 17


@pytest.fixture(scope="module")
def ztwin():
    from lrge_amd import build as B
    return load_slide_twin(B.build_zstd_twin())


def slide_flags():
    from lrge_amd import _ffi
    return inflate_flags() | _ffi.GPU_INGEST_WINDOWED | _ffi.GPU_INGEST_WINDOWED_ZSTD


class Host:
    """the host reader's records of a text, read once"""

    def __init__(self, path, text):
        path.write_bytes(text)
        rc, rec, msg = read_host(path)
        assert rc == 0 and len(rec) > 100, msg
        self.text, self.names, self.seqs = text, [n for n, _ in rec], [s for _, s in rec]
        self.lens = np.array([len(s) for s in self.seqs], dtype=np.uint32)
        self.n, self.bases = len(rec), int(self.lens.sum())


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    return Host(tmp_path_factory.mktemp("zstd_windowed") / "small.fq", small_window_text())


def small_blocks_frame(text):
    """`text` as raw blocks of 300 bytes in a frame with a window of 1 KiB: from the fifth block on the history (1024 bytes) is
    longer than the round in front of it, so it moves to the front over itself"""
    f = ZW.Frame(window_log=10)
    for at in range(0, len(text), 300):
        f.raw(text[at:at + 300])
    return f.bytes()


def test_windowed_open_equals_the_resident_open_and_the_twin(ctx, knobs, ztwin, small, tmp_path):
    window = 50_000
    knobs.set("INGEST_WINDOW_BYTES", window)
    multi, fq3 = three_frames()
    part = small.text[:60_000 + small.text[60_000:].index(b"\n@read") + 1]
    cases = [("window_log_10", Z.compress(small.text, 3, window_log=10), small), ("window_log_12", Z.compress(small.text, 3, window_log=12), small),
             ("three_frames", multi, Host(tmp_path / "three.fq", fq3)), ("blocks_of_300", small_blocks_frame(part), Host(tmp_path / "part.fq", part))]
    for name, comp, host in cases:
        ref = ctx.open_reads(comp, inflate_flags())
        assert ref.window_stats()[0] == 0 and ref.zstd_stats() == (0, 0, 0, 0), name
        assert ref.n == host.n and ref.names == host.names and np.array_equal(ref.lens, host.lens), name
        ref.free()
        for round_blocks in (1, 2, 0):
            if round_blocks:
                knobs.set("ZSTD_ROUND_BLOCKS", round_blocks)
            else:
                knobs.unset("ZSTD_ROUND_BLOCKS")
            dr = ctx.open_reads(comp, slide_flags())
            assert dr.window_stats()[0] > 1, (name, round_blocks, dr.window_stats())
            assert dr.n == host.n and dr.text_bytes == len(host.text) and dr.names == host.names and np.array_equal(dr.lens, host.lens), (name, round_blocks)
            # the default round keeps a round's text within the window: one block here
            rc, out, _, _, sl = run_sliding(ztwin, comp, round_blocks or max(1, window // BLOCK_MAX))
            assert rc == 0 and out == host.text and dr.zstd_stats() == sl, (name, round_blocks, dr.zstd_stats(), sl)
            check_seqset(ctx, dr, host.seqs, list(range(dr.n)), (name, round_blocks))
            dr.free()
    assert run_sliding(ztwin, cases[3][1], 1)[4][1] == 1024


def test_text_above_the_cap_is_taken_only_with_the_flag(ctx, knobs, ztwin, small):
    from lrge_amd import _ffi
    comp = Z.compress(small.text, 3, window_log=10)
    window = 8_000
    knobs.set("INGEST_WINDOW_BYTES", window)
    _, _, _, _, sl = run_sliding(ztwin, comp, 1)
    # the store holds the bases; the window block starts at two windows and needs no more (a round adds 1 KiB to less than a window);
    # the work block is the twin's largest work text and the 64 bytes of padding the decoder allocates behind it
    cap = small.bases + 2 * window + sl[2] + 64
    assert cap < len(small.text), (cap, len(small.text))
    knobs.set("INGEST_MAX_BYTES", cap)
    print("INGEST_MAX_BYTES %d: bases %d, two windows %d, work text %d; text %d" % (cap, small.bases, 2 * window, sl[2], len(small.text)))
    dr = ctx.open_reads(comp, slide_flags())
    assert dr.n == small.n and dr.text_bytes == len(small.text) and dr.names == small.names and np.array_equal(dr.lens, small.lens)
    assert dr.window_stats()[0] > 1 and dr.window_stats()[1] == small.bases and dr.zstd_stats() == sl
    check_seqset(ctx, dr, small.seqs, list(range(dr.n)), "above the cap")
    dr.free()
    for flags in (inflate_flags(), inflate_flags() | _ffi.GPU_INGEST_WINDOWED, inflate_flags() | _ffi.GPU_INGEST_WINDOWED_ZSTD):
        with pytest.raises(_ffi.UnprovenInput) as ei:
            ctx.open_reads(comp, flags)
        assert "reads_open: text above INGEST_MAX_BYTES (%d)" % cap in str(ei.value), (flags, str(ei.value))
    # a cap the work block alone does not fit in: the same refusal
    knobs.set("INGEST_MAX_BYTES", sl[2])
    with pytest.raises(_ffi.UnprovenInput) as ei:
        ctx.open_reads(comp, slide_flags())
    assert "reads_open: text above INGEST_MAX_BYTES (%d)" % sl[2] in str(ei.value), str(ei.value)
    upload_still_works(ctx)


def test_sampled_calls_equal_those_on_the_plain_text(ctx, knobs, small):
    from lrge_amd import _ffi
    knobs.set("INGEST_WINDOW_BYTES", 20_000)
    knobs.set("INGEST_SEEK_STRIDE_BYTES", 4096)
    fl = inflate_flags() | _ffi.GPU_INGEST_WINDOWED_ZSTD
    rng = np.random.default_rng(26)
    sels = {"first and last": [0, small.n - 1], "random quarter": sorted(rng.permutation(small.n)[:small.n // 4].tolist()), "none": []}
    for name, comp in (("window_log_10", Z.compress(small.text, 3, window_log=10)), ("three_frames", three_frames()[0])):
        text = Z.decompress(comp)
        host_n = small.n if text == small.text else text.count(b"\n") // 4
        plain = ctx.census_reads(text, fl)
        got = ctx.census_reads(comp, fl)
        assert got[:3] == plain[:3] and got[0] == host_n and got[2] == len(text) and got[3] > 1, (name, got, plain)
        counts_p, map_p = ctx.census_map_reads(text, fl)
        counts_z, map_z = ctx.census_map_reads(comp, fl)
        assert counts_z[:3] == counts_p[:3] == plain[:3], (name, counts_z, counts_p)
        for what, sel in sels.items():
            sel = [i for i in sel if i < host_n]
            a = ctx.open_reads_selected(text, sel, fl)
            for how, b in (("selected", ctx.open_reads_selected(comp, sel, fl)), ("mapped", ctx.open_reads_mapped(comp, map_z, sel, fl))):
                assert b.n == a.n == len(sel) and b.names == a.names and np.array_equal(b.lens, a.lens) and b.text_bytes == a.text_bytes, (name, what, how)
                assert b.select_stats() == a.select_stats(), (name, what, how, b.select_stats(), a.select_stats())
                assert b.zstd_stats()[0] > 1 and a.zstd_stats() == (0, 0, 0, 0), (name, what, how)
                if text == small.text and sel:
                    assert b.names == [small.names[i] for i in sel]
                    check_seqset(ctx, b, [small.seqs[i] for i in sel], list(range(len(sel))), (name, what, how))
                b.free()
            m = ctx.open_reads_mapped(text, map_p, sel, fl)
            assert m.names == a.names and m.select_stats() == a.select_stats(), (name, what)
            m.free()
            a.free()
        map_p.free()
        map_z.free()
    # without the flag: the refusal of before, word for word
    comp = Z.compress(small.text, 3, window_log=10)
    for call in (lambda f: ctx.census_reads(comp, f), lambda f: ctx.open_reads_selected(comp, [0], f), lambda f: ctx.census_map_reads(comp, f)):
        for flags in (inflate_flags(), inflate_flags() | _ffi.GPU_INGEST_WINDOWED, (inflate_flags() | _ffi.GPU_INGEST_WINDOWED_ZSTD) & ~_ffi.GPU_INFLATE_ZSTD):
            with pytest.raises(_ffi.UnprovenInput) as ei:
                call(flags)
            want = "selected ingest takes FASTA / FASTQ only, not Zstandard input" if flags & _ffi.GPU_INFLATE_ZSTD else "bzip2, zstd and xz input is decompressed on the host"
            assert want in str(ei.value), (flags, str(ei.value))
    upload_still_works(ctx)


def test_refusals(ctx, knobs, small):
    from lrge_amd import _ffi
    comp = Z.compress(small.text, 3, window_log=10)
    knobs.set("INGEST_WINDOW_BYTES", 50_000)
    knobs.set("ZSTD_ROUND_BLOCKS", 30)                               # 71 blocks: the frame spans three rounds
    dr = ctx.open_reads(comp, slide_flags())
    assert dr.zstd_stats()[0] == 3 and dr.n == small.n
    dr.free()
    wrong = comp[:-2] + bytes([comp[-2] ^ 0x10]) + comp[-1:]
    for call in (lambda d: ctx.open_reads(d, slide_flags()), lambda d: ctx.census_reads(d, slide_flags())):
        with pytest.raises(_ffi.UnprovenInput) as ei:
            call(wrong)
        assert "zstd data not accepted by the device (content checksum mismatch" in str(ei.value), str(ei.value)
        upload_still_works(ctx)
        with pytest.raises(_ffi.UnprovenInput) as ei:
            call(comp[:-20])                                          # the last block is cut short
        assert "zstd data not accepted by the device (" in str(ei.value), str(ei.value)
        upload_still_works(ctx)
    knobs.set("ZSTD_CHECKSUM", 0)
    dr = ctx.open_reads(wrong, slide_flags())
    assert dr.n == small.n
    dr.free()


def test_cli_sampled_zstd(tmp_path):
    from lrge_amd import build as B, readio
    tn, ts = readio.load(os.path.join(GOLDEN, "toy_reads.fa.gz"))
    p = tmp_path / "toy.fq.zst"
    p.write_bytes(Z.compress(W.fastq_bytes(tn, ts)))
    args = [B.CLI_PATH, str(p), "-T", "300", "-Q", "100", "-s", "6", "-f"]
    runs = {k: subprocess.run(args + extra, capture_output=True, text=True, timeout=300)
            for k, extra in (("host", []), ("device", ["--gpu-ingest", "--gpu-zstd"]), ("sampled", ["--gpu-ingest", "--gpu-zstd", "--gpu-sample"]),
                             ("seek", ["--gpu-ingest", "--gpu-zstd", "--gpu-sample", "--gpu-seek"]), ("no zstd", ["--gpu-ingest", "--gpu-sample"]))}
    assert all(r.returncode == 0 for r in runs.values()), {k: r.stderr for k, r in runs.items()}
    assert len({r.stdout for r in runs.values()}) == 1 and runs["host"].stdout.strip(), {k: r.stdout for k, r in runs.items()}
    assert "gpu-ingest: device\n" in runs["device"].stderr and "gpu-ingest: device (sampled)\n" in runs["sampled"].stderr, (runs["device"].stderr, runs["sampled"].stderr)
    assert "gpu-ingest: device (sampled, seek)\n" in runs["seek"].stderr and "gpu-ingest: host" in runs["no zstd"].stderr, (runs["seek"].stderr, runs["no zstd"].stderr)
