"""The base blocks of unaligned CRAM decoded on the device (k_rans_decode): Context.rans_decode over the stream cases of
tests/cram_corpus.py against the writer's plain bytes and the host twin (statuses and stats field for field), read sets opened with
GPU_INGEST_CRAM against the host reader, every refusal by its reason, calls without the flag, the CLI.  The largest file holds
200 KB of bases."""
import os
import random
import subprocess

import numpy as np
import pytest

import cram_corpus as K
import cram_writer as CW
from test_cram_twin import STAT_KEYS, STATUS, damage_cases, load_twin, twin_decode, twin_open
from test_gpu_ingest import check_seqset, read_host, upload_still_works

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TODAY = "reads_open: not proven on the device (neither FASTA nor FASTQ by its first line)"     # what a CRAM gets without the flag


@pytest.fixture(scope="module")
def twin():
    from lrge_amd import build as B
    return load_twin(B.build_cram_twin())


def cram_flags():
    from lrge_amd import _ffi
    return _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INGEST_CRAM


def test_streams_statuses_and_stats_equal_the_twin(ctx, twin):
    cases = K.stream_cases()
    items = [(m, comp, len(plain)) for _, m, comp, plain in cases]
    outs, status, st = ctx.rans_decode(items)                           # one batch of all
    out_t, status_t, st_t, _ = twin_decode(twin, items)
    assert status == status_t == [0] * len(cases), [(cases[i][0], s) for i, s in enumerate(status) if s][:5]
    for (name, _, _, plain), got in zip(cases, outs):
        assert got == plain, name
    assert b"".join(outs) == out_t
    assert [st[k] for k in STAT_KEYS] == [st_t[k] for k in STAT_KEYS], (st, st_t)
    assert st["rounds"] == 1 and st["global_table_blocks"] >= 3
    for name, m, comp, plain in cases[::5]:                             # one block a call
        outs1, status1, st1 = ctx.rans_decode([(m, comp, len(plain))])
        assert status1 == [0] and outs1 == [plain] and st1["rounds"] == 1, name


def test_stream_rounds_refusals_and_damage_equal_the_twin(ctx, twin, knobs):
    cases = K.stream_cases()
    knobs.set("CRAM_ROUND_BYTES", 1)                                    # every block a round of its own
    items = [(m, comp, len(plain)) for _, m, comp, plain in cases[:60]]
    outs, status, st = ctx.rans_decode(items)
    assert status == [0] * 60 and st["rounds"] == 60 and outs == [c[3] for c in cases[:60]]
    knobs.unset("CRAM_ROUND_BYTES")
    good = cases[100]
    refused = K.refused_streams()
    items = [(good[1], good[2], len(good[3]))] + [(m, body, raw) for _, m, body, raw, _ in refused] + [(good[1], good[2], len(good[3]))]
    outs, status, st = ctx.rans_decode(items)
    assert status == [0] + [STATUS["head"]] * len(refused) + [0] and outs[0] == outs[-1] == good[3]
    assert "STRIPE" in ctx.rans_why and all(o == bytes(len(o)) for o in outs[1:-1])
    # single-byte flips inside stream bodies: the device's status words and bytes are the twin's
    rng = random.Random(5)
    items = []
    for name in ("rans0_n4097_a4", "rans1_n4097_a17", "nx16_o0_n4097_a4", "nx16_o1_n4097_a17", "nx16_o1x32_n4097_a4", "nx16_packrle_n4097_a4", "nx16_rle_cm_n4097_a4",
                 "nx16_o1_n4097_a256", "nx16_cat_n129_a5"):
        _, m, comp, plain = next(c for c in cases if c[0] == name)
        for _ in range(12):
            at = rng.randrange(len(comp))
            items.append((m, comp[:at] + bytes([comp[at] ^ (1 << rng.randrange(8))]) + comp[at + 1:], len(plain)))
    outs, status, st = ctx.rans_decode(items)
    out_t, status_t, st_t, _ = twin_decode(twin, items)
    assert status == status_t and len(set(status)) >= 4, (status, status_t)
    o = 0
    for (m, comp, raw), got, s in zip(items, outs, status):
        if s == 0:
            assert got == out_t[o:o + raw]
        o += raw
    assert [st[k] for k in STAT_KEYS] == [st_t[k] for k in STAT_KEYS]
    upload_still_works(ctx)


def test_open_reads_from_cram(ctx, tmp_path, knobs, twin):
    knobs.set("CRAM_MIN_BLOCKS", 0)
    files = K.file_cases()
    rng = random.Random(3)
    for name, data in files:
        p = tmp_path / (name + ".cram")
        p.write_bytes(data)
        rc_h, rec_h, msg = read_host(p)
        assert rc_h == 0, (name, msg)
        seqs = [s for _, s in rec_h]
        _, _, st_t = twin_open(twin, data)
        for round_bytes in (0, 1):
            if round_bytes:
                knobs.set("CRAM_ROUND_BYTES", 1)                        # every block a round of its own
            else:
                knobs.unset("CRAM_ROUND_BYTES")
            for src in (data, str(p)):
                dr = ctx.open_reads(src, cram_flags())
                assert dr.n == len(rec_h) and dr.names == [n for n, _ in rec_h], name
                assert np.array_equal(dr.lens, np.array([len(s) for s in seqs], dtype=np.uint32)), name
                assert dr.text_bytes == sum(len(s) for s in seqs) and dr.window_stats()[0] == 0
                st = dr.cram_stats()
                blocks = st["ba_raw"] + st["ba_rans4x8"] + st["ba_ransnx16"]
                assert st["rounds"] == (blocks if round_bytes else min(1, blocks)) and st["records"] == dr.n and st["raw_bytes"] == dr.text_bytes, (name, st)
                if not round_bytes:
                    assert [st[k] for k in STAT_KEYS] == [st_t[k] for k in STAT_KEYS], (name, st, st_t)
                if dr.n and src is data:
                    check_seqset(ctx, dr, seqs, list(range(dr.n)), (name, round_bytes))
                    check_seqset(ctx, dr, seqs, [rng.randrange(dr.n) for _ in range(2 * dr.n)], (name, round_bytes, "shuffled"))
                dr.free()
    knobs.unset("CRAM_ROUND_BYTES")
    dr = ctx.open_reads(K.by_name("external_stop_q1_t1_spc3"), cram_flags())
    st = dr.cram_stats()
    assert (st["containers"], st["slices"], st["ba_rans4x8"], st["order1_blocks"], st["rounds"]) == (2, 4, 4, 4, 1), st
    dr.free()
    dr = ctx.open_reads(K.by_name("larger_200k"), cram_flags())
    st = dr.cram_stats()
    assert st["slices"] == 5 and st["ba_ransnx16"] == 5 and 150_000 < st["raw_bytes"] <= 200_000 and st["comp_bytes"] < st["raw_bytes"] // 2, st
    dr.free()
    fq = ctx.open_reads(b"@r\nACGT\n+\n!!!!\n", cram_flags())                # the flag changes nothing for other input
    assert fq.n == 1
    with pytest.raises(Exception):
        fq.cram_stats()                                                  # LRGE_ERR_INVALID: not CRAM
    fq.free()
    upload_still_works(ctx)


def test_refusals_name_their_reason(ctx, knobs):
    from lrge_amd import _ffi
    knobs.set("CRAM_MIN_BLOCKS", 0)
    for name, data, reason in K.refused_files():
        with pytest.raises(_ffi.UnprovenInput) as ei:
            ctx.open_reads(data, cram_flags())
        assert "reads_open: not proven on the device (" in str(ei.value) and (reason is None or reason in str(ei.value)), (name, str(ei.value))
    refused = 0
    for name, data in damage_cases()[::3]:                               # a damaged file: refused, or the host reader's bases
        try:
            dr = ctx.open_reads(data, cram_flags())
        except _ffi.UnprovenInput as e:
            assert "reads_open: not proven on the device (CRAM: " in str(e), (name, str(e))
            refused += 1
            continue
        dr.free()
    assert refused >= 8
    data = K.by_name("ba_rans1")
    for min_blocks in (5, None):                                         # None: the default, 32 (the file has 4)
        if min_blocks:
            knobs.set("CRAM_MIN_BLOCKS", min_blocks)
        else:
            knobs.unset("CRAM_MIN_BLOCKS")
        with pytest.raises(_ffi.UnprovenInput) as ei:
            ctx.open_reads(data, cram_flags())
        assert "fewer BA blocks than CRAM_MIN_BLOCKS" in str(ei.value)
    dr = ctx.open_reads(CW.write_cram(K.reads(32, 8, 1, 60), method="rans0", records_per_slice=1), cram_flags())    # 32 blocks: the default takes them
    assert dr.cram_stats()["ba_rans4x8"] == 32
    dr.free()
    knobs.set("CRAM_MIN_BLOCKS", 0)
    bases = sum(len(s) for _, s in K.reads(23, 1, zero_at=5))
    knobs.set("INGEST_MAX_BYTES", bases)                                 # the bases alone fit, a round beside them does not
    with pytest.raises(_ffi.UnprovenInput) as ei:
        ctx.open_reads(data, cram_flags())
    assert "reads_open: bases and one round above INGEST_MAX_BYTES (%d)" % bases in str(ei.value)
    knobs.set("INGEST_MAX_BYTES", 2 * bases)
    ctx.open_reads(data, cram_flags()).free()
    upload_still_works(ctx)


def test_without_the_flag_a_cram_is_refused_as_before(ctx):
    from lrge_amd import _ffi
    every_other = (_ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INFLATE_BZIP2 | _ffi.GPU_INFLATE_ZSTD | _ffi.GPU_INFLATE_XZ | _ffi.GPU_INGEST_BAM |
                   _ffi.GPU_INGEST_SAM | _ffi.GPU_INGEST_WINDOWED | _ffi.GPU_INGEST_WINDOWED_ALN)
    data = K.by_name("ba_rans1")
    for flags in (0, _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP, _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INFLATE_XZ, every_other):
        assert not flags & _ffi.GPU_INGEST_CRAM
        with pytest.raises(_ffi.UnprovenInput) as ei:
            ctx.open_reads(data, flags)
        assert TODAY in str(ei.value), (flags, str(ei.value))
    upload_still_works(ctx)


def test_cli_gpu_cram(tmp_path):
    from lrge_amd import build as B, readio
    tn, ts = readio.load(os.path.join(GOLDEN, "toy_reads.fa.gz"))
    recs, total = [], 0
    for n, s in zip(tn, ts):
        if total + len(s) > 200_000:
            break
        recs.append((n if isinstance(n, bytes) else n.encode(), s if isinstance(s, bytes) else bytes(s)))
        total += len(s)
    assert len(recs) >= 32                                               # (the default of CRAM_MIN_BLOCKS is 32 blocks: the CLI sets no options)
    p = tmp_path / "toy.cram"
    p.write_bytes(CW.write_cram(recs, method="gzip", records_per_slice=1, slices_per_container=8, method_for={"BA": "rans1"}))
    args = [B.CLI_PATH, str(p), "-T", "10", "-Q", "5", "-s", "1", "-f"]
    a = subprocess.run(args, capture_output=True, text=True, timeout=120)
    b = subprocess.run(args + ["--gpu-ingest", "--gpu-cram"], capture_output=True, text=True, timeout=120)
    d = subprocess.run(args + ["--gpu-ingest"], capture_output=True, text=True, timeout=120)
    assert a.returncode == 0 and b.returncode == 0 and d.returncode == 0, (a.stderr, b.stderr, d.stderr)
    assert a.stdout == b.stdout == d.stdout and a.stdout.strip()
    assert "gpu-ingest: device" in b.stderr and "gpu-ingest: host" in d.stderr      # --gpu-ingest alone: CRAM stays with the host, as before
