"""The refusals of the device ingest (lrge_hip_reads_open_mem, host_fastx.inl): for every refusal that input and options alone
reach, the exact return code and the exact text of lrge_hip_last_error.  The texts are literals taken from the source as it
stood before the ingest's host code was split into sources, sink and sniff: the file is meant to pass unmodified against a
library built from that commit (LRGE_HIP_LIB_AB), which makes it a pin of the messages and not a description of the new code.
Numbers in a message are the option the test sets; the status and offset of the corrupt gzip member and bzip2 stream are what
the host twins of the two decoders (the same round drivers) give on these bytes.  After every refusal the context still
uploads and sketches."""
import bz2
import random

import pytest

import bam_corpus as B
import bgzf_writer as W
import fastx_corpus as F
import gzip_corpus as G
import sam_corpus as S
from test_gpu_ingest_windowed import upload_still_works

pytestmark = pytest.mark.gpu

_rng = random.Random(11)
LENS = [2000 - 200 * i for i in range(10)]                   # the longest first: the block of the windows has its size early
READS = [(b"read%d" % i, bytes(_rng.choice(b"ACGT") for _ in range(n))) for i, n in enumerate(LENS)]
FQ = F.fastq_text(READS)
FA = F.fasta_text(READS, 60)
BAM = B.bam([B.record(n, s) for n, s in READS])
SAM = S.toy_sam([n for n, _ in READS], [s for _, s in READS])
UNPROVEN = -10


def fl(*names):
    from lrge_amd import _ffi
    return sum(getattr(_ffi, "GPU_" + n) for n in names)


def inflate():
    return fl("INFLATE_BGZF", "INFLATE_GZIP", "INFLATE_BZIP2")


def bgzf(text, block=1000, first=None):
    """(file, the offset of every block): blocks of `block` text bytes behind an optional first one of `first` bytes"""
    cuts = ([0, first] if first else [0]) + list(range((first or 0) + block, len(text), block)) + [len(text)]
    blocks = [W.bgzf_block(text[a:b]) for a, b in zip(cuts, cuts[1:])] + [W.EOF_BLOCK]
    offs = [sum(len(x) for x in blocks[:i]) for i in range(len(blocks))]
    return b"".join(blocks), offs


def flipped(data, at):
    return data[:at] + bytes([data[at] ^ 0xFF]) + data[at + 1:]


def bgzf_bad_second(text, first=None):
    """one payload byte of the second block flipped (a block is 18 bytes of header, the payload, 8 bytes of CRC32 and ISIZE)"""
    data, offs = bgzf(text, first=first)
    return flipped(data, (offs[1] + 18 + offs[2] - 8) // 2)


def refused(ctx, data, flags, msg, code=UNPROVEN):
    from lrge_amd import _ffi
    with pytest.raises(_ffi.LrgeHipError) as ei:
        ctx.open_reads(data, flags)
    assert ei.value.code == code and str(ei.value) == "lrge_hip error %d: %s" % (code, msg), (str(ei.value), msg)
    upload_still_works(ctx)


def test_text_above_the_cap(ctx, knobs):
    cap = len(FQ) - 1
    knobs.set("INGEST_MAX_BYTES", cap)
    for data in (FQ, bgzf(FQ)[0], G.gz(FQ), bz2.compress(FQ, 1)):
        refused(ctx, data, inflate(), "reads_open: text above INGEST_MAX_BYTES (%d)" % cap)


def test_bases_and_window_above_the_cap(ctx, knobs):
    cap = sum(LENS) - 1
    knobs.set("INGEST_WINDOW_BYTES", 64)
    knobs.set("INGEST_MAX_BYTES", cap)
    for data in (FQ, bgzf(FQ)[0]):
        refused(ctx, data, inflate() | fl("INGEST_WINDOWED"), "reads_open: bases and window above INGEST_MAX_BYTES (%d)" % cap)


def test_sources_left_to_the_host(ctx):
    refused(ctx, bgzf(FQ)[0], fl("INFLATE_GZIP"), "reads_open: BGZF input without LRGE_GPU_INFLATE_BGZF")
    refused(ctx, G.gz(FQ), fl("INFLATE_BGZF"), "reads_open: gzip input without LRGE_GPU_INFLATE_GZIP")
    for data in (bz2.compress(FQ, 1), b"\x28\xb5\x2f\xfd" + FQ[:200], b"\xfd7zXZ\x00" + FQ[:200]):
        refused(ctx, data, fl("INFLATE_BGZF", "INFLATE_GZIP"), "reads_open: bzip2, zstd and xz input is decompressed on the host")


def test_bgzf_block_that_fails_its_checks(ctx, knobs):
    msg = "reads_open: a BGZF block failed its checks"
    refused(ctx, bgzf_bad_second(FQ), inflate(), msg)
    knobs.set("INGEST_WINDOW_BYTES", 64)
    refused(ctx, bgzf_bad_second(FQ), inflate() | fl("INGEST_WINDOWED"), msg)
    # a first block of two text bytes: the sniff for BAM decodes two blocks, and meets the bad one
    refused(ctx, bgzf_bad_second(FQ, first=2), inflate() | fl("INGEST_WINDOWED", "INGEST_BAM"), msg)


def test_gzip_and_bzip2_streams_that_fail(ctx):
    gz, bz = G.gz(FQ), bz2.compress(FQ, 1)
    refused(ctx, flipped(gz, len(gz) // 2), inflate(), "reads_open: gzip data not proven on the device (status 5 near file offset 0)")
    refused(ctx, flipped(bz, len(bz) // 2), inflate(), "reads_open: bzip2 data not accepted by the device (a block above the level's block size near file offset 4)")


NOT_FASTX = b"neither a header nor a record line\n" * 20
_groups = FQ.split(b"\n+\n")
BAD_SEPARATOR = b"\n+\n".join(_groups[:4]) + b"\n-\n" + b"\n+\n".join(_groups[4:])      # (the fourth record's)
NINE_FIELDS = SAM + b"short\t4\t*\t0\t0\t*\t*\t0\t0\n"
TRUNCATED_BAM = BAM[:-5]
RECORD_REFUSALS = [
    (NOT_FASTX, (), "neither FASTA nor FASTQ by its first line"),
    (BAD_SEPARATOR, (), "a record outside the strict form"),
    (NINE_FIELDS, ("INGEST_SAM",), "a SAM record line outside the strict form"),
    (TRUNCATED_BAM, ("INGEST_BAM",), "the BAM record chain"),
]


def test_records_the_scan_does_not_prove(ctx, knobs):
    """resident, then through windows of 64 bytes (BAM and SAM with the flag that windows them)"""
    for data, extra, why in RECORD_REFUSALS:
        refused(ctx, data, inflate() | fl(*extra), "reads_open: not proven on the device (%s)" % why)
    knobs.set("INGEST_WINDOW_BYTES", 64)
    for data, extra, why in RECORD_REFUSALS:
        refused(ctx, data, inflate() | fl("INGEST_WINDOWED", "INGEST_WINDOWED_ALN", *extra), "reads_open: not proven on the device (%s)" % why)


def test_window_of_another_format(ctx, knobs):
    """FASTQ, then FASTA whose first sequence line is longer than a window: the block that holds the FASTA header and a part of
    that line is cut behind the last group of four lines, and the next window starts with the header.  (The other order is a
    FASTA file by the rules of the scan: the FASTQ lines are the last record's sequence.)"""
    knobs.set("INGEST_WINDOW_BYTES", 64)
    refused(ctx, FQ + F.fasta_text(READS, 3000), inflate() | fl("INGEST_WINDOWED"), "reads_open: not proven on the device (a window of another format than the first)")
    dr = ctx.open_reads(FA + FQ, inflate() | fl("INGEST_WINDOWED"))
    assert dr.n == len(READS) and dr.window_stats()[0] > 1
    dr.free()
