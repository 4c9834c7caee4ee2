"""The corpus of the xz tests: FASTQ / FASTA / random / highly repetitive texts through liblzma (Python's lzma) at several presets,
lc / lp / pb and dictionary sizes, cut into blocks by tests/xz_writer.py; one text of 300 KB in ONE block (three chunks or more, so
a block crosses launches); incompressible stretches (uncompressed chunks); multi-stream files with and without padding."""
import lzma
import random

import xz_writer as XW
from bzip2_corpus import fastq, noise

E_NAMES = ("OK", "MAGIC", "INPUT", "FOOTER", "RESERVED", "CHECK_ID", "HEADER_CRC", "FLAGS", "INDEX", "FILTER", "PADDING", "SIZES", "CONTROL", "PROPS", "DICT_SIZE",
           "DIST", "END_MARKER", "MATCH_CROSS", "RC", "CHECK", "FEW_BLOCKS", "TOO_BIG")       # xz_core.h


def fasta(n_bytes, seed):
    rng = random.Random(seed)
    out, size, i = [], 0, 0
    while size < n_bytes:
        seq = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(100, 3000)))
        rec = b">contig%d len=%d\n" % (i, len(seq)) + b"\n".join(seq[k:k + 60] for k in range(0, len(seq), 60)) + b"\n"
        out.append(rec); size += len(rec); i += 1
    return b"".join(out)


def decompress(data):
    """what liblzma gives for the whole of `data` with LZMA_CONCATENATED, every stream and the padding between them (lzma.decompress
    stops at stream padding: the streams are decoded one by one), or None where it reports an error or the data ends early"""
    out = []
    try:
        while True:
            d = lzma.LZMADecompressor(format=lzma.FORMAT_XZ)
            out.append(d.decompress(data))
            if not d.eof:
                return None
            data = d.unused_data
            pad = len(data) - len(data.lstrip(b"\0"))
            if not data[pad:]:
                return b"".join(out) if pad % 4 == 0 else None
            if pad % 4:
                return None
            data = data[pad:]
    except lzma.LZMAError:
        return None


def one_block_text():
    return fastq(300_000, 41)


_CASES = None


def cases():
    """(name, xz bytes, plain bytes); computed once"""
    global _CASES
    if _CASES is not None:
        return _CASES
    r23 = random.Random(23)
    fq, fa, rnd = fastq(400_000, 21), fasta(120_000, 22), bytes(r23.getrandbits(8) for _ in range(90_000))
    rep = (b"ACGTACGTTTGACCA" * 50 + b"\n") * 300
    out = []
    for preset, nm in ((0, "p0"), (1, "p1"), (6, "p6"), (9, "p9"), (9 | lzma.PRESET_EXTREME, "p9e")):
        out.append(("fastq_" + nm, XW.xz_of(fq, 130_000, XW.CHECK_CRC64, preset=preset), fq))
    for lc, lp, pb in ((0, 0, 0), (4, 0, 2), (0, 4, 4), (2, 2, 0)):
        out.append(("fasta_lc%d_lp%d_pb%d" % (lc, lp, pb), XW.xz_of(fa, 50_000, XW.CHECK_CRC32, sizes=False, lc=lc, lp=lp, pb=pb), fa))
    out.append(("fastq_dict_4k", XW.xz_of(fq[:200_000], 200_000, XW.CHECK_CRC32, dict_size=4096), fq[:200_000]))
    out.append(("fastq_dict_1m", XW.xz_of(fq, 200_000, XW.CHECK_NONE, dict_size=1 << 20), fq))
    out.append(("repetitive", XW.xz_of(rep, 100_000, XW.CHECK_CRC64), rep))
    out.append(("random_bytes", XW.xz_of(rnd, 60_000, XW.CHECK_CRC32), rnd))
    mixed = fq[:80_000] + rnd[:70_000] + fa[:50_000] + rnd[70_000:] + rep[:30_000]
    out.append(("incompressible_stretches", XW.xz_of(mixed, 150_000, XW.CHECK_CRC64), mixed))
    one = one_block_text()
    out.append(("one_block_300k", XW.xz_of(one, len(one), XW.CHECK_CRC64, preset=1), one))
    a, b, c = XW.xz_of(fq[:100_000], 60_000), XW.xz_of(fa[:50_000], 50_000, XW.CHECK_CRC64, sizes=False), lzma.compress(fq[100_000:150_000])
    out.append(("three_streams", a + b + c, fq[:100_000] + fa[:50_000] + fq[100_000:150_000]))
    out.append(("three_streams_padded", a + b"\0" * 4 + b + b"\0" * 16 + c + b"\0" * 8, fq[:100_000] + fa[:50_000] + fq[100_000:150_000]))
    out.append(("python_default", lzma.compress(fa), fa))
    _CASES = out
    return out


def by_name(name):
    return next(c for c in cases() if c[0] == name)


# ---- the walker (of files that are well formed) ----
def _vli(d, p):
    v = s = 0
    while True:
        b = d[p]; p += 1
        v |= (b & 0x7F) << s; s += 7
        if not b & 0x80:
            return v, p


def walk(data):
    """{streams, blocks, chunks, raw_chunks, checks, per_block: [chunks], chunk_at: [(control byte offset, payload offset, control)], check_at: [...]}"""
    st = dict(streams=0, blocks=0, chunks=0, raw_chunks=0, checks=0, per_block=[], chunk_at=[], check_at=[], block_at=[], index_at=[])
    e, streams = len(data), []
    while e > 0:
        while e >= 4 and data[e - 4:e] == b"\0\0\0\0":
            e -= 4
        if e == 0:
            break
        assert data[e - 2:e] == b"YZ"
        check = data[e - 3]
        isize = (int.from_bytes(data[e - 8:e - 4], "little") + 1) * 4
        ia = e - 12 - isize
        count, p = _vli(data, ia + 1)
        recs = []
        for _ in range(count):
            u, p = _vli(data, p)
            n, p = _vli(data, p)
            recs.append((u, n))
        at = ia - sum((u + 3) & ~3 for u, _ in recs) - 12
        streams.append((at, ia, check, recs))
        e = at
    for at, ia, check, recs in reversed(streams):
        st["streams"] += 1
        st["index_at"].append(ia)
        p = at + 12
        csz = {0: 0, 1: 4, 4: 8, 10: 32}[check]
        for u, n in recs:
            hs = (data[p] + 1) * 4
            q, end, k = p + hs, p + u - csz, 0
            st["block_at"].append(p)
            while data[q]:
                c = data[q]
                if c >= 0x80:
                    cs = int.from_bytes(data[q + 3:q + 5], "big") + 1
                    h = 6 if c >= 0xC0 else 5
                else:
                    cs = int.from_bytes(data[q + 1:q + 3], "big") + 1
                    h = 3
                    st["raw_chunks"] += 1
                st["chunk_at"].append((q, q + h, c))
                q += h + cs; k += 1
            assert q + 1 == end
            st["chunks"] += k; st["per_block"].append(k); st["blocks"] += 1
            st["checks"] += 1 if csz and check != 10 else 0
            st["check_at"].append(p + ((u + 3) & ~3) - csz)
            p += (u + 3) & ~3
    return st
