"""gzip inputs for the speculative-decode tests: every level and strategy, single and concatenated members, flushed streams,
headers with every optional field, BGZF, and the payloads of the BGZF corpus."""
import struct
import zlib

import bgzf_writer as W

STRATEGIES = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED]


def gz(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, memlevel=8):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, memlevel, strategy)
    return c.compress(data) + c.flush()


def gz_flushed(data, mode, step=3000, level=6):
    """one member with Z_SYNC_FLUSH / Z_FULL_FLUSH every `step` bytes"""
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    out = [c.compress(data[i:i + step]) + c.flush(mode) for i in range(0, len(data), step)]
    return b"".join(out) + c.flush()


def gz_header(data, fname=None, comment=None, extra=None, fhcrc=False, level=6, comp=None, crc=None, isize=None):
    """one member with the optional header fields.  comp: a ready-made raw deflate stream instead of zlib's; crc / isize:
    trailer fields other than those of `data` (for streams that are meant to be rejected)"""
    flg = (4 if extra is not None else 0) | (8 if fname is not None else 0) | (16 if comment is not None else 0) | (2 if fhcrc else 0)
    head = bytes([0x1f, 0x8b, 8, flg, 1, 2, 3, 4, 0, 3])
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    if fname is not None:
        head += fname + b"\0"
    if comment is not None:
        head += comment + b"\0"
    if fhcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + (W.deflate_raw(data, level) if comp is None else comp) + \
        struct.pack("<II", zlib.crc32(data) if crc is None else crc, (len(data) & 0xFFFFFFFF) if isize is None else isize)


def fastq(n=2000, seed=3):
    import random
    rng = random.Random(seed)
    names = [b"read%05d" % i for i in range(n)]
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(50, 400))) for _ in range(n)]
    return W.fastq_bytes(names, seqs)


def cases():
    """(name, gzip bytes, plain bytes)"""
    from test_bgzf_twin import payloads
    fq = fastq()
    out = []
    for level in (0, 1, 6, 9):
        for st in STRATEGIES:
            out.append(("fq_l%d_s%d" % (level, st), gz(fq, level, st), fq))
    pay = payloads()
    for name, d in pay.items():
        out.append(("pay_" + name, gz(d), d))
    allp = b"".join(pay.values())
    out.append(("pay_all_l9", gz(allp, 9), allp))
    out.append(("pay_all_multi", b"".join(gz(d, 6) for d in pay.values()), allp))
    members = [fq[i:i + 7000] for i in range(0, len(fq), 7000)]
    out.append(("multi_member", b"".join(gz(m, 1 + i % 9) for i, m in enumerate(members)), fq))
    out.append(("empty_members", gz(b"") + gz(fq[:5000]) + gz(b"") + gz(fq[5000:20000]) + gz(b""), fq[:20000]))
    out.append(("sync_flush", gz_flushed(fq, zlib.Z_SYNC_FLUSH), fq))
    out.append(("full_flush", gz_flushed(fq, zlib.Z_FULL_FLUSH), fq))
    out.append(("headers", gz_header(fq[:30000], fname=b"reads.fq") + gz_header(fq[30000:60000], comment=b"a comment", fhcrc=True) +
                gz_header(fq[60000:], extra=b"XY\x03\x00abc", fname=b"x", comment=b"y", fhcrc=True), fq))
    out.append(("bgzf", W.bgzf_compress(fq), fq))
    out.append(("empty", gz(b""), b""))
    return out
