"""BGZF writer for the tests (SAM/BAM specification section 4.1): raw deflate from Python's zlib (wbits=-15), CRC-32 from
zlib.crc32, and a real `BC` subfield in every member.  Every block can be compressed with its own level / strategy /
memLevel, and may carry other extra subfields, a file name, a comment or a header CRC."""
import struct
import zlib

MAX_BLOCK = 65536
DEFAULT_BLOCK = 65280          # what bgzip puts in a block: fits even when it does not compress


def deflate_raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, memlevel=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, memlevel, strategy)
    return c.compress(data) + c.flush()


def bgzf_block(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, memlevel=8, extra_before=b"", extra_after=b"",
               fname=None, comment=None, fhcrc=False, comp=None):
    """One BGZF member holding `data` (<= 65536 bytes).  extra_before / extra_after: whole subfields (SI1 SI2 SLEN data)
    around the BC subfield.  comp: a ready-made raw deflate stream for `data` (tests/deflate_writer.py) instead of zlib's."""
    assert len(data) <= MAX_BLOCK
    if comp is None:
        comp = deflate_raw(data, level, strategy, memlevel)
    flg = 4 | (8 if fname is not None else 0) | (16 if comment is not None else 0) | (2 if fhcrc else 0)
    tail = (fname + b"\0" if fname is not None else b"") + (comment + b"\0" if comment is not None else b"")
    xlen = len(extra_before) + 6 + len(extra_after)
    size = 12 + xlen + len(tail) + (2 if fhcrc else 0) + len(comp) + 8
    assert size <= 65536, "block does not fit in BSIZE"
    head = bytes([0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 0xff]) + struct.pack("<H", xlen) + extra_before + \
        b"BC" + struct.pack("<HH", 2, size - 1) + extra_after + tail
    if fhcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + comp + struct.pack("<II", zlib.crc32(data), len(data))


EOF_BLOCK = bgzf_block(b"")


def bgzf_compress(data, block=DEFAULT_BLOCK, eof=True, **kw):
    """`data` cut into blocks of `block` bytes, each a BGZF member, then the empty end-of-file block."""
    out = [bgzf_block(data[i:i + block], **kw) for i in range(0, len(data), block)]
    if eof:
        out.append(EOF_BLOCK)
    return b"".join(out)


def bam_bytes(names, seqs):
    """Uncompressed unaligned BAM (flag 4, no references): the layout of tests/conftest.py's uBAM writer."""
    code = {c: i for i, c in enumerate(b"=ACMGRSVTWYHKDBN")}
    text = b"@HD\tVN:1.6\tSO:unknown\n"
    body = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", 0)]
    for n, s in zip(names, seqs):
        nib = [code.get(c, 15) for c in s.upper()]
        if len(nib) & 1:
            nib.append(0)
        packed = bytes((nib[i] << 4) | nib[i + 1] for i in range(0, len(nib), 2))
        name = n + b"\0"
        rec = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 0, 4680, 0, 4, len(s), -1, -1, 0) + name + packed + b"\xff" * len(s)
        body.append(struct.pack("<i", len(rec)) + rec)
    return b"".join(body)


def fastq_bytes(names, seqs):
    return b"".join(b"@%s extra words\n%s\n+\n%s\n" % (n, s, bytes(33 + (i * 7 + 3 * j) % 40 for j in range(len(s))))
                    for i, (n, s) in enumerate(zip(names, seqs)))


def fasta_bytes(names, seqs, width=60):
    return b"".join(b">%s\n" % n + b"".join(s[i:i + width] + b"\n" for i in range(0, len(s), width)) for n, s in zip(names, seqs))
