"""Uncompressed BAM for the record-scan tests (tests/test_bam_twin.py on the CPU, tests/test_gpu_bam.py on the device), written
from the SAM/BAM specification (section 4.2) alone: a well-formed corpus of unaligned records that the device scan must prove,
with baits for its speculative starts, and the explicit list of inputs it must leave to the host parser."""
import random
import struct

NT16 = b"=ACMGRSVTWYHKDBN"
CODE = {c: i for i, c in enumerate(NT16)}


def pack_seq(seq):
    nib = [CODE[c] for c in seq] + [0]
    return bytes((nib[i] << 4) | nib[i + 1] for i in range(0, len(seq), 2))


def header(text=b"@HD\tVN:1.6\tSO:unknown\n", refs=()):
    out = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, length in refs:
        out.append(struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length))
    return b"".join(out)


def record(name, seq, flag=4, tags=b"", cigar=(), qual=None, read_name=None, l_seq=None, block=None, pos=-1):
    """One alignment record with its block_size in front.  read_name: the field's bytes verbatim (default: name + NUL);
    l_seq / block: written instead of the true values."""
    rn = name + b"\0" if read_name is None else read_name
    q = bytes([0xFF]) * len(seq) if qual is None else qual
    assert len(q) == len(seq) and len(rn) < 256
    body = struct.pack("<iiBBHHHiiii", -1, pos, len(rn), 0, 4680, len(cigar), flag, len(seq) if l_seq is None else l_seq, -1, -1, 0) + rn + \
        b"".join(struct.pack("<I", c) for c in cigar) + pack_seq(seq) + q + tags
    return struct.pack("<i", len(body) if block is None else block) + body


def tag_z(tag, s):
    return tag + b"Z" + s + b"\0"


def tag_b(tag, sub, payload, count=None):
    width = {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}[sub]
    return tag + b"B" + sub + struct.pack("<I", len(payload) // width if count is None else count) + payload


def _seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def bam(records, hdr=None):
    return (header() if hdr is None else hdr) + b"".join(records)


def big_reads():
    """the 60 mixed-length reads of fastx_corpus's *_big cases, with their descriptions as part of the name"""
    import fastx_corpus as F
    lines = dict(F.well_formed())["fq_big"].split(b"\n")
    return [(lines[i][1:], lines[i + 1]) for i in range(0, len(lines) - 1, 4)]


def _bait_chain(rng, k, tail=b"\0" * 8):
    """k chained flag-4 records, as a speculative start would read them, then bytes that are no record (block_size 0)"""
    return b"".join(record(b"bait%d" % i, _seq(rng, rng.randint(1, 9))) for i in range(k)) + tail


def well_formed():
    """(name, bytes): every one must be proven by the device scan, and parsed by the host parser"""
    rng = random.Random(31)
    recs = [(b"read%d" % i, _seq(rng, rng.randint(1, 300))) for i in range(40)]
    out = [("empty", header()), ("empty_no_text", header(b"")), ("one_record", bam([record(b"only", b"ACGTTGCA")]))]
    out.append(("plain_40", bam([record(n, s) for n, s in recs])))
    out.append(("lengths", bam([record(b"l%d" % k, _seq(rng, k, b"ACGTN")) for k in (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 0, 1, 0)])))
    out.append(("all_codes", bam([record(b"codes", NT16), record(b"codes_rev", NT16[::-1] + b"="), record(b"codes_odd", (NT16 * 5)[3:])])))
    names = [record(b"*", b"ACGTAC"), record(b"", b"GGA", read_name=b""), record(b"", b"TTC", read_name=b"\0"), record(b"with space and\ttab", b"ACCA"),
             record(b"n" * 100 + b" \t" + b"m" * 152, b"GATTACA"), record(b"nul\0inside", b"CCGG"), record(b"**", b"AC"), record(b"*", b"")]
    out.append(("names", bam(names)))
    mm = tag_z(b"MM", b"C+m,5,12,0;C+h,5,12,0;") + tag_b(b"ML", b"C", bytes(range(200, 206)))
    tags = [record(b"t0", _seq(rng, 50), tags=tag_z(b"RG", b"group one") + tag_b(b"ZB", b"s", struct.pack("<4h", -1, 2, -3, 4))),
            record(b"t1", _seq(rng, 33), tags=mm + b"qsf" + struct.pack("<f", 12.5) + b"nsi" + struct.pack("<i", -7)),
            record(b"t2", _seq(rng, 1), tags=tag_b(b"ZF", b"f", struct.pack("<3f", 1.0, -2.0, 0.5)) + tag_z(b"pi", b"parent-read"))]
    out.append(("tags", bam(tags)))
    out.append(("cigar_unmapped", bam([record(b"c0", b"ACGTACGT", cigar=(8 << 4,)), record(b"c1", b"ACG", cigar=(1 << 4 | 4, 2 << 4)), record(b"c2", b"TT")])))
    out.append(("flags_with_4", bam([record(b"f%d" % f, _seq(rng, 20), flag=f) for f in (4, 5, 77, 141, 516, 0xFFFF)])))
    out.append(("unmapped_with_pos", bam([record(b"p%d" % i, _seq(rng, 30 + i), pos=1000 * i) for i in range(12)])))        # no candidate anywhere: repair only
    co = b"@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chrM\tLN:16569\n" + b"".join(b"@CO\t" + b"x" * 95 + b"\n" for _ in range(1000))
    out.append(("header_refs_100k", bam([record(n, s) for n, s in recs[:9]], header(co, [(b"chr1", 1000), (b"chrM", 16569)]))))
    long_seq = _seq(rng, 20001, b"ACGTN")
    out.append(("long_record", bam([record(n, s) for n, s in recs[:3]] + [record(b"long", long_seq)] + [record(n, s) for n, s in recs[3:8]])))
    out.append(("short_3000", bam([record(bytes([33 + i % 90]), b"ACGT"[i % 4:i % 4 + 1]) for i in range(3000)])))
    out.append(("big_60", bam([record(n, s) for n, s in big_reads()])))
    for name, data in baits():
        out.append((name, data))
    return out


def baits():
    """well-formed files with bytes inside records that pass for record starts"""
    rng = random.Random(32)
    out = []
    # a B:C tag whose payload is a chain of three valid records, then bytes that break the chain; one such tag in every record
    rs = []
    for i in range(60):
        rs.append(record(b"tagbait%d" % i, _seq(rng, rng.randint(1, 120)), tags=tag_z(b"RG", b"g") + tag_b(b"ZC", b"C", _bait_chain(rng, 3) + bytes(rng.randint(0, 40)))))
    out.append(("bait_tag_chain", bam(rs)))
    # a quality string that spells record headers
    rs = []
    for i in range(40):
        q = _bait_chain(rng, 2, b"")
        q += bytes([0xFF]) * rng.randint(5, 60)
        rs.append(record(b"qualbait%d" % i, _seq(rng, len(q)), qual=q))
    out.append(("bait_quality", bam(rs)))
    # a bait whose chain lands on a true record start: its second record's block reaches to the end of the carrying record
    rs = []
    for i in range(40):
        first = record(b"land%d" % i, _seq(rng, rng.randint(1, 9)))
        rest = bytes(rng.randint(0, 50))
        second = record(b"x", b"AC")
        second = struct.pack("<i", len(second) - 4 + len(rest)) + second[4:] + rest
        rs.append(record(b"landing%d" % i, _seq(rng, rng.randint(1, 120)), tags=tag_b(b"ZC", b"C", first + second)))
    out.append(("bait_lands_on_true_start", bam(rs)))
    return out


def unproven():
    """(name, bytes): the device scan must return the unproven verdict for each; what the host does with it is its business"""
    rng = random.Random(33)
    recs = [record(b"u%d" % i, _seq(rng, 10 + 3 * i)) for i in range(9)]
    mapped = record(b"mapped", _seq(rng, 25), flag=0)
    whole = bam(recs)
    out = [("mapped_first", bam([mapped] + recs)), ("mapped_middle", bam(recs[:4] + [mapped] + recs[4:])), ("mapped_last", bam(recs + [mapped])),
           ("block_below_32", bam(recs[:3]) + struct.pack("<i", 31) + bytes(31) + b"".join(recs[3:])),
           ("negative_l_seq", bam(recs[:5] + [record(b"neg", b"ACGT", l_seq=-4)] + recs[5:])),
           ("seq_does_not_fit", bam(recs[:5] + [record(b"fit", b"ACGT", l_seq=4000)] + recs[5:])),
           ("last_record_cut", whole[:-7])]
    out += [("trailing_%d" % k, whole + bytes(k)) for k in (1, 2, 3)]
    out.append(("negative_l_text", b"BAM\x01" + struct.pack("<i", -1) + whole[8:]))
    h = header(refs=[(b"chr1", 1000), (b"chr2", 2000)])
    out.append(("header_cut_in_references", h[:-6]))
    return out
