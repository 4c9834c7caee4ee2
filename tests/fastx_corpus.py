"""FASTA / FASTQ texts for the record-scan tests (tests/test_fastx_twin.py on the CPU, tests/test_gpu_ingest.py on the device):
a well-formed corpus that the device parser must prove, and the explicit list of inputs it must leave to the host parser."""
import random

WS = [b" ", b"\t", b"\n", b"\r", b"\v", b"\f"]


def _seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def fastq_text(recs, eol=b"\n", final=True, lead=0, trail=0, quals=None):
    out = [eol * lead]
    for i, (h, s) in enumerate(recs):
        q = quals[i] if quals else bytes(33 + (i + 5 * j) % 40 for j in range(len(s))).replace(b"@", b"I").replace(b"+", b"J")
        out.append(b"@" + h + eol + s + eol + b"+" + eol + q + eol)
    t = b"".join(out)
    if not final and t.endswith(eol):
        t = t[:-len(eol)]
    return t + (eol * trail if final else b"")


def fasta_text(recs, width=60, eol=b"\n", final=True, lead=0, trail=0):
    out = [eol * lead]
    for h, s in recs:
        out.append(b">" + h + eol)
        if width is None:
            out.append(s + eol)
        else:
            out += [s[i:i + width] + eol for i in range(0, len(s), width)]
    t = b"".join(out)
    if not final and t.endswith(eol):
        t = t[:-len(eol)]
    return t + (eol * trail if final else b"")


def _sized_fastq(size):
    """a FASTQ text of exactly `size` bytes"""
    rng = random.Random(size)
    recs = []
    while len(fastq_text(recs)) + 200 < size:
        recs.append((b"r%d d" % len(recs), _seq(rng, rng.randint(1, 90))))
    t = fastq_text(recs)
    pad = size - len(t)               # one more record of exactly `pad` bytes: "@" h "\n" s "\n+\n" q "\n" = 6 + |h| + 2 |s|
    k = (pad - 6) // 2
    t += fastq_text([(b"x" * (pad - 6 - 2 * k), _seq(rng, k))])
    assert len(t) == size
    return t


def well_formed():
    """(name, text): every one must be proven by the device parser, and parsed by the host parser"""
    rng = random.Random(20)
    recs = [(b"read%d some description" % i, _seq(rng, rng.randint(1, 300))) for i in range(40)]
    out = []
    for eol, en in ((b"\n", "lf"), (b"\r\n", "crlf")):
        for final in (True, False):
            tag = "%s_%s" % (en, "nl" if final else "nonl")
            out.append(("fq_" + tag, fastq_text(recs, eol, final)))
            out.append(("fa_" + tag, fasta_text(recs, 60, eol, final)))
        out.append(("fq_lead_trail_" + en, fastq_text(recs, eol, True, lead=3, trail=5)))
        out.append(("fa_lead_trail_" + en, fasta_text(recs, 60, eol, True, lead=2, trail=4)))
        for w in (1, 60, 61, None):
            out.append(("fa_w%s_%s" % (w, en), fasta_text(recs[:12], w, eol)))
    # identifiers: empty, and cut at each of the six whitespace bytes (LF and CR end the header line itself)
    ids = [(b"", b"ACGT"), (b" only a description", b"GGCC")] + [(b"id%d" % i + ws + b"rest", _seq(rng, 30)) for i, ws in enumerate(WS) if ws not in (b"\n", b"\r")]
    out.append(("fq_ids", fastq_text(ids)))
    out.append(("fa_ids", fasta_text(ids)))
    out.append(("fq_id_cr_inside", b"@a\rb c\nACGT\n+\nIIII\n"))
    out.append(("fa_id_cr_inside", b">a\rb c\r\nAC\rGT\r\n"))
    # zero-length sequences
    empt = [(b"e0", b""), (b"n1", b"ACGT"), (b"e2", b""), (b"e3", b"")]
    out.append(("fq_empty_seqs", fastq_text(empt)))
    out.append(("fa_empty_seqs", fasta_text(empt)))
    out.append(("fa_header_only", b">h"))
    out.append(("fa_header_only_cr", b">h x\r"))
    out.append(("fa_blank_lines_inside", b">a\nAC\n\nGT\n\r\n>b\n\n\nTT"))
    # sequence lines that start with '@' (FASTA), quality lines that start with '@' and '+' (FASTQ)
    out.append(("fa_at_lines", b">a\n@CGT\n@@\n>b\n@\n"))
    q = [(b"q0", b"ACGTA"), (b"q1", b"CCCCC"), (b"q2", b"GG")]
    out.append(("fq_qual_at_plus", fastq_text(q, quals=[b"@IIII", b"+@+@+", b"@+"])))
    out.append(("fq_plus_repeats_id", b"@a x\nACGT\n+a x\nIIII\n@b\nGG\n+b\n@@\n"))
    # lower case and IUPAC
    out.append(("fq_iupac", fastq_text([(b"i0", b"acgtnRYKMswbdhvNU-*"), (b"i1", b"ACGTacgtuU")])))
    out.append(("fa_iupac", fasta_text([(b"i0", b"acgtnRYKMswbdhvNU-*" * 9), (b"i1", b"ACGTacgtuU")], 7)))
    # a single record
    out.append(("fq_single", fastq_text(recs[:1])))
    out.append(("fa_single", fasta_text(recs[:1])))
    out.append(("fa_gt_inside", b">a >b\nAC>GT\nA>\n>c\nTT\n"))
    # sizes around the tile
    out.append(("size_0", b""))
    out.append(("size_1_lf", b"\n"))
    out.append(("blank_only", b"\n\r\n\n\r"))
    for size in (4095, 4096, 4097):
        out.append(("fq_size_%d" % size, _sized_fastq(size)))
        fa = fasta_text([(b"s", b"A" * 5000)], 60)[:size]
        out.append(("fa_size_%d" % size, fa))
    # many tiles
    big = [(b"big%d len=%d" % (i, i), _seq(rng, rng.randint(100, 3000), b"ACGTN")) for i in range(60)]
    out.append(("fq_big", fastq_text(big)))
    out.append(("fa_big_w60_crlf", fasta_text(big, 60, b"\r\n")))
    out.append(("fa_big_one_line", fasta_text(big, None)))
    return out


def unproven():
    """(name, text): the device parser must return the unproven verdict for each; what the host does with it is its business"""
    r = [(b"a", b"ACGT"), (b"b", b"GGTT"), (b"c", b"TTAA")]
    fq = fastq_text(r)
    return [
        ("fq_empty_line_between_records", fastq_text(r[:1]) + b"\n" + fastq_text(r[1:])),
        ("fq_three_line_tail", fq + b"@d\nACGT\n+\n"[:-1]),
        ("fq_plus_missing", b"@a\nACGT\nIIII\n@b\nGG\n+\nII\n"),
        ("fq_fifth_line_not_at", fastq_text(r[:1]) + b"b\nGGTT\n+\nIIII\n"),
        ("first_byte_other", b"ACGT\n>a\nACGT\n"),
        ("sam_header", b"@HD\tVN:1.6\tSO:unknown\nr0\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n"),
        ("bam_magic", b"BAM\x01" + b"\0" * 8),
        ("fq_empty_quality_line_missing", b"@a\nAC\n+\nII\n@b\n\n+\n"),
    ]
