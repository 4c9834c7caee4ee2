"""Unaligned SAM text for the record-scan tests (tests/test_sam_twin.py on the CPU, tests/test_gpu_sam.py on the device), written
from the SAM specification (sections 1.3 and 1.4) alone: a well-formed corpus that the device scan must prove, and the explicit
list of inputs it must leave to the host parser, each with what the host parser does with it."""
import random

HD = b"@HD\tVN:1.6\tSO:unknown\n"
MAPPED = "Mapped records are not supported. Only unaligned BAM/CRAM/SAM is allowed."
FEW = "invalid SAM record: fewer than 11 fields"
BAD_FLAG = "invalid SAM record: bad flag field"
# the tenth tab on every side of a 16-byte group and of a 1 KiB step
LENGTHS = [1, 15, 16, 17] + list(range(1007, 1041)) + [5000]
SHIFT_LENGTHS = [1, 15, 16, 17, 1007, 1015, 1016, 1017, 1023, 1024, 1039, 1040]


def _seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def rec(name, seq, flag=b"4", qual=None, tags=(), eol=b"\n"):
    """One alignment line: the eleven mandatory fields of an unaligned read, then the tags.  qual: the field's bytes verbatim
    (default: '*' for an empty sequence, else one 'I' per base)."""
    q = (b"I" * len(seq) or b"*") if qual is None else qual
    return b"\t".join([name, flag, b"*", b"0", b"0", b"*", b"*", b"0", b"0", seq, q] + list(tags)) + eol


def sam(lines, hdr=HD):
    return hdr + b"".join(lines)


def _length_lines(rng, lengths, eol=b"\n"):
    out = [rec(b"star", b"*", eol=eol), rec(b"none", b"", qual=b"*", eol=eol)]
    return out + [rec(b"l%d" % k, _seq(rng, k, b"ACGTN"), eol=eol) for k in lengths]


def toy_sam(names, seqs, flag=b"4"):
    """reads as `samtools view -h` would print an unaligned BAM of them"""
    return sam([rec(n, s, flag=flag, tags=[b"RG:Z:toy"]) for n, s in zip(names, seqs)], HD + b"@RG\tID:toy\tPL:ONT\n")


def well_formed():
    """(name, bytes): every one must be proven by the device scan, and parsed by the host parser"""
    rng = random.Random(41)
    reads = [(b"read%d" % i, _seq(rng, rng.randint(100, 300))) for i in range(40)]
    out = [("header_only", HD), ("header_no_lf", b"@HD"), ("header_three_lines", HD + b"@SQ\tSN:chr1\tLN:1000\n@CO\tnothing else\n")]
    one = rec(b"only", b"ACGTTGCA")
    out += [("magic_hd", sam([one])), ("magic_sq", sam([one], b"@SQ\tSN:chr1\tLN:1000\n")), ("magic_rg", sam([one], b"@RG\tID:g\n")),
            ("magic_alone", sam([one], b"@RG\n"))]
    out.append(("plain_40", sam([rec(n, s) for n, s in reads])))
    out.append(("lengths", sam(_length_lines(rng, LENGTHS))))
    for k in range(16):             # the same lines behind a header of every length modulo 16
        out.append(("shift_%d" % k, sam(_length_lines(random.Random(42), SHIFT_LENGTHS), HD + b"@CO\t" + b"x" * k + b"\n")))
    names = [rec(b"*", b"ACGTAC"), rec(b"", b"GGA"), rec(b"n" * 254, b"GATTACA"), rec(b"with blanks  inside ", b"ACCA"), rec(b" lead", b"TT"),
             rec(b"nul\0inside", b"CCGG"), rec(b"@skipped_by_both", b"ACGTACGT"), rec(b"**", b"AC"), rec(b"*x", b"CA"), rec(b"*", b"*")]
    out.append(("names", sam(names)))
    out.append(("star_star_sequence", sam([rec(b"ss", b"**"), rec(b"s1", b"*"), rec(b"s2", b"*A")])))
    out.append(("flags_with_4", sam([rec(b"f" + f, _seq(rng, 20), flag=f) for f in (b"4", b"004", b"77", b"141", b"2052", b"000000004", b"999999999")])))
    out.append(("empty_quality", sam([rec(b"q0", b"ACGTACGTAC", qual=b""), rec(b"q1", b"", qual=b""), rec(b"q2", _seq(rng, 130), qual=b"")])))
    tags = [b"RG:Z:group one", b"MM:Z:C+m,5,12,0;C+h,5,12,0;", b"ML:B:C,200,201,202,203,204,205", b"qs:f:12.5", b"ns:i:-7", b"pi:Z:parent-read",
            b"mv:B:c," + b",".join(b"1" for _ in range(600))] + [b"x%d:i:%d" % (i % 10, i) for i in range(40)]
    out.append(("many_tags", sam([rec(b"t%d" % i, _seq(rng, 120 + i), tags=tags[i % 3:]) for i in range(12)])))
    lines = []
    for i, (n, s) in enumerate(reads[:12]):
        lines += [rec(n, s)] + [b"@CO\tbetween records %d\n" % i, b"\n", b"\n\n@CO\n", b"@\n"][i % 5:i % 5 + 1]
    out.append(("co_and_empty_lines", sam(lines, HD + b"\n")))
    crlf = HD.replace(b"\n", b"\r\n") + b"@CO\tdos\r\n" + b"".join(rec(n, s, eol=b"\r\n") for n, s in reads[:20]) + b"\r\n"
    out.append(("crlf", crlf))
    out.append(("crlf_lengths", HD.replace(b"\n", b"\r\n") + b"".join(_length_lines(rng, SHIFT_LENGTHS, eol=b"\r\n"))))
    out.append(("no_final_lf", sam([rec(n, s) for n, s in reads[:5]])[:-1]))
    out.append(("no_final_lf_empty_quality", sam([rec(b"a", b"ACGT"), rec(b"b", b"GGCC", qual=b"", eol=b"")])))
    out.append(("final_cr_line", sam([rec(n, s) for n, s in reads[:5]]) + b"\r"))
    out.append(("final_cr_after_crlf", crlf + b"\r"))
    out.append(("short_3000", sam([rec(b"s%d" % i, b"ACGTACGT"[i % 5:i % 5 + 1 + i % 3], flag=b"4") for i in range(3000)])))
    long_seq = _seq(rng, 200000, b"ACGTN")
    out.append(("long_200k", sam([rec(n, s) for n, s in reads[:3]] + [rec(b"long", long_seq)] + [rec(n, s) for n, s in reads[3:6]])))
    return out


def mutation_bases():
    """the three well-formed cases the single-byte mutations start from: every read has 100 bases or more"""
    cases = dict(well_formed())
    return [(k, cases[k]) for k in ("plain_40", "crlf", "many_tags")]


def unproven():
    """(name, bytes, host): the device scan must return the unproven verdict for each.  host: what the host parser does with the
    same bytes -- its message, or the number of records it returns where strtoul takes a flag the device does not restate"""
    rng = random.Random(43)
    reads = [(b"u%d" % i, _seq(rng, 10 + 3 * i)) for i in range(9)]
    lines = [rec(n, s) for n, s in reads]

    def with_line(line):
        return sam(lines[:4] + [line] + lines[4:])

    nine = b"\t".join([b"nine", b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0", b"ACGT"]) + b"\n"
    out = [("tabs_9", with_line(nine), FEW), ("tabs_9_last_no_lf", sam(lines + [nine[:-1]]), FEW), ("tabs_0", with_line(b"just a line\n"), FEW),
           ("flag_empty", with_line(rec(b"fe", b"ACGT", flag=b"")), BAD_FLAG),
           ("flag_4x", with_line(rec(b"fx", b"ACGT", flag=b"4x")), BAD_FLAG),
           ("flag_blank_4", with_line(rec(b"fb", b"ACGT", flag=b" 4")), 10),
           ("flag_plus_4", with_line(rec(b"fp", b"ACGT", flag=b"+4")), 10),
           ("flag_minus_4", with_line(rec(b"fm", b"ACGT", flag=b"-4")), 10),
           ("flag_4_nul", with_line(rec(b"fn", b"ACGT", flag=b"4\0")), 10),
           ("flag_10_digits", with_line(rec(b"ft", b"ACGT", flag=b"0000000004")), 10),
           ("flag_0", with_line(rec(b"m0", b"ACGT", flag=b"0")), MAPPED),
           ("flag_16", with_line(rec(b"m16", b"ACGT", flag=b"16")), MAPPED),
           ("flag_3", with_line(rec(b"m3", b"ACGT", flag=b"3")), MAPPED),
           ("mapped_first", sam([rec(b"m", b"ACGT", flag=b"0")] + lines), MAPPED)]
    hundred = [rec(b"h%d" % i, _seq(rng, 30 + i)) for i in range(99)]
    out.append(("mapped_last_of_100", sam(hundred + [rec(b"mapped", _seq(rng, 25), flag=b"0")]), MAPPED))
    out.append(("line_cr_cr", with_line(b"\r\r\n"), FEW))
    # without the sniffed magic the text never reaches the SAM parser on the host: it is FASTQ by its '@', or nothing it knows
    out.append(("starts_with_co", sam(lines[:2], b"@CO\tno magic\n"), "truncated FASTQ record"))
    out.append(("starts_with_record", b"".join(lines), "unrecognised sequence file"))
    return out
