"""Inputs of the CRAM device ingest tests (tests/test_cram_twin.py on the CPU, tests/test_gpu_cram.py on the device), all from
tests/cram_writer.py: single rANS 4x8 / rANS Nx16 streams at the lengths and alphabets where an interleaved decoder goes wrong, and
small unaligned CRAM files in every layout the walker must reproduce or refuse."""
import functools
import random

import cram_writer as CW

LENGTHS = (0, 1, 2, 3, 4, 5, 31, 32, 33, 127, 128, 129, 4095, 4096, 4097, 70_001)
ALPHABETS = {1: b"A", 2: b"AC", 4: b"ACGT", 5: b"ACGTN", 16: bytes(range(97, 113)), 17: bytes(range(65, 82)), 256: bytes(range(256))}
# the forms the device takes: (name, method byte, encoder)
FORMS = [("rans0", 4, lambda d: CW.rans4x8(d, 0)), ("rans1", 4, lambda d: CW.rans4x8(d, 1))]
for _k, _v in CW.NX16_FORMS.items():
    if "stripe" not in _k:
        FORMS.append((_k, 5, functools.partial(lambda d, kw: CW.nx16(d, **kw), kw=_v)))
FORMS.append(("nx16_nosz", 5, lambda d: CW.nx16(d, order=0, nosz=True)))
FORMS.append(("nx16_o1x32_nosz_pack", 5, lambda d: CW.nx16(d, order=1, x32=True, nosz=True, pack=True)))
FORMS.append(("nx16_packrle_o1", 5, lambda d: CW.nx16(d, order=1, pack=True, rle=True)))


def text(n, alphabet, seed):
    """n bytes over `alphabet`: runs of geometric length (so RLE has runs) of symbols drawn with a skew"""
    rng = random.Random(seed)
    out = bytearray()
    k = len(alphabet)
    while len(out) < n:
        s = alphabet[min(k - 1, int(rng.expovariate(3.0 / k)))] if k > 1 else alphabet[0]
        out += bytes([s]) * (1 + int(rng.expovariate(0.7)))
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def stream_cases():
    """[(name, method, compressed bytes, plain bytes)]: every form at every length over ACGT, the short lengths over every alphabet,
    the lengths around 4096 over 17 and 256 symbols (256: an order-1 model that does not fit LDS), and the special shapes"""
    out = []
    for fname, method, enc in FORMS:
        for n in LENGTHS:
            for a, alpha in ALPHABETS.items():
                if (n > 129 and a not in (4, 17, 256)) or (n > 4097 and a != 4) or (a == 256 and n not in (0, 5, 129, 4097)):
                    continue
                plain = text(n, alpha, 1000 * a + n)
                out.append(("%s_n%d_a%d" % (fname, n, a), method, enc(plain), plain))
    rare = b"A" * 3000 + b"C" + b"A" * 2000                     # a symbol of frequency 1: rANS 4x8 renormalises by two bytes
    out.append(("rans0_freq1", 4, CW.rans4x8(rare, 0), rare))
    out.append(("rans1_freq1", 4, CW.rans4x8(rare, 1), rare))
    every = b"".join(bytes([i, i]) for i in range(256)) * 3     # 256 run symbols: the count byte is 0
    out.append(("nx16_rle_256_run_symbols", 5, CW.nx16(every, order=0, rle=True), every))
    out.append(("nx16_rle_no_repeats", 5, CW.nx16(b"ACGT" * 50, order=1, rle=True), b"ACGT" * 50))
    long_runs = b"A" * 5000 + b"C" * 3 + b"G" * 70_000 + b"T"
    out.append(("nx16_rle_long_runs", 5, CW.nx16(long_runs, order=0, rle=True), long_runs))
    out.append(("nx16_packrle_long_runs", 5, CW.nx16(long_runs, order=0, pack=True, rle=True), long_runs))
    for n in (1, 2, 4, 16, 17):
        plain = text(777, bytes(range(48, 48 + n)), n)
        plain = plain + bytes(range(48, 48 + n))               # (every symbol is there)
        out.append(("nx16_pack_%d_symbols" % n, 5, CW.nx16(plain, order=0, pack=True), plain))
    raw = text(1234, b"ACGT", 5)
    out.append(("raw_1234", 0, raw, raw))
    out.append(("raw_0", 0, b"", b""))
    return out


def short_table_stream():
    """a rANS 4x8 order-0 stream whose table sums to 4095: legal for the host reader, refused by the device path"""
    plain = text(500, b"ACGT", 9)
    keep = CW._normalise

    def short(counts):
        F = keep(counts)
        F[max(range(256), key=lambda s: F[s])] -= 1
        return F
    CW._normalise = short
    try:
        return CW.rans4x8(plain, 0), plain
    finally:
        CW._normalise = keep


def refused_streams():
    """[(name, method, bytes, raw size, text the reason holds)]"""
    plain = text(900, b"ACGT", 3)
    short, sp = short_table_stream()
    return [("stripe", 5, CW.nx16(plain, order=0, stripe=4), len(plain), "STRIPE"),
            ("stripe_o1", 5, CW.nx16(plain, order=1, stripe=3), len(plain), "STRIPE"),
            ("gzip", 1, CW.compress(plain, "gzip"), len(plain), "gzip"),
            ("bzip2", 2, CW.compress(plain, "bzip2"), len(plain), "bzip2"),
            ("lzma", 3, CW.compress(plain, "lzma"), len(plain), "lzma"),
            ("arith", 6, plain, len(plain), "arith"),
            ("fqzcomp", 7, plain, len(plain), "fqzcomp"),
            ("tok3", 8, plain, len(plain), "tok3"),
            ("short_table", 4, short, len(sp), "short table"),
            ("size_differs", 4, CW.rans4x8(plain, 0), len(plain) + 1, "size mismatch")]


def reads(n, seed, lo=0, hi=400, zero_at=None):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        ln = 0 if i == zero_at else rng.randint(lo, hi)
        name = b"*" if i % 11 == 7 else b"read%d/%d" % (seed, i)
        out.append((name, text(ln, b"ACGTN", seed * 100 + i)))
    return out


@functools.lru_cache(maxsize=None)
def file_cases():
    """[(name, file bytes)]: the walker's corpus.  7 records a slice unless said otherwise"""
    out = []
    R = reads(23, 1, zero_at=5)
    for variant in ("external", "core"):
        for name_form in ("stop", "len"):
            for q, t in ((True, True), (False, False)):
                for spc in (1, 3):
                    tag = "%s_%s_q%d_t%d_spc%d" % (variant, name_form, q, t, spc)
                    out.append((tag, CW.write_cram(R, variant=variant, method="rans0", slices_per_container=spc, records_per_slice=7, with_quality=q, with_tags=t,
                                                   name_form=name_form, method_for={"BA": "rans1"})))
    for m in ("raw", "rans0", "rans1"):
        out.append(("ba_" + m, CW.write_cram(R, method="gzip", records_per_slice=7, method_for={"BA": m})))
    for m in CW.NX16_FORMS:
        if "stripe" not in m:
            out.append(("v31_" + m, CW.write_cram(R, method="gzip", records_per_slice=7, slices_per_container=2, minor=1, method_for={"BA": m, "RN": "tok3"})))
    out.append(("empty", CW.write_cram([], method="raw")))
    out.append(("all_raw", CW.write_cram(R, method="raw", records_per_slice=7)))
    out.append(("one_record_of_length_0", CW.write_cram([(b"z", b"")], method="rans0")))
    big = reads(300, 2, 300, 1000)
    out.append(("larger_200k", CW.write_cram(big, method="gzip", records_per_slice=60, slices_per_container=2, minor=1, method_for={"BA": "nx16_o1"})))
    return out


def by_name(name):
    return next(f for n, f in file_cases() if n == name)


def _patch(data, old, new, count=1):
    assert data.count(old) == count, (old, data.count(old))
    return data.replace(old, new)


def refused_files():
    """[(name, file bytes, text the reason holds)]"""
    R = reads(14, 3, 1, 200)
    out = []
    out.append(("stripe_ba", CW.write_cram(R, method="gzip", minor=1, records_per_slice=7, method_for={"BA": "nx16_stripe"}), "STRIPE"))
    out.append(("gzip_ba", CW.write_cram(R, method="gzip", records_per_slice=7), "a BA block in gzip"))
    out.append(("mapped", CW.write_cram(R, method="rans0", records_per_slice=7, mapped_at=9), "Mapped records are not supported"))
    # everything raw, so that the compression header and the RL block can be edited in place
    plain = CW.write_cram(R, method="raw", records_per_slice=7)
    noq = CW.write_cram(R, method="raw", records_per_slice=7, with_quality=False)      # (no record has qualities: the host reader never follows QS)
    out.append(("shared_ba_id", _patch(noq, b"QS\x01\x01\x0e", b"QS\x01\x01\x0d", 2), "shared with another series"))
    lens = b"".join(CW.itf8(len(s)) for _, s in R[:7])
    shorter = bytearray(lens)
    k = next(i for i, v in enumerate(shorter) if 2 <= v < 0x80)
    shorter[k] -= 1                                                     # one read a base shorter than the BA block says
    out.append(("lengths_do_not_add_up", _patch(plain, lens, bytes(shorter)), "do not add up"))
    short, sp = short_table_stream()
    one = CW.write_cram([(b"r", sp)], method="raw", method_for={"BA": "rans0"})
    out.append(("short_table", _patch(one, CW.rans4x8(sp, 0), short), "short table"))
    out.append(("rn_not_preserved", _patch(plain, b"RN\x01AP", b"RN\x00AP", 2), "names are not preserved"))
    out.append(("behind_gzip", __import__("gzip").compress(plain), None))
    return out


def ba_body_span(data, plain_bases, method):
    """where the compressed BA body of a one-slice file starts and ends"""
    body = CW.compress(plain_bases, method)
    at = data.index(body)
    return at, at + len(body)
