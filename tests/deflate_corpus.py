"""Legal (and deliberately illegal) deflate streams that zlib's encoder never writes, made by tests/deflate_writer.py: code
shapes up to the 15-bit limit, odd dynamic headers, stored blocks at every bit alignment with any padding, thousands of tiny
blocks, one block for a whole member, matches at the edges of the window, members that reach into their predecessor.

The reference is zlib's inflate, for the bytes and for accept / reject alike: `expected` of a case is what zlib decodes at
import, or None when zlib refuses the stream; every case states which of the two it means and the module asserts that zlib
agrees.  `claimed` is what the writer's tokens say the output is; for an accepted case it equals `expected`, for a rejected one
it is what the trailer of a gzip / BGZF wrapper is made of, so that only the deflate error can be the reason to refuse it.

Slots.  The gzip decoder gives each chunk of compressed bytes a slot of ratio x chunk symbols and refuses (TOO_MANY) a file
whose chunk expands beyond it.  For every accepted gzip case outside DENSE the module asserts, with zlib alone, that no
chunk-sized piece of the file inflates to more than ratio x chunk bytes, at every (chunk, ratio) the tests run (SLOTS); a
piece is measured against the nominal chunk size because the slot is sized from it, also for the last, shorter piece."""
import collections
import gzip
import random
import zlib

import bgzf_writer as W
import deflate_writer as D
import gzip_corpus as G

Case = collections.namedtuple("Case", "name raw expected claimed")

# (chunk bytes, slot ratio): the CPU twin runs chunks 512 .. 512 KiB at ratio 64; the device runs its defaults (512 KiB, 8)
# and (512, 64)
SLOTS = [(512, 64), (4096, 64), (65536, 64), (512 << 10, 64), (512 << 10, 8)]
# accepted cases that may end in TOO_MANY: denser than a slot by construction
DENSE = ["overlap_dist1to8_len258_pure"]

STATS = {"max_lit_len": 0, "max_dist_len": 0, "stored_align": set(), "len258": set(), "blocks": 0}


def zlib_raw(raw):
    """zlib's verdict on a raw deflate stream that must end with its last byte: the bytes, or None"""
    try:
        o = zlib.decompressobj(-15)
        out = o.decompress(raw)
        return out if o.eof and not o.unused_data else None
    except zlib.error:
        return None


def zlib_gzip(data):
    try:
        return gzip.decompress(data)
    except Exception:
        return None


def note(d):
    STATS["max_lit_len"] = max(STATS["max_lit_len"], d.max_lit_len)
    STATS["max_dist_len"] = max(STATS["max_dist_len"], d.max_dist_len)
    STATS["stored_align"] |= d.stored_align
    STATS["blocks"] += d.n_blocks
    STATS["len258"] |= d.enc258


def text(n, seed=1, alphabet=b"ACGT"):
    rng = random.Random(seed)
    return bytes(rng.choice(alphabet) for _ in range(n))


def noise(n, seed=1):
    return random.Random(seed).randbytes(n)


# ------------------------------------------------------------------------------------------------------------------------
# the raw cases
# ------------------------------------------------------------------------------------------------------------------------
def _build():
    cases = []

    def add(name, d, accept, pad=0):
        raw = d.finish(pad) if isinstance(d, D.Deflate) else d[0]
        claimed = bytes(d.out) if isinstance(d, D.Deflate) else d[1]
        if isinstance(d, D.Deflate):
            note(d)
        exp = zlib_raw(raw)
        if accept:
            assert exp is not None, "zlib rejects %s" % name
            assert exp == claimed, "the writer's model and zlib differ on %s" % name
        else:
            assert exp is None, "zlib accepts %s" % name
        assert name not in [c.name for c in cases]
        cases.append(Case(name, raw, exp, claimed))

    lit_chain = lambda lo, hi, first: {first + i: lo + i for i in range(hi - lo + 1)}   # noqa: E731

    # ---- 1. literal/length codes of every length 1 .. 15 ----
    # one chain 1, 2, .. 14, 15, 15 (the Fibonacci shape) over literals, two length symbols and the end of block
    syms = [256, 257, 65, 258] + list(range(66, 78))
    lens = D.fibonacci_lengths(syms)
    assert sorted(lens.values()) == list(range(1, 15)) + [15, 15]
    d = D.Deflate()
    toks = [s for s in syms if s < 256] * 3 + [(3, 5), (4, 7)] + [77, 76, 65]
    d.dynamic(toks, lens, {0: 1, 4: 2, 5: 2}, final=True)
    add("lit_lengths_1_to_15_chain", d, True)
    # a literal, a length symbol and the end of block each at 11 .. 15 bits: the count walk past the 10-bit table, per length
    for eob_len in (11, 12, 13, 14, 15, 1):
        pinned = {256: eob_len}
        pinned.update(lit_chain(2, 8, 33) if eob_len == 1 else lit_chain(1, 8, 33))
        for k, L in enumerate(range(11, 16)):
            pinned[97 + k] = L           # literals a .. e at 11 .. 15 bits
            pinned[257 + k] = L          # lengths 3 .. 7 at 11 .. 15 bits
        lens = D.pinned_lengths(pinned, list(range(128, 256)))
        used = sorted(lens)
        d = D.Deflate()
        toks = [s for s in used if s < 256]
        toks += [(3 + k, 1 + 3 * k) for k in range(5)] + [97, 98, 99, 100, 101] + [(7, 40), (6, 2)]
        for rep in range(2 if eob_len != 12 else 1):      # two blocks: the end of block is decoded mid-stream too
            d.dynamic(toks, lens, None, final=rep == 1 or eob_len == 12)
        add("lit_walk_eob%d" % eob_len, d, True)

    # ---- 2. distance codes to 15 bits, all 30 symbols ----
    dl = D.fibonacci_lengths(list(range(30)))
    assert max(dl.values()) == 15 and len(dl) == 30
    d = D.Deflate()
    d.stored(noise(32768, 2))
    toks = []
    for ds in range(30):
        lo, hi = D.DIST_BASE[ds], D.DIST_BASE[ds] + (1 << D.DIST_EXTRA[ds]) - 1
        toks += [(3, lo), 120, (4, hi), 121]
    toks += [(258, 32768), (3, 32768)]
    d.dynamic(toks, None, dl, final=True)
    add("dist_lengths_to_15_all_30_min_max_extra", d, True)
    dl = D.random_complete_lengths(range(30), random.Random(5))
    d = D.Deflate()
    d.stored(noise(32768, 3))
    d.dynamic(toks, None, dl, final=True)
    add("dist_random_tree_all_30", d, True)

    # ---- 3. the code-length code ----
    # all 19 symbols in use, lengths up to 7 bits, HCLEN at its largest: 3 codes of 2 bits, 2 of 4, 2 of 6, 12 of 7
    syms = [256, 257, 65, 258] + list(range(66, 78))
    lens = D.as_vector(D.fibonacci_lengths(syms), 280)            # literal lengths 1 .. 15: code-length symbols 1 .. 15
    dist = [3, 3, 3, 3, 3, 3, 3, 3] + [0] * 4                      # (the kept zeros make a 17 run)
    seq = lens + dist
    cl = D.rle_code_lengths(seq)
    k = next(i for i, (s, _) in enumerate(cl) if s == 18)
    cl[k:k + 1] = [(18, cl[k][1] - 3), (17, 0)] if cl[k][1] >= 3 else cl[k:k + 1]
    k = max(i for i, (s, x) in enumerate(cl) if s == 17 and x >= 1)
    cl[k:k + 1] = [(17, cl[k][1] - 1), (0, 0)]
    assert {s for s, _ in cl} == set(range(19)), sorted({s for s, _ in cl})
    pre = [0] * 19
    for s, l in zip([0, 18, 3] + [16, 17] + [1, 2] + [4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15], [2] * 3 + [4] * 2 + [6] * 2 + [7] * 12):
        pre[s] = l
    d = D.Deflate()
    d.dynamic([s for s in syms if s < 256] + [(3, 2), (4, 8)], lens, dist, final=True, header=D.Header(cl=cl, pre=pre, nlen=280, ndist=12))
    add("precode_all_19_symbols_7_bits_hclen19", d, True)
    # the smallest HCLEN a valid block can have: 16 17 18 0 8, so every code is 8 bits long: 255 literals and the end of block
    lens = [8] * 255 + [0, 8]
    d = D.Deflate()
    d.dynamic(list(range(255)) * 2, lens, [], final=True, header=D.Header(pre=D.as_vector({8: 1, 0: 1}, 19), ncode=5, rle=dict(use16=False, use17=False, use18=False)))
    add("precode_hclen_smallest_valid", d, True)
    # HCLEN 0 (16 17 18 0 only) can say nothing but zeros: no end-of-block code
    d = D.Deflate()
    d.dynamic([], [0] * 257, [0], final=True, invalid=True, eob=False, header=D.Header(pre=D.as_vector({18: 1, 0: 1}, 19), ncode=4))
    add("precode_hclen0_all_zero_lengths", d, False)

    # ---- 4. code-length runs, accepted ----
    body = text(300, 4) + b"N" * 20
    toks = D.lz77(body)
    lf, df = D.token_symbols(toks)
    lens = D.as_vector(D.limited_lengths(lf), 286)
    dist = D.as_vector(D.limited_lengths(df), 30)
    seq = lens + dist
    cl = []
    for s, x in D.rle_code_lengths(seq):       # every long zero run ends in a 16: "repeat the previous length", which is 0
        if s == 18 and x >= 3:
            cl += [(18, x - 3), (16, 0)]
        elif s == 17 and x >= 3:
            cl += [(17, x - 3), (16, 0)]
        else:
            cl.append((s, x))
    assert any(a[0] in (17, 18) and b[0] == 16 for a, b in zip(cl, cl[1:]))
    d = D.Deflate()
    d.dynamic(toks, lens, dist, final=True, header=D.Header(cl=cl, nlen=286, ndist=30))
    add("clen_16_after_zero_run_repeats_zero", d, True)

    def crossing(cl, nlen):
        """the symbols of runs that cover both index nlen - 1 and nlen"""
        i, out = 0, set()
        for s, x in cl:
            n = 1 if s < 16 else (3 + x, 3 + x, 11 + x)[s - 16]
            if i < nlen < i + n:
                out.add(s)
            i += n
        return out

    # literal/length lengths end in 6 6 6 6 and the distance lengths begin 6 6 6 6: a 16 run over the boundary
    pinned = {256: 6, 257: 6, 258: 6, 259: 6, 260: 6}
    lens = D.as_vector(D.pinned_lengths(pinned, list(range(64, 123))), 261)
    dist = [6] * 4 + D.as_vector(D.pinned_lengths({0: 6, 1: 6, 2: 6, 3: 6}, list(range(4, 30)), 15), 30)[4:]
    cl = D.rle_code_lengths(lens + dist)
    assert 16 in crossing(cl, 261)
    toks = [s for s in range(64, 123) if lens[s]] + [(3, 1), (4, 2), (5, 3), (6, 4)]
    d = D.Deflate()
    d.dynamic(toks, lens, dist, header=D.Header(cl=cl, nlen=261, ndist=30))
    # kept trailing zeros up to HLIT = 29 and unused short distances: an 18 run over the boundary
    lens2 = D.as_vector(D.limited_lengths({65: 5, 66: 3, 67: 2, 256: 1, 257: 1}), 286)
    dist2 = D.as_vector({20: 1, 21: 1}, 22)
    cl2 = D.rle_code_lengths(lens2 + dist2)
    assert 18 in crossing(cl2, 286)
    d.dynamic([65, 66, 67] * 600 + [(3, 1100), (3, 1600)], lens2, dist2, final=True, header=D.Header(cl=cl2, nlen=286))
    add("clen_16_and_18_runs_span_lit_dist_boundary", d, True)
    # the same vectors with runs cut at the boundary and no 18 / no 16 / no 17 at all
    d = D.Deflate()
    d.dynamic(toks, lens, dist, header=D.Header(rle=dict(cuts=[261], use18=False)))
    d.dynamic(toks, lens, dist, header=D.Header(rle=dict(use16=False, max_run=5)))
    d.dynamic(toks, lens, dist, header=D.Header(rle=dict(use17=False, max_run=20), nlen=286, ndist=30))
    d.dynamic(toks, lens, dist, final=True, header=D.Header(rle=dict(use16=False, use17=False, use18=False)))
    add("clen_header_encodings_vary", d, True)

    # ---- 5. code-length runs, rejected ----
    lens = D.as_vector({65: 1, 256: 1}, 257)
    good = D.rle_code_lengths(lens + [0])
    d = D.Deflate()
    d.dynamic([65], lens, [0], final=True, invalid=True, header=D.Header(cl=[(16, 0)] + D.rle_code_lengths((lens + [0])[3:]), pre=D.as_vector({16: 2, 18: 2, 0: 2, 1: 2}, 19)))
    add("clen_16_as_first_symbol", d, False)          # (were "the previous length" 0, the three zeros would fit exactly)
    assert good[-1] == (0, 0) and good[-3][0] == 18
    d = D.Deflate()
    d.dynamic([65], lens, [0], final=True, invalid=True, header=D.Header(cl=good[:-1] + [(17, 0)], pre=D.as_vector({17: 2, 18: 2, 0: 2, 1: 2}, 19)))
    add("clen_run_past_nlen_plus_ndist", d, False)
    d = D.Deflate()
    d.dynamic([65], lens, [0], final=True, invalid=True, header=D.Header(cl=good[:-3] + [(18, 127)], pre=D.as_vector({17: 2, 18: 2, 0: 2, 1: 2}, 19)))
    add("clen_18_run_past_nlen_plus_ndist", d, False)

    # ---- 6. one distance code of one bit ----
    d = D.Deflate()
    d.dynamic([97, 98, (5, 1), 99, (3, 1)], None, {0: 1}, final=True)
    add("one_dist_code_bit0_used", d, True)
    d = D.Deflate()
    d.dynamic([97, 98, 99, (5, 3), 100], None, {2: 1}, final=True)
    add("one_dist_code_symbol2_bit0_used", d, True)
    d = D.Deflate()
    d.dynamic([97, 98, D.Raw(259), D.Bits(1, 1), 99], {97: 2, 98: 2, 99: 2, 256: 3, 259: 3}, {0: 1}, final=True)
    add("one_dist_code_bit1_is_no_code", d, False)

    # ---- 7. no distance code at all ----
    d = D.Deflate()
    d.dynamic(list(b"no distances here"), None, [0], final=True)
    add("no_dist_codes_literals_only", d, True)
    d = D.Deflate()
    d.dynamic([97, 98, 99, D.Raw(257), D.Bits(0, 1)], {97: 2, 98: 2, 99: 2, 256: 3, 257: 3}, [0], final=True)
    add("no_dist_codes_with_length_symbol", d, False)

    # ---- 8. the empty dynamic block ----
    d = D.Deflate()
    d.dynamic([], {256: 1}, [0], final=True)
    add("dynamic_only_eob_at_1_bit", d, True)
    d = D.Deflate()
    d.dynamic([], {256: 1}, [0])
    d.fixed(list(b"after an empty block"))
    d.dynamic([], {256: 1}, [0])
    d.dynamic([], {256: 1}, [0], final=True)
    add("dynamic_only_eob_between_data", d, True)

    # ---- 9. code sets zlib rejects ----
    for name, ll, dd, eob in (("incomplete_2_symbol_literal_code", {97: 2, 256: 2}, [0], True),
                              ("oversubscribed_literal_code", {97: 1, 98: 1, 256: 1}, [0], True),
                              ("oversubscribed_distance_code", {97: 1, 256: 1}, {0: 1, 1: 1, 2: 1}, True),
                              ("incomplete_distance_code_two_symbols", {97: 1, 256: 1}, {0: 2, 1: 2}, True),
                              ("missing_eob_code", {97: 1, 98: 1}, [0], False)):
        d = D.Deflate()
        d.dynamic([97], ll, dd, final=True, invalid=True, eob=eob)
        add(name, d, False)
    d = D.Deflate()
    d.dynamic([97], {97: 1, 256: 1}, [0], final=True, header=D.Header(pre=D.as_vector({18: 1, 1: 2, 0: 3}, 19), invalid=True))
    add("incomplete_precode", d, False)
    d = D.Deflate()
    d.dynamic([97], {97: 1, 256: 1}, [0], final=True, header=D.Header(pre=D.as_vector({18: 1, 1: 1, 0: 1}, 19), invalid=True))
    add("oversubscribed_precode", d, False)
    d = D.Deflate()
    d.dynamic([97], {97: 1, 256: 1}, [0], final=True, header=D.Header(pre=D.as_vector({18: 1}, 19), cl=[(18, 127), (18, 108)], invalid=True))
    add("single_symbol_precode", d, False)

    # ---- 10. header counts ----
    body = text(600, 6)
    toks = D.lz77(body) + [(258, 4), D.Raw(284, 30, 3, 0), D.Raw(284, 31, 2, 0), D.Raw(284, 0, 0, 0)]
    d = D.Deflate()
    d.dynamic(toks, final=True)
    add("hlit29_with_284_and_285", d, True)
    for nlen in (287, 288):
        d = D.Deflate()
        d.dynamic(D.lz77(body), final=True, header=D.Header(nlen=nlen))
        add("hlit_%d" % (nlen - 257), d, False)
    for ndist in (31, 32):
        d = D.Deflate()
        d.dynamic(D.lz77(body), final=True, header=D.Header(ndist=ndist))
        add("hdist_%d" % (ndist - 1), d, False)

    # ---- 11. lengths and the fixed code ----
    for long258 in (False, True):
        toks = list(b"abcdefgh")
        for n in range(3, 259):
            toks += [(n, 1 + n % 8), 48 + n % 10, 65 + n % 26]
        toks += [(258, 8), 10, 10, 10, (258, 1), 10, 10, 10]
        d = D.Deflate(long258=long258)
        d.fixed(toks)
        d.dynamic(toks, final=True)
        add("every_length_3_to_258_len258_as_%s" % ("284_31" if long258 else "285"), d, True)
    d = D.Deflate()
    d.fixed(list(range(144, 256)) + list(range(255, 143, -1)) + list(range(0, 144)), final=True)
    add("fixed_9_bit_literals_144_to_255", d, True)
    for sym in (286, 287):
        d = D.Deflate()
        d.fixed(list(b"abc") + [D.Raw(sym), 100], final=True)
        add("fixed_length_symbol_%d" % sym, d, False)
    for sym in (30, 31):
        d = D.Deflate()
        d.fixed(list(b"abc") + [D.Raw(257, 0, sym, 0), 100], final=True)
        add("fixed_distance_symbol_%d" % sym, d, False)
    d = D.Deflate()
    d.dynamic(list(b"abc") + [D.Raw(257, 0, 30, 0), 100], None, D.as_vector(D.limited_lengths({0: 1, 30: 1}), 31), final=True, invalid=True,
              header=D.Header(ndist=31))
    add("dynamic_distance_symbol_30", d, False)

    # ---- 12. stored blocks ----
    d = D.Deflate()
    d.fixed(list(b"before"))
    d.stored(b"")
    d.stored(b"", pad="ones")
    d.dynamic(list(b"between"))
    d.stored(noise(65535, 7))
    d.stored(b"")
    d.fixed(list(b"after"), final=True)
    add("stored_len0_midstream_and_len65535", d, True)
    d = D.Deflate()
    d.fixed(list(b"data then a final stored block "))
    d.stored(b"the end", final=True, pad="ones")
    add("stored_final_block", d, True)
    d = D.Deflate()
    d.stored(b"", final=True)
    add("stored_lone_final_len0", d, True)
    for pad, pname in ((0, "zero"), ("ones", "ones"), (random.Random(12), "random")):
        d = D.Deflate()
        for j in range(24):
            d.fixed([144 + (5 * j + i) % 112 for i in range(j % 8)])      # 10 + 9 (j % 8) bits: every alignment
            d.stored(b"<%d>" % j * (j % 3), pad=pad)
        d.fixed([], final=True)
        assert d.stored_align == set(range(8))
        add("stored_at_8_alignments_pad_%s" % pname, d, True, pad=pad)
    d = D.Deflate()
    d.stored(b"abc", final=True, nlen=0x1234)
    add("stored_len_nlen_mismatch", d, False)
    d = D.Deflate()
    d.stored(b"abc", final=True, length=9)
    add("stored_longer_than_input", d, False)

    # ---- 13. stored blocks that hold a gzip member: magic and valid dynamic headers inside data ----
    inner = G.gz(G.fastq(260, seed=13), 6)
    d = D.Deflate()
    d.fixed(list(b"wrapped:"))
    for i in range(0, len(inner), 9000):
        d.stored(inner[i:i + 9000], pad="ones" if i % 18000 else 0)
    d.dynamic(list(b":done"), final=True)
    add("stored_payload_is_a_gzip_member", d, True)

    # ---- 14. block counts ----
    rng = random.Random(14)
    body = text(40000, 14, b"ACGTN\n")
    d = D.Deflate()
    i = k = 0
    while i < len(body) and (k < 5200 or i < 24000):
        n = rng.randint(1, 8)
        piece = body[i:i + n]
        if k % 3 == 0:
            d.stored(piece, pad=rng)
        elif k % 3 == 1:
            d.fixed(D.lz77(body[:i + n], start=i, max_dist=rng.choice([8, 300, 32768])))
        else:
            d.dynamic(D.lz77(body[:i + n], start=i))
        i += len(piece)
        k += 1
    d.stored(b"", final=True)
    assert d.n_blocks >= 5000
    add("5000_tiny_blocks_types_alternate", d, True)
    d = D.Deflate()
    for kind in range(3):
        d.dynamic(D.lz77(body[:3000 * (kind + 1)], start=3000 * kind))
        for _ in range(1000):
            if kind == 0:
                d.fixed([])
            elif kind == 1:
                d.dynamic([], {256: 1}, [0])
            else:
                d.stored(b"")
    d.fixed(D.lz77(body[:10000], start=9000), final=True)
    add("runs_of_1000_empty_blocks", d, True)

    # ---- 15. one dynamic block for a whole 2 MB member ----
    rng = random.Random(15)
    reads = [text(rng.randint(200, 900), 1500 + i) for i in range(40)]
    toks, n = [], 0
    while n < 2 << 20:
        r = rng.choice(reads)
        a = rng.randrange(0, len(r) - 60)
        k = rng.randint(20, 60)
        head = b"@r%d\n" % n
        toks += list(head) + list(r[a:a + k])
        n += len(head) + k
        L = rng.randint(30, 258)
        toks += [(L, rng.randint(1, min(32768, n))), 10]
        n += L + 1
    d = D.Deflate()
    d.dynamic(toks, final=True)
    assert len(d.out) >= 2 << 20 and d.n_blocks == 1
    add("one_dynamic_block_2mb_member", d, True)

    # ---- 16. matches ----
    d = D.Deflate()
    d.stored(noise(700, 16))
    d.fixed(list(b"fixed block text ") + [(20, 700), (9, 717)])
    d.stored(text(300, 16))
    d.dynamic([(258, 300), 65, (100, 1017 + 259), (30, 1), (258, 259 + 131 + 258 + 300)], final=True)
    add("matches_reach_into_earlier_blocks_and_stored", d, True)
    d = D.Deflate()
    d.fixed(list(b"abcdefgh"))
    toks = []
    for dist in range(1, 9):
        toks += [(258, dist), 48 + dist, 10, 58]
    d.fixed(toks * 6)
    d.dynamic(toks * 6, final=True)
    add("overlap_dist1to8_len258", d, True)
    d = D.Deflate()
    d.fixed(list(b"abcdefgh"))
    d.dynamic([(258, dist) for dist in range(1, 9)] * 160, final=True)
    add("overlap_dist1to8_len258_pure", d, True)
    d = D.Deflate()
    d.fixed(list(b"abc") + [(3, 3), (258, 6)], final=True)
    add("distance_equals_position", d, True)
    d = D.Deflate()
    d.fixed(list(b"abc") + [(3, 4)], final=True)
    add("distance_is_position_plus_1", d, False)
    d = D.Deflate()
    d.stored(noise(32767, 17))
    d.dynamic([(5, 32767), (4, 32768)], final=True)
    add("distance_32768_equals_position", d, True)
    d = D.Deflate()
    d.stored(noise(32767, 17))
    d.dynamic([(5, 32768)], final=True)
    add("distance_32768_is_position_plus_1", d, False)
    d = D.Deflate()
    d.fixed([(3, 1)], final=True)
    add("match_as_first_symbol", d, False)

    # ---- 17. padding bits before the trailer ----
    for pad, pname in (("ones", "ones"), (random.Random(18), "random")):
        for extra in range(4):
            d = D.Deflate()
            d.fixed(list(b"padding") + [200] * extra, final=True)
            add("last_byte_padding_%s_%d" % (pname, extra), d, True, pad=pad)

    # ---- damage that the fixed code has a name for ----
    d = D.Deflate()
    d.w.bits(1, 1)
    d.w.bits(3, 2)
    add("btype_3", d, False)
    d = D.Deflate()
    d.fixed(list(b"no final block"))
    add("no_final_block", d, False)
    return cases


def _provenance():
    """case 20: 3 MB in which every byte but the mixed-in literals descends from the first 32 KiB through distance-32768 matches"""
    rng = random.Random(20)
    d = D.Deflate()
    d.stored(noise(32768, 20))
    n = 32768
    while n < 3 << 20:
        toks = []
        for _ in range(150):                  # blocks of about 400 compressed bytes: a window hand-over in nearly every 512-byte chunk
            L = rng.randint(16, 48)
            toks.append((L, 32768))
            n += L
            if rng.random() < 0.1:
                toks.append(rng.randrange(256))
                n += 1
        d.dynamic(toks)
    d.fixed([], final=True)
    return d


RAW = _build()
_prov = _provenance()
note(_prov)
RAW.append(Case("provenance_chains_of_distance_32768", _prov.finish(), zlib_raw(_prov.finish()), bytes(_prov.out)))
assert RAW[-1].expected == RAW[-1].claimed
BY_NAME = {c.name: c for c in RAW}


def raw_cases():
    """[Case(name, raw deflate, expected bytes or None, claimed bytes)]"""
    return RAW


# ------------------------------------------------------------------------------------------------------------------------
# wrappers
# ------------------------------------------------------------------------------------------------------------------------
def member(raw, plain):
    return G.gz_header(plain, comp=raw)


def _writer_fastq_member(data, style):
    d = D.Deflate()
    if style == "tiny":
        rng = random.Random(len(data))
        i = 0
        while i < len(data):
            n = rng.randint(200, 700)
            toks = D.lz77(data[:i + n], start=i)
            (d.dynamic if rng.random() < 0.7 else d.fixed)(toks)
            i += n
        d.stored(b"", final=True)
    else:                                              # one code with 15-bit lengths per 20 KB block
        for i in range(0, len(data), 20000):
            toks = D.lz77(data[:i + 20000], start=i)
            lf, df = D.token_symbols(toks)
            ll = D.fibonacci_lengths(sorted(lf, key=lambda s: lf[s]))
            dd = D.fibonacci_lengths(sorted(df, key=lambda s: df[s])) if df else [0]
            d.dynamic(toks, ll, dd, final=i + 20000 >= len(data))
    note(d)
    raw = d.finish("ones")
    assert zlib_raw(raw) == data
    return raw


def fastq_files():
    """{name: (gzip or BGZF bytes, plain FASTQ)}: FASTQ through the writer, many tiny blocks and 15-bit codes, gzip and BGZF"""
    fq = G.fastq(160, seed=21)
    out = {}
    for style in ("tiny", "deep"):
        out["gzip_" + style] = (member(_writer_fastq_member(fq, style), fq), fq)
        blocks = [W.bgzf_block(fq[i:i + 30000], comp=_writer_fastq_member(fq[i:i + 30000], style)) for i in range(0, len(fq), 30000)]
        out["bgzf_" + style] = (b"".join(blocks) + W.EOF_BLOCK, fq)
    return out


def fastq_rejected():
    """a gzip FASTQ whose second member reaches into the first: zlib rejects it"""
    fq = G.fastq(60, seed=22)
    d = D.Deflate()
    d.dynamic(D.lz77(fq[:5000]), final=True)
    e = D.Deflate()
    e.dynamic([(40, 3000)] + D.lz77(fq[5040:9000]), final=True)
    data = member(d.finish(), fq[:5000]) + member(e.finish(), bytes(e.out))
    assert zlib_gzip(data) is None
    return data


def _gzip_cases():
    out = [(c.name, member(c.raw, c.claimed), c.expected) for c in RAW]
    pick = lambda *names: [BY_NAME[n] for n in names]   # noqa: E731
    # 18. multi-member files of writer-made members, some empty, one a lone final stored block of LEN 0
    ms = pick("lit_walk_eob15", "stored_lone_final_len0", "dist_lengths_to_15_all_30_min_max_extra", "dynamic_only_eob_at_1_bit",
              "5000_tiny_blocks_types_alternate", "stored_lone_final_len0", "stored_at_8_alignments_pad_random", "last_byte_padding_ones_1",
              "stored_payload_is_a_gzip_member", "every_length_3_to_258_len258_as_284_31", "stored_lone_final_len0")
    out.append(("multi_member_writer_made_some_empty", b"".join(member(c.raw, c.claimed) for c in ms), b"".join(c.expected for c in ms)))
    ms = pick("stored_lone_final_len0", "dynamic_only_eob_at_1_bit") * 40
    out.append(("multi_member_80_empty_members", b"".join(member(c.raw, c.claimed) for c in ms), b""))
    # 19. member k+1 reaches before its own first byte: the bytes would be member k's.  The header of member k+1 and the bad
    # reference are 12 KB of compressed data apart: in different chunks at 512 .. 4096-byte chunks, in different rounds at
    # 8 KiB rounds
    a = D.Deflate()
    a.dynamic(D.lz77(text(30000, 19)), final=True)
    note(a)
    hist = bytes(a.out)
    for name, dist_of in (("far", lambda pos: 20000), ("by_1", lambda pos: pos + 1), ("window", lambda pos: 32768)):
        # (the trailer of member k+1 is that of the bytes a decoder would get that let the match read member k: only the
        # distance check can refuse the file, not the CRC)
        b = D.Deflate(history=hist)
        for j in range(20):
            b.dynamic(list(noise(600, 1900 + j)))
        n = len(b.plain())
        b.dynamic([(10, dist_of(n))] + list(b"tail"), final=True)
        note(b)
        assert n < dist_of(n) <= n + len(hist)
        data = member(a.finish(), hist) + member(b.finish(), b.plain())
        out.append(("member_reaches_into_previous_member_%s" % name, data, None))
        # the same reference inside one member is fine: the case is about the member boundary, nothing else
        c = D.Deflate()
        c.dynamic(D.lz77(text(30000, 19)))
        for j in range(20):
            c.dynamic(list(noise(600, 1900 + j)))
        c.dynamic([(10, dist_of(len(c.out) - 30000))] + list(b"tail"), final=True)
        out.append(("same_reference_within_one_member_%s" % name, member(c.finish(), bytes(c.out)), bytes(c.out)))
    # the member header and the reference in one chunk: the decoder knows the member's first symbol itself
    small = BY_NAME["lit_walk_eob14"]
    for name, toks in (("first_symbol", [(3, 1)] + list(b"abc")), ("by_1", list(b"abc") + [(3, 4)]), ("far", list(b"abcdef") + [(5, 40)])):
        b = D.Deflate(history=small.expected)
        b.fixed(toks, final=True)
        data = member(small.raw, small.expected) + member(b.finish(), b.plain())
        out.append(("small_member_reaches_into_previous_member_%s" % name, data, None))
    # trailers
    c = BY_NAME["lit_walk_eob13"]
    out.append(("trailer_crc_wrong", G.gz_header(c.claimed, comp=c.raw, crc=zlib.crc32(c.claimed) ^ 1), None))
    out.append(("trailer_isize_wrong", G.gz_header(c.claimed, comp=c.raw, isize=len(c.claimed) + 1), None))
    for name, data, exp in out:
        got = zlib_gzip(data)
        assert got == exp, "zlib and the corpus differ on gzip case %s" % name
    return out


GZIP = _gzip_cases()


def gzip_cases():
    """[(name, gzip file, expected bytes or None)]"""
    return GZIP


def bgzf_fits(c):
    return len(c.claimed) <= 65536 and len(c.raw) + 26 <= 65536


def bgzf_reach_files():
    """[(name, BGZF file, offset of the bad block)]: a block whose match reaches into the block before it, with the CRC of
    the bytes a decoder would get that allowed it.  zlib rejects each."""
    first = BY_NAME["lit_walk_eob14"]
    out = []
    for name, toks in (("first_symbol", [(3, 1)] + list(b"abc")), ("by_1", list(b"abc") + [(3, 4)]), ("far", list(b"abcdef") + [(5, 40)])):
        b = D.Deflate(history=first.expected)
        b.fixed(toks, final=True)
        head = W.bgzf_block(first.expected, comp=first.raw)
        data = head + W.bgzf_block(b.plain(), comp=b.finish()) + head + W.EOF_BLOCK
        assert zlib_gzip(data) is None
        out.append(("block_reaches_into_previous_block_" + name, data, len(head)))
    return out


def bgzf_cases():
    """[(name, one BGZF block, expected bytes or None)]: every raw case that fits in a block (a rejected one with the CRC and
    ISIZE of what it claims).  Inside BGZF a block is a member, so the legal reach of a match is the block."""
    return [(c.name, W.bgzf_block(c.claimed, comp=c.raw), c.expected) for c in RAW if bgzf_fits(c)]


# ------------------------------------------------------------------------------------------------------------------------
# slots: the reference decides that no accepted case outside DENSE can end in TOO_MANY
# ------------------------------------------------------------------------------------------------------------------------
def max_piece_output(data, chunk):
    """the most bytes zlib yields for one chunk-sized piece of a gzip file (members followed)"""
    o = zlib.decompressobj(31)
    worst = 0
    for i in range(0, len(data), chunk):
        piece, got = data[i:i + chunk], 0
        while piece:
            got += len(o.decompress(piece))
            piece = b""
            if o.eof:
                piece = o.unused_data
                o = zlib.decompressobj(31)
        worst = max(worst, got)
    return worst


def slot_table():
    """{(name, chunk, ratio): (most bytes per piece, slot)} for the accepted gzip cases"""
    out = {}
    for name, data, exp in GZIP:
        if exp is None:
            continue
        for chunk in sorted({c for c, _ in SLOTS}):
            worst = max_piece_output(data, chunk)
            for c, ratio in SLOTS:
                if c == chunk:
                    out[(name, chunk, ratio)] = (worst, ratio * chunk)
    return out


assert len(DENSE) <= 3
for (_name, _chunk, _ratio), (_worst, _slot) in slot_table().items():
    assert _name in DENSE or _worst <= _slot, "case %s is too dense for chunk %d ratio %d: %d > %d" % (_name, _chunk, _ratio, _worst, _slot)


# ------------------------------------------------------------------------------------------------------------------------
# property cases
# ------------------------------------------------------------------------------------------------------------------------
def random_stream(rng, max_tokens=300):
    """(raw deflate, plain): a random token stream over a small alphabet with planted repeats, cut at random into blocks of
    random types, dynamic blocks with random complete code trees (unused symbols included) and random header encodings"""
    d = D.Deflate(long258=rng.random() < 0.5)
    alphabet = [rng.randrange(256) for _ in range(rng.randint(1, 6))]
    n_blocks = rng.randint(1, 6)
    for blk in range(n_blocks):
        final = blk == n_blocks - 1
        kind = rng.choice(["stored", "fixed", "dynamic", "dynamic"])
        if kind == "stored":
            d.stored(bytes(rng.choice(alphabet) for _ in range(rng.choice([0, 1, rng.randint(0, 200)]))), final=final, pad=rng)
            continue
        toks, pos = [], len(d.out)
        for _ in range(rng.choice([0, 1, rng.randint(0, max_tokens)])):
            if pos and rng.random() < 0.35:
                L = rng.choice([3, 4, 10, 257, 258, rng.randint(3, 258)])
                dist = rng.choice([1, pos, min(pos, 32768), rng.randint(1, min(pos, 32768))])
                dist = min(dist, pos, 32768)
                toks.append((L, dist))
                pos += L
            else:
                toks.append(rng.choice(alphabet))
                pos += 1
        if kind == "fixed":
            d.fixed(toks, final=final)
            continue
        lf, df = D.token_symbols(toks, d.long258)
        ls = set(lf) | {rng.randrange(286) for _ in range(rng.choice([0, 0, 3, 40]))}
        ds = set(df) | {rng.randrange(30) for _ in range(rng.choice([0, 0, 2, 12]))}
        ll = D.as_vector(D.random_complete_lengths(sorted(ls), rng), 286)
        dd = D.as_vector(D.random_complete_lengths(sorted(ds), rng), 30) if ds else [0] * 30
        trim = lambda v, lo: max(lo, max([i + 1 for i, l in enumerate(v) if l] + [0]))   # noqa: E731
        nlen, ndist = rng.randint(trim(ll, 257), 286), rng.randint(trim(dd, 1), 30)
        rle = dict(use16=rng.random() < 0.8, use17=rng.random() < 0.8, use18=rng.random() < 0.8, max_run=rng.choice([3, 4, 7, 11, 50, 138]),
                   cuts=[nlen] if rng.random() < 0.3 else [])
        d.dynamic(toks, ll, dd, final=final, header=D.Header(nlen=nlen, ndist=ndist, rle=rle))
    raw = d.finish(rng)
    return raw, bytes(d.out), d
