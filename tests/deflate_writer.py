"""A deflate writer from RFC 1951 alone, for the tests: no zlib on the encode side (zlib.crc32 for gzip trailers only).  It
leaves every choice an encoder has to the caller -- block types and cuts, stored blocks at any bit offset with any padding,
code lengths up to 15 bits, the header encoding of a dynamic block (HLIT / HDIST / HCLEN, which of 16 / 17 / 18, how runs are
cut), both encodings of length 258 -- and can write symbols that no valid stream holds.  While it writes it keeps `out`, the
bytes a decoder that followed the tokens would produce (a reference before the first byte reads as '?'), so a rejected stream
can be wrapped with a trailer that fits what it claims."""
import heapq
import struct
import zlib

CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


# ---- bits ----
class BitWriter:
    """RFC 1951 section 3.1.1: fields LSB first, Huffman codes MSB first, bytes filled from bit 0."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, v, k):
        assert 0 <= v < (1 << k) or k == 0
        self.acc |= v << self.n
        self.n += k
        if self.n >= 64:
            m = self.n >> 3
            self.buf += (self.acc & ((1 << (8 * m)) - 1)).to_bytes(m, "little")
            self.acc >>= 8 * m
            self.n -= 8 * m

    def code(self, c, k):
        self.bits(int(format(c, "0%db" % k)[::-1], 2) if k else 0, k)

    def bitpos(self):
        return 8 * len(self.buf) + self.n

    def align(self, pad=0):
        """to a byte boundary; the padding bits come from `pad`: an int (its low bits, LSB first), "ones", or a random.Random"""
        k = -self.bitpos() & 7
        if pad == "ones":
            v = (1 << k) - 1
        elif hasattr(pad, "getrandbits"):
            v = pad.getrandbits(k) if k else 0
        else:
            v = pad & ((1 << k) - 1)
        self.bits(v, k)
        return k

    def raw(self, data):
        assert self.bitpos() & 7 == 0
        m = self.n >> 3
        self.buf += self.acc.to_bytes(m, "little")
        self.acc, self.n = 0, 0
        self.buf += data

    def getvalue(self, pad=0):
        self.align(pad)
        self.raw(b"")
        return bytes(self.buf)


# ---- codes ----
def kraft(lens, maxbits=15):
    """sum of 2^(maxbits - l) over the codes: 2^maxbits when complete"""
    return sum(1 << (maxbits - l) for l in lens if l)


def is_valid_code(lens, strict=False):
    """what RFC 1951 and zlib allow: complete; or (not the code-length code) no code at all or a single code of 1 bit"""
    used = [l for l in lens if l]
    if kraft(lens) == 1 << 15:
        return True
    return not strict and (not used or used == [1])


def canonical(lens):
    """RFC 1951 section 3.2.2: {symbol: (code, length)}"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def huffman_lengths(freqs):
    """{symbol: freq > 0} -> {symbol: length}, unlimited depth (one symbol: 1 bit)"""
    if len(freqs) == 1:
        return {s: 1 for s in freqs}
    heap = [(f, i, (s,)) for i, (s, f) in enumerate(sorted(freqs.items()))]
    heapq.heapify(heap)
    depth = {s: 0 for s in freqs}
    tick = len(heap)
    while len(heap) > 1:
        fa, _, a = heapq.heappop(heap)
        fb, _, b = heapq.heappop(heap)
        for s in a + b:
            depth[s] += 1
        heapq.heappush(heap, (fa + fb, tick, a + b))
        tick += 1
    return depth


def limited_lengths(freqs, maxbits=15):
    """a complete prefix code of depth <= maxbits for the symbols of `freqs`, close to optimal: Huffman lengths clamped to
    maxbits, then the Kraft sum repaired (cheapest symbols lengthened while over-subscribed, longest codes shortened while
    incomplete)"""
    depth = huffman_lengths(freqs)
    if len(depth) == 1:
        return depth
    assert len(depth) <= 1 << maxbits
    for s in depth:
        depth[s] = min(depth[s], maxbits)
    full = 1 << maxbits
    k = sum(1 << (maxbits - l) for l in depth.values())
    order = sorted(depth, key=lambda s: (freqs[s], s))
    while k > full:
        s = max((s for s in order if depth[s] < maxbits), key=lambda s: (depth[s], -freqs[s]))
        k -= 1 << (maxbits - depth[s] - 1)
        depth[s] += 1
    while k < full:
        fit = [s for s in order if depth[s] > 1 and (1 << (maxbits - depth[s])) <= full - k]
        s = max(fit, key=lambda s: (depth[s], freqs[s]))
        k += 1 << (maxbits - depth[s])
        depth[s] -= 1
    return depth


def fibonacci_lengths(symbols, maxbits=15):
    """Fibonacci weights give the deepest Huffman tree there is: lengths 1, 2, 3, ... so that 11 .. 15 all occur (the first
    symbol gets the longest code); more than maxbits + 1 symbols are limited to maxbits"""
    a, b, freqs = 1, 1, {}
    for s in symbols:
        freqs[s] = a
        a, b = b, a + b
    return limited_lengths(freqs, maxbits)


def random_complete_lengths(symbols, rng, maxbits=15):
    """a random complete tree of depth <= maxbits whose leaves are `symbols` in random order"""
    symbols = list(symbols)
    if len(symbols) == 1:
        return {symbols[0]: 1}
    leaves = [1, 1]
    while len(leaves) < len(symbols):
        can = [i for i, d in enumerate(leaves) if d < maxbits]
        i = rng.choice(can) if rng.random() < 0.5 else max(can, key=lambda j: leaves[j])
        leaves[i] += 1
        leaves.append(leaves[i])
    rng.shuffle(symbols)
    return dict(zip(symbols, leaves))


def pinned_lengths(pinned, fillers, maxbits=15):
    """a complete code in which the symbols of `pinned` ({symbol: length}) have exactly those lengths; the rest of the code
    space goes to as many of `fillers` as it takes (at most all of them, split as evenly as the space allows)"""
    space = (1 << maxbits) - sum(1 << (maxbits - l) for l in pinned.values())
    assert space >= 0, "pinned lengths are over-subscribed"
    parts = [maxbits - i for i in range(maxbits + 1) if space >> i & 1]      # the fewest codes that fill the space
    assert len(parts) <= len(fillers), "not enough filler symbols"
    parts.sort()
    while len(parts) < len(fillers) and parts[0] < maxbits:
        l = parts.pop(0)
        parts += [l + 1, l + 1]
        parts.sort()
    out = dict(pinned)
    out.update(zip(fillers, parts))
    assert kraft(out.values(), maxbits) == 1 << maxbits
    return out


def as_vector(lengths, n):
    v = [0] * n
    for s, l in lengths.items():
        v[s] = l
    return v


# ---- symbols ----
def length_symbol(length, long258=False):
    """(symbol, extra bits, extra value); 258 as 285, or as 284 with extra 31"""
    assert 3 <= length <= 258
    if length == 258:
        return (284, 5, 31) if long258 else (285, 0, 0)
    i = max(j for j in range(28) if LEN_BASE[j] <= length)
    return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    i = max(j for j in range(30) if DIST_BASE[j] <= dist)
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


_LEN_SYM = {}
_DIST_SYM = {}


def _reversed(codes):
    return {s: (int(format(c, "0%db" % l)[::-1], 2), l) for s, (c, l) in codes.items()}


_FIXED = (_reversed(canonical(FIXED_LIT)), _reversed(canonical(FIXED_DIST)))


class Raw:
    """A length / distance pair written symbol by symbol: any symbol numbers (286, 287, distance 30, 31 too) and any extra
    bits.  dsym None: the length symbol alone."""

    def __init__(self, lsym, lextra=0, dsym=None, dextra=0, lbits=None, dbits=None):
        self.lsym, self.lextra, self.dsym, self.dextra = lsym, lextra, dsym, dextra
        self.lbits = lbits if lbits is not None else (LEN_EXTRA[lsym - 257] if 257 <= lsym <= 285 else 0)
        self.dbits = dbits if dbits is not None else (DIST_EXTRA[dsym] if dsym is not None and dsym < 30 else 0)


class Bits:
    """raw bits in the middle of a block's symbols (a bit pattern that is no code, say); no output"""

    def __init__(self, value, nbits):
        self.value, self.nbits = value, nbits


def token_symbols(tokens, long258=False):
    """(literal/length symbols, distance symbols) that `tokens` use, with their counts; the end-of-block symbol included"""
    lit, dist = {256: 1}, {}
    for t in tokens:
        if isinstance(t, int):
            lit[t] = lit.get(t, 0) + 1
        elif isinstance(t, Bits):
            continue
        elif isinstance(t, Raw):
            lit[t.lsym] = lit.get(t.lsym, 0) + 1
            if t.dsym is not None:
                dist[t.dsym] = dist.get(t.dsym, 0) + 1
        else:
            ls = length_symbol(t[0], long258)[0]
            ds = dist_symbol(t[1])[0]
            lit[ls] = lit.get(ls, 0) + 1
            dist[ds] = dist.get(ds, 0) + 1
    return lit, dist


def lz77(data, min_match=3, max_match=258, max_dist=32768, start=0, history=True):
    """A small greedy parser: tokens for data[start:], matches found through the last position of each min_match-gram
    (history=False: no match reaches before `start`)."""
    out, last, i, n = [], {}, start, len(data)
    k = max(3, min_match)
    if history:
        for j in range(max(0, start - max_dist), max(0, start - k + 1)):
            last[data[j:j + k]] = j
    while i < n:
        key = data[i:i + k]
        j = last.get(key) if len(key) == k else None
        if j is not None and i - j <= max_dist:
            m = k
            lim = min(max_match, n - i)
            while m < lim and data[j + m] == data[i + m]:
                m += 1
            for q in range(i, min(i + m, n - k + 1)):
                last[data[q:q + k]] = q
            out.append((m, i - j))
            i += m
        else:
            if len(key) == k:
                last[key] = i
            out.append(data[i])
            i += 1
    return out


# ---- the dynamic block header ----
def rle_code_lengths(seq, use16=True, use17=True, use18=True, max_run=138, cuts=()):
    """the code-length sequence as (symbol, extra value) pairs.  Runs are cut at most max_run long and never cross an index
    in `cuts` (pass [nlen] to keep runs from crossing the literal/distance boundary; by default they cross it)."""
    out, i, n = [], 0, len(seq)
    cuts = set(cuts)
    while i < n:
        v = seq[i]
        j = i + 1
        while j < n and seq[j] == v and j not in cuts:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11 and use18:
                r = min(run, 138, max(11, max_run))
                out.append((18, r - 11)); run -= r
            while run >= 3 and use17:
                r = min(run, 10, max(3, max_run))
                out.append((17, r - 3)); run -= r
            out += [(0, 0)] * run
        else:
            out.append((v, 0)); run -= 1
            while run >= 3 and use16:
                r = min(run, 6, max(3, max_run))
                out.append((16, r - 3)); run -= r
            out += [(v, 0)] * run
        i = j
    return out


class Header:
    """How a dynamic block's header is written.  Everything left None is chosen the usual way.
    nlen / ndist: how many literal/length and distance lengths are sent (trailing zeros kept up to that count; nlen 287 / 288
    and ndist 31 / 32 write HLIT 30 / 31 and HDIST 30 / 31, which no decoder may accept)
    cl: the code-length symbols as (symbol, extra value) pairs, instead of rle_code_lengths(**rle)
    pre: the 19 lengths of the code-length code (checked complete unless invalid=True)
    ncode: how many of them are sent (HCLEN + 4), 4 .. 19"""

    def __init__(self, nlen=None, ndist=None, cl=None, pre=None, ncode=None, rle=None, invalid=False):
        self.nlen, self.ndist, self.cl, self.pre, self.ncode, self.rle, self.invalid = nlen, ndist, cl, pre, ncode, rle or {}, invalid


class Deflate:
    """One raw deflate stream written block by block.  `out` is what the tokens say the output is."""

    def __init__(self, long258=False, history=b""):
        """history: bytes that precede the stream (an earlier member or block); a match may read them in `out`, which a
        conforming decoder refuses"""
        self.w = BitWriter()
        self.out = bytearray(history)
        self.base = len(history)
        self.long258 = long258
        self.max_lit_len = 0          # the longest literal/length and distance codes of the dynamic blocks written
        self.max_dist_len = 0
        self.stored_align = set()     # bit offsets (mod 8) at which stored block headers began
        self.n_blocks = 0
        self.enc258 = set()           # how length 258 was written: "285", "284+31"

    # -- blocks --
    def stored(self, data, final=False, pad=0, length=None, nlen=None):
        """a stored block at the current bit offset.  pad: see BitWriter.align.  length / nlen: the LEN and NLEN fields when
        they shall not be len(data) and its complement"""
        self.stored_align.add(self.w.bitpos() & 7)
        self.w.bits(1 if final else 0, 1)
        self.w.bits(0, 2)
        self.w.align(pad)
        n = len(data) if length is None else length
        assert 0 <= n <= 65535
        self.w.raw(struct.pack("<HH", n, (n ^ 0xFFFF) if nlen is None else nlen) + bytes(data))
        self.out += data
        self.n_blocks += 1

    def fixed(self, tokens, final=False, eob=True):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(1, 2)
        self._tokens(tokens, _FIXED[0], _FIXED[1], eob)
        self.n_blocks += 1

    def dynamic(self, tokens, litlens=None, distlens=None, final=False, header=None, eob=True, invalid=False):
        """a dynamic block.  litlens / distlens: code-length vectors (lists, or {symbol: length}); by default
        limited_lengths over the symbols the tokens use.  invalid=True: the vectors need not be valid codes."""
        lf, df = token_symbols(tokens, self.long258)
        if litlens is None:
            litlens = limited_lengths(lf)
        if distlens is None:
            distlens = limited_lengths(df) if df else {}
        if isinstance(litlens, dict):
            litlens = as_vector(litlens, max(list(litlens) + [256]) + 1)
        if isinstance(distlens, dict):
            distlens = as_vector(distlens, max(list(distlens) + [0]) + 1)
        if not invalid:
            assert is_valid_code(litlens) and is_valid_code(distlens), "not a valid code (pass invalid=True to write it anyway)"
            assert len(litlens) <= 286 and len(distlens) <= 30
        self.max_lit_len = max([self.max_lit_len] + list(litlens))
        self.max_dist_len = max([self.max_dist_len] + list(distlens))
        self.w.bits(1 if final else 0, 1)
        self.w.bits(2, 2)
        self._header(list(litlens), list(distlens), header or Header())
        self._tokens(tokens, _reversed(canonical(litlens)), _reversed(canonical(distlens)), eob)
        self.n_blocks += 1

    def finish(self, pad=0):
        return self.w.getvalue(pad)

    def plain(self):
        """what the tokens say this stream's own output is (without the history)"""
        return bytes(self.out[self.base:])

    # -- pieces --
    def _header(self, litlens, distlens, h):
        trim = lambda v, lo: max(lo, max([i + 1 for i, l in enumerate(v) if l] + [0]))   # noqa: E731
        nlen = h.nlen if h.nlen is not None else trim(litlens, 257)
        ndist = h.ndist if h.ndist is not None else trim(distlens, 1)
        assert 257 <= nlen <= 288 and 1 <= ndist <= 32
        seq = (litlens + [0] * 288)[:nlen] + (distlens + [0] * 32)[:ndist]
        cl = h.cl if h.cl is not None else rle_code_lengths(seq, **h.rle)
        pre = h.pre
        if pre is None:
            freqs = {}
            for s, _ in cl:
                freqs[s] = freqs.get(s, 0) + 1
            if len(freqs) == 1:                       # the code-length code must be complete: give it a second symbol
                freqs[(next(iter(freqs)) + 1) % 19] = 1
            pre = as_vector(limited_lengths(freqs, 7), 19)
        assert len(pre) == 19 and max(pre) <= 7
        assert h.invalid or is_valid_code(pre, strict=True), "incomplete code-length code"
        ncode = h.ncode if h.ncode is not None else max(4, max(i + 1 for i in range(19) if pre[CLEN_ORDER[i]]))
        assert 4 <= ncode <= 19 and all(pre[CLEN_ORDER[i]] == 0 for i in range(ncode, 19)), "HCLEN cuts a used symbol"
        w = self.w
        w.bits(nlen - 257, 5)
        w.bits(ndist - 1, 5)
        w.bits(ncode - 4, 4)
        for i in range(ncode):
            w.bits(pre[CLEN_ORDER[i]], 3)
        codes = canonical(pre)
        for s, x in cl:
            c, l = codes[s]
            w.code(c, l)
            if s >= 16:
                w.bits(x, (2, 3, 7)[s - 16])

    def _tokens(self, tokens, lit, dist, eob):
        """lit / dist: {symbol: (bit-reversed code, length)}"""
        w, out, long258 = self.w, self.out, self.long258
        for t in tokens:
            if isinstance(t, int):
                c, l = lit[t]
                w.bits(c, l)
                out.append(t)
                continue
            if isinstance(t, Bits):
                w.bits(t.value, t.nbits)
                continue
            if isinstance(t, Raw):
                c, l = lit[t.lsym]
                w.bits(c, l)
                w.bits(t.lextra, t.lbits)
                if t.dsym is None:
                    continue
                c, l = dist[t.dsym]
                w.bits(c, l)
                w.bits(t.dextra, t.dbits)
                if not (257 <= t.lsym <= 285 and t.dsym < 30):
                    continue
                length = min(258, LEN_BASE[t.lsym - 257] + t.lextra)
                if length == 258:
                    self.enc258.add("285" if t.lsym == 285 else "284+31")
                d = DIST_BASE[t.dsym] + t.dextra
            else:
                length, d = t
                key = (length, long258)
                if length == 258:
                    self.enc258.add("284+31" if long258 else "285")
                ls = _LEN_SYM.get(key)
                if ls is None:
                    ls = _LEN_SYM[key] = length_symbol(length, long258)
                ds = _DIST_SYM.get(d)
                if ds is None:
                    ds = _DIST_SYM[d] = dist_symbol(d)
                c, l = lit[ls[0]]
                w.bits(c, l)
                w.bits(ls[2], ls[1])
                c, l = dist[ds[0]]
                w.bits(c, l)
                w.bits(ds[2], ds[1])
            p = len(out) - d
            if p >= 0 and d >= length:
                out += out[p:p + length]
            else:
                for _ in range(length):
                    out.append(out[p] if p >= 0 else 0x3F)
                    p += 1
        if eob:
            c, l = lit[256]
            w.bits(c, l)
