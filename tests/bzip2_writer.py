"""A small bzip2 writer, written from the format's description, for the legal forms libbz2's encoder never writes: 2 and 6 coding
tables on tiny blocks, tables no selector uses, code lengths of 20, a count byte of 0 behind a run of 4, origPtr 0 and n - 1, blocks of one symbol.  The BWT is a naive sort of the rotations: blocks of a few
hundred bytes.  cases() keeps the streams that bz2.decompress accepts and counts the others (dropped())."""
import bz2

BLOCK_MAGIC, END_MAGIC = 0x314159265359, 0x177245385090


def _crc_table():
    t = []
    for i in range(256):
        c = i << 24
        for _ in range(8):
            c = ((c << 1) ^ 0x04c11db7) & 0xFFFFFFFF if c & 0x80000000 else (c << 1) & 0xFFFFFFFF
        t.append(c)
    return t


_CRC = _crc_table()


def crc(data):
    c = 0xFFFFFFFF
    for b in data:
        c = ((c << 8) & 0xFFFFFFFF) ^ _CRC[(c >> 24) ^ b]
    return c ^ 0xFFFFFFFF


class Bits:
    """MSB first"""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, k):
        assert 0 <= value < (1 << k)
        self.v = (self.v << k) | value
        self.n += k

    def bytes(self):
        pad = -self.n % 8
        return ((self.v << pad).to_bytes((self.n + pad) // 8, "big")) if self.n else b""


def rle1(data):
    """runs of 4 to 259 equal bytes as four bytes and a count"""
    out, i = bytearray(), 0
    while i < len(data):
        j = i
        while j < len(data) and data[j] == data[i] and j - i < 259:
            j += 1
        k = j - i
        out += data[i:i + min(k, 4)]
        if k >= 4:
            out.append(k - 4)
        i = j
    return bytes(out)


def bwt(block):
    n = len(block)
    order = sorted(range(n), key=lambda i: block[i:] + block[:i])
    return bytes(block[(i - 1) % n] for i in order), order.index(0)


def mtf_rle2(column):
    """(symbols with the end-of-block symbol, the byte values in use)"""
    used = sorted(set(column))
    lst = list(range(len(used)))
    where = {b: i for i, b in enumerate(used)}
    syms, run = [], 0

    def flush():
        nonlocal run
        while run > 0:
            run -= 1
            syms.append(run & 1)
            run >>= 1
    for b in column:
        at = lst.index(where[b])
        if at == 0:
            run += 1
            continue
        flush()
        lst.insert(0, lst.pop(at))
        syms.append(at + 1)
    flush()
    syms.append(len(used) + 1)
    return syms, used


def lengths(alpha, shape):
    if shape == "flat":
        return [max(1, (alpha - 1).bit_length())] * alpha
    if shape == "deep":                       # one short code, every other code 20 bits long (an incomplete code)
        return [1] + [20] * (alpha - 1)
    if shape == "skew":                       # 1, 2, 3, ... up to the two longest
        assert alpha <= 21
        return [min(i + 1, alpha - 1) for i in range(alpha)]
    raise ValueError(shape)


def codes(lens):
    """canonical: by length, then by symbol"""
    out, code = {}, 0
    for k in range(min(lens), max(lens) + 1):
        for s, l in enumerate(lens):
            if l == k:
                out[s] = (code, k)
                code += 1
        code <<= 1
    return out


def block(bits, pre, plain, groups=2, shapes=("flat",), select="rotate", orig=None):
    """one block: `pre` are its bytes behind the run-length layer, `plain` the text they stand for"""
    column, o = bwt(pre)
    syms, used = mtf_rle2(column)
    alpha = len(used) + 2
    bits.put(BLOCK_MAGIC, 48)
    bits.put(crc(plain), 32)
    bits.put(0, 1)
    bits.put(o if orig is None else orig, 24)
    ranges = [any(16 * r <= b < 16 * r + 16 for b in used) for r in range(16)]
    bits.put(sum(1 << (15 - r) for r in range(16) if ranges[r]), 16)
    for r in range(16):
        if ranges[r]:
            bits.put(sum(1 << (15 - j) for j in range(16) if 16 * r + j in used), 16)
    tabs = [lengths(alpha, shapes[g % len(shapes)]) for g in range(groups)]
    n_sel = (len(syms) + 49) // 50
    sel = [(i % groups) if select == "rotate" else 0 for i in range(n_sel)]
    bits.put(groups, 3)
    bits.put(n_sel, 15)
    order = list(range(groups))
    for g in sel:
        at = order.index(g)
        bits.put((1 << (at + 1)) - 2, at + 1)
        order.insert(0, order.pop(at))
    for t in tabs:
        cur = t[0]
        bits.put(cur, 5)
        for want in t:
            while cur != want:
                bits.put(2 if want > cur else 3, 2)
                cur += 1 if want > cur else -1
            bits.put(0, 1)
    cs = [codes(t) for t in tabs]
    for i, s in enumerate(syms):
        c, k = cs[sel[i // 50]][s]
        bits.put(c, k)


def stream(plain, level=1, size=300, raw_blocks=None, **kw):
    """`plain` in blocks of `size` bytes of text; raw_blocks: [(pre, plain)] instead"""
    bits = Bits()
    for ch in b"BZh":
        bits.put(ch, 8)
    bits.put(48 + level, 8)
    parts = raw_blocks if raw_blocks is not None else [(rle1(plain[i:i + size]), plain[i:i + size]) for i in range(0, len(plain), size)]
    combined = 0
    for pre, text in parts:
        block(bits, pre, text, **kw)
        combined = (((combined << 1) | (combined >> 31)) & 0xFFFFFFFF) ^ crc(text)
    bits.put(END_MAGIC, 48)
    bits.put(combined, 32)
    return bits.bytes()


def stops_behind_four_equal():
    """a block whose bytes stop where a run's count byte belongs: libbz2 gives an error"""
    return stream(b"", raw_blocks=[(b"xyAAAA", b"xyAAAA")])


def _text(n, seed):
    import random
    rng = random.Random(seed)
    return b"".join(rng.choice([b"ACGT", b"GATTACA", b"N", b"AAAA", b"CCCCC", b"\n@r\n", b"TTTTTTTT"]) for _ in range(n))


def _all():
    t = _text(220, 1)
    nineteen = bytes(range(65, 84)) * 3                                   # 19 byte values: an alphabet of 21 symbols
    out = [
        ("groups2_flat", t, stream(t, groups=2)),
        ("groups6_flat", t, stream(t, groups=6)),
        ("groups6_unused_tables", t, stream(t, groups=6, select="first")),
        ("groups3_mixed_shapes", t, stream(t, groups=3, shapes=("flat", "deep", "flat"))),
        ("lengths_of_20", t, stream(t, groups=2, shapes=("deep",))),
        ("skew_1_to_20", nineteen, stream(nineteen, groups=2, shapes=("skew",))),
        ("tiny_blocks", t, stream(t, size=7, groups=2)),
        ("count_zero_after_4", b"xAAAAyBBBBz", stream(b"xAAAAyBBBBz")),
        ("orig_ptr_0", b"abcdefgh", stream(b"abcdefgh")),
        ("orig_ptr_last", b"hgfedcba", stream(b"hgfedcba")),
        ("one_symbol_blocks", b"qrs", stream(b"qrs", size=1)),
        ("one_byte_value_run", b"G" * 600, stream(b"G" * 600, size=259)),
        ("level9_header", t, stream(t, level=9, groups=4)),
        ("all_bytes", bytes(range(256)), stream(bytes(range(256)), size=256, groups=6)),
    ]
    return out


_KEPT = None
_DROPPED = None


def _split():
    global _KEPT, _DROPPED
    if _KEPT is None:
        _KEPT, _DROPPED = [], []
        for name, plain, comp in _all():
            try:
                ok = bz2.decompress(comp) == plain
            except Exception:
                ok = False
            (_KEPT if ok else _DROPPED).append((name, comp, plain))
    return _KEPT, _DROPPED


def cases():
    """(name, bzip2 bytes, plain bytes) of the streams libbz2 accepts"""
    return _split()[0]


def dropped():
    """names of the streams libbz2 does not accept"""
    return [c[0] for c in _split()[1]]
