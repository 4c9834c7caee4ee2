"""A small Zstandard writer, written from the format's description (RFC 8878), for the legal forms libzstd's encoder does not
write on the corpus: RLE literals, Huffman descriptions with direct weights, RLE mode for each of the three sequence tables,
repeat modes behind predefined and RLE tables, every repeat-offset case, Number_of_Sequences at the edges of its three
encodings, short offsets with lengths around the 64-byte steps of the device's copy, the largest length codes, treeless literals
two blocks behind their table, frames without content size, an empty frame, skippable frames.  The writer executes its own
sequences to know the text it intends.  cases() keeps the streams that libzstd decodes to that text and counts the others
(dropped())."""
import struct

import zstd_corpus as Z

P1, P2, P3, P4, P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5
M = (1 << 64) - 1


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M


def _round(acc, w):
    return (_rotl((acc + w * P2) & M, 31) * P1) & M


def xxh64(data):
    n, i = len(data), 0
    if n >= 32:
        v = [(P1 + P2) & M, P2, 0, (-P1) & M]
        while i + 32 <= n:
            for k, w in enumerate(struct.unpack_from("<4Q", data, i)):
                v[k] = _round(v[k], w)
            i += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M
        for x in v:
            h = ((h ^ _round(0, x)) * P1 + P4) & M
    else:
        h = P5
    h = (h + n) & M
    while i + 8 <= n:
        h = (_rotl(h ^ _round(0, struct.unpack_from("<Q", data, i)[0]), 27) * P1 + P4) & M
        i += 8
    if i + 4 <= n:
        h = (_rotl(h ^ (struct.unpack_from("<I", data, i)[0] * P1 & M), 23) * P2 + P3) & M
        i += 4
    while i < n:
        h = (_rotl(h ^ (data[i] * P5 & M), 11) * P1) & M
        i += 1
    h ^= h >> 33
    h = h * P2 & M
    h ^= h >> 29
    h = h * P3 & M
    return h ^ (h >> 32)


def backward(fields):
    """fields [(value, bits)] in the order the decoder reads them -> the bytes of a backward bitstream with its end mark"""
    acc = n = 0
    for v, b in reversed(fields):
        assert 0 <= v < (1 << b) or (b == 0 and v == 0), (v, b)
        acc |= v << n
        n += b
    acc |= 1 << n
    return acc.to_bytes(n // 8 + 1, "little")


# ---- FSE decode tables (the decoder's construction; the writer walks them backwards to encode) ----
LL_NORM = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_NORM = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_NORM = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def fse_table(norm, log):
    """[(symbol, bits, base)] per state"""
    size = 1 << log
    sym = [None] * size
    high = size
    nxt = {}
    for s, p in enumerate(norm):
        if p == -1:
            high -= 1
            sym[high] = s
            nxt[s] = 1
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, p in enumerate(norm):
        if p <= 0:
            continue
        nxt[s] = p
        for _ in range(p):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos >= high:
                pos = (pos + step) & (size - 1)
    assert pos == 0
    tab = []
    for i in range(size):
        d = nxt[sym[i]]
        nxt[sym[i]] += 1
        nb = log - (d.bit_length() - 1)
        tab.append((sym[i], nb, (d << nb) - size))
    return tab


PREDEFINED = {"ll": (fse_table(LL_NORM, 6), 6), "of": (fse_table(OF_NORM, 5), 5), "ml": (fse_table(ML_NORM, 6), 6)}


def fse_states(tab, codes):
    """the states a decoder of `tab` passes through while it emits `codes`"""
    states = [None] * len(codes)
    states[-1] = next(i for i, e in enumerate(tab) if e[0] == codes[-1])
    for i in range(len(codes) - 2, -1, -1):
        states[i] = next(j for j, (s, nb, base) in enumerate(tab) if s == codes[i] and base <= states[i + 1] < base + (1 << nb))
    return states


def code_of(value, base):
    return max(c for c, b in enumerate(base) if b <= value)


# ---- literals ----
def lit_header(typ, regen, comp=None, streams=1):
    if typ < 2:
        if regen < 32:
            return bytes([typ | regen << 3])
        if regen < 4096:
            return struct.pack("<H", typ | 1 << 2 | regen << 4)
        return (typ | 3 << 2 | regen << 4).to_bytes(3, "little")
    if streams == 1:
        assert regen < 1024 and comp < 1024
        return (typ | regen << 4 | comp << 14).to_bytes(3, "little")
    if regen < 1024 and comp < 1024:
        return (typ | 1 << 2 | regen << 4 | comp << 14).to_bytes(3, "little")
    if regen < 16384 and comp < 16384:
        return (typ | 2 << 2 | regen << 4 | comp << 18).to_bytes(4, "little")
    return (typ | 3 << 2 | regen << 4 | comp << 22).to_bytes(5, "little")


class Huffman:
    """weights {symbol: weight}; the symbol of the largest value carries the implied weight"""

    def __init__(self, weights):
        self.w = dict(weights)
        total = sum(1 << (w - 1) for w in self.w.values())
        self.log = total.bit_length() - 1
        assert total == 1 << self.log
        at, self.code = 0, {}
        for w in range(1, self.log + 1):
            for s in sorted(self.w):
                if self.w[s] == w:
                    self.code[s] = (at >> (w - 1), self.log + 1 - w)
                    at += 1 << (w - 1)

    def description(self):
        top = max(self.w)
        ws = [self.w.get(s, 0) for s in range(top)]
        assert 1 <= len(ws) <= 128
        out = bytearray([127 + len(ws)])
        for i in range(0, len(ws), 2):
            out.append(ws[i] << 4 | (ws[i + 1] if i + 1 < len(ws) else 0))
        return bytes(out)

    def stream(self, data):
        return backward([self.code[b] for b in data])


def literals(kind, data, huf=None, streams=1):
    """kind: raw, rle, huffman (with its description), treeless"""
    if kind == "raw":
        return lit_header(0, len(data)) + data
    if kind == "rle":
        assert len(set(data)) == 1
        return lit_header(1, len(data)) + data[:1]
    body = huf.description() if kind == "huffman" else b""
    if streams == 1:
        body += huf.stream(data)
    else:
        seg = (len(data) + 3) // 4
        parts = [huf.stream(data[i * seg:(i + 1) * seg]) for i in range(4)]
        body += struct.pack("<3H", *(len(p) for p in parts[:3])) + b"".join(parts)
    return lit_header(2 if kind == "huffman" else 3, len(data), len(body), streams) + body


# ---- a frame under construction ----
class Frame:
    def __init__(self, window_log=None, content_size=True, checksum=True):
        self.window_log, self.content_size, self.checksum = window_log, content_size, checksum
        self.blocks, self.text, self.rep = [], bytearray(), [1, 4, 8]
        self.prev = {}                      # table name -> (table, log): what a repeat mode would use

    def raw(self, data):
        self.blocks.append((0, len(data), data))
        self.text += data

    def rle(self, byte, n):
        self.blocks.append((1, n, bytes([byte])))
        self.text += bytes([byte]) * n

    def body(self, data):
        """a compressed block of these bytes, whatever they mean (for streams that are to be refused)"""
        self.blocks.append((2, len(data), bytes(data)))

    def compressed(self, lit_bytes, lit_data, seqs=(), modes=("predefined", "predefined", "predefined"), nseq_form=None, lenient=False):
        """lit_bytes: the literals section; lit_data: what it regenerates; seqs: [(ll, ml, offset_value)]; lenient: the sequences
        need not make sense (for streams that are to be refused: the text is then not the frame's)"""
        body = bytearray(lit_bytes)
        n = len(seqs)
        if nseq_form == 3 or n >= 0x7F00:
            body += bytes([255]) + struct.pack("<H", n - 0x7F00)
        elif n >= 128:
            body += bytes([128 + (n >> 8), n & 255])
        else:
            body += bytes([n])
        if n:
            codes = {"ll": [code_of(s[0], LL_BASE) for s in seqs], "ml": [code_of(s[1], ML_BASE) for s in seqs], "of": [s[2].bit_length() - 1 for s in seqs]}
            mode_byte, extra, tabs = 0, b"", {}
            for name, mode, shift in (("ll", modes[0], 6), ("of", modes[1], 4), ("ml", modes[2], 2)):
                if mode == "predefined":
                    tabs[name] = PREDEFINED[name]
                elif mode == "rle":
                    assert len(set(codes[name])) == 1
                    tabs[name] = ([(codes[name][0], 0, 0)], 0)
                    extra += bytes([codes[name][0]])
                    mode_byte |= 1 << shift
                else:
                    assert mode == "repeat"
                    tabs[name] = self.prev[name]
                    mode_byte |= 3 << shift
            body += bytes([mode_byte]) + extra
            st = {name: fse_states(tabs[name][0], codes[name]) for name in tabs}
            fields = [(st[name][0], tabs[name][1]) for name in ("ll", "of", "ml")]
            for i, (ll, ml, ofv) in enumerate(seqs):
                cl, cm, co = codes["ll"][i], codes["ml"][i], codes["of"][i]
                fields += [(ofv - (1 << co), co), (ml - ML_BASE[cm], ML_BITS[cm]), (ll - LL_BASE[cl], LL_BITS[cl])]
                if i + 1 < n:
                    for name in ("ll", "ml", "of"):
                        _, nb, base = tabs[name][0][st[name][i]]
                        fields.append((st[name][i + 1] - base, nb))
            body += backward(fields)
            self.prev.update(tabs)
        self.blocks.append((2, len(body), bytes(body)))
        # the text the sequences mean
        lp = 0
        for ll, ml, ofv in seqs:
            self.text += lit_data[lp:lp + ll]
            lp += ll
            r = self.rep
            if ofv > 3:
                off = ofv - 3
                self.rep = [off, r[0], r[1]]
            else:
                idx = ofv - (1 if ll else 0)
                if idx == 0:
                    off = r[0]
                else:
                    off = r[0] - 1 if idx == 3 else r[idx]
                    self.rep = [off, r[0], r[1]] if idx != 1 else [off, r[0], r[2]]
            assert lenient or 0 < off <= len(self.text), (off, len(self.text))
            for _ in range(ml if 0 < off <= len(self.text) else 0):
                self.text.append(self.text[-off])
        self.text += lit_data[lp:]

    def bytes(self):
        n = len(self.text)
        fhd = 4 if self.checksum else 0
        out = bytearray(Z.MAGIC)
        if self.window_log is None:               # single segment: the content size is the window
            assert self.content_size
            flag, field = (0, bytes([n])) if n < 256 else (1, struct.pack("<H", n - 256)) if n < 65536 + 256 else (2, struct.pack("<I", n))
            out += bytes([fhd | 0x20 | flag << 6]) + field
        else:
            field = struct.pack("<I", n) if self.content_size else b""
            out += bytes([fhd | (0x80 if self.content_size else 0), (self.window_log - 10) << 3]) + field
        if not self.blocks:
            self.blocks.append((0, 0, b""))
        for i, (typ, size, body) in enumerate(self.blocks):
            out += (int(i + 1 == len(self.blocks)) | typ << 1 | size << 3).to_bytes(3, "little") + body
        if self.checksum:
            out += struct.pack("<I", xxh64(bytes(self.text)) & 0xFFFFFFFF)
        return bytes(out)


DNA = Huffman({65: 2, 67: 2, 71: 2, 10: 1, 84: 1})                  # A, C, G two bits; line feed, T three


def _dna(n, seed):
    x, out = seed * 2654435761 % (1 << 32) or 1, bytearray()
    for i in range(n):
        x = (x * 1103515245 + 12345) % (1 << 31)
        out.append(10 if i % 61 == 60 else b"ACGT"[(x >> 16) & 3])
    return bytes(out)


def _all():
    out = []

    def add(name, *frames, around=(b"", b"", b"")):
        """frames back to back, with `around` = bytes before, between and behind them"""
        data = around[0] + around[1].join(f.bytes() for f in frames) + around[2]
        out.append((name, data, b"".join(bytes(f.text) for f in frames)))

    f = Frame()
    f.compressed(literals("rle", b"A" * 50), b"A" * 50)
    add("rle_literals", f)
    f = Frame()
    f.compressed(literals("rle", b"N" * 5000), b"N" * 5000, [(100, 40, 7), (4000, 10, 1)])
    add("rle_literals_long_with_sequences", f)
    d = _dna(900, 1)
    f = Frame()
    f.compressed(literals("huffman", d, DNA), d)
    add("direct_weights_1_stream", f)
    d = _dna(30000, 2)
    f = Frame()
    f.compressed(literals("huffman", d, DNA, 4), d, [(1000, 200, 500 + 3), (29000, 70, 2)])
    add("direct_weights_4_streams", f)
    # RLE mode per table: every sequence has that table's one code
    d = _dna(600, 3)
    for which, seqs in ((0, [(5, 10, 8), (5, 40, 20), (5, 3, 1)]), (1, [(25, 10, 16 + 3), (0, 40, 20 + 3), (9, 3, 17 + 3)]), (2, [(5, 7, 8), (0, 7, 12), (50, 7, 1)])):
        f = Frame()
        modes = ["predefined"] * 3
        modes[which] = "rle"
        f.compressed(literals("raw", d), d, seqs, modes)
        add("rle_mode_" + "ll of ml".split()[which], f)
    # the six repeat-offset cases, and r1 - 1 twice in a row
    f = Frame()
    f.compressed(literals("raw", d), d, [(20, 5, 10 + 3), (3, 4, 15 + 3), (2, 6, 7 + 3), (4, 5, 1), (4, 5, 2), (4, 5, 3), (0, 5, 1), (0, 5, 2), (0, 5, 3), (7, 9, 3)])
    add("repeat_offsets_all_six", f)
    f = Frame()
    f.compressed(literals("raw", d), d, [(30, 5, 9 + 3), (0, 4, 3), (0, 4, 3), (0, 4, 3), (2, 4, 1)])
    add("r1_minus_1_in_a_row", f)
    # Number_of_Sequences at the edges of its encodings
    for n in (127, 128):
        f = Frame()
        f.compressed(literals("raw", d), d, [(3, 3, 5)] + [(1, 3, 1)] * (n - 1))
        add("nseq_%d" % n, f)
    f = Frame(window_log=17)
    f.raw(b"xyz")
    f.compressed(literals("raw", b""), b"", [(0, 3, 3 + 3)] + [(0, 3, 1)] * (0x7F00 + 5 - 1), ("rle", "predefined", "rle"))
    add("nseq_three_bytes", f)
    f = Frame()
    f.compressed(literals("raw", d), d, [(2, 3, 4)] * 20, nseq_form=None)
    add("nseq_20", f)
    # short offsets, lengths around one and two steps of 64
    seqs = []
    for off in (1, 2, 3, 63, 64, 65):
        for ml in (63, 64, 65, 127, 128, 129):
            seqs.append((1, ml, off + 3))
    d = _dna(300, 4)
    f = Frame(window_log=17)
    f.compressed(literals("raw", d), d, [(100, 3, 50 + 3)] + seqs)
    add("short_offsets_step_edges", f)
    # the same matches reaching over the front of their block (deferred sources), behind a raw and an RLE block
    f = Frame(window_log=17)
    f.raw(_dna(70, 5))
    f.rle(ord("G"), 3)
    f.compressed(literals("raw", d), d, [(0, 130, off + 3) for off in (1, 2, 3, 63, 64, 65, 73)] + [(5, 200, 40 + 3)])
    f.compressed(literals("raw", d), d, [(0, 300, 900 + 3), (1, 64, 65 + 3), (0, 64, 1), (2, 700, 2 + 3)])
    add("matches_over_block_fronts", f)
    # the largest length codes
    big = _dna(65536 + 40, 6)
    f = Frame(window_log=18)
    f.compressed(literals("raw", big), big, [(65536 + 17, 3, 9 + 3)])
    f.compressed(literals("raw", b"ACGT"), b"ACGT", [(1, 65539 + 100, 60000 + 3)])
    add("largest_length_codes", f)
    # repeat modes behind predefined and behind RLE tables
    d = _dna(400, 7)
    f = Frame()
    f.compressed(literals("raw", d), d, [(10, 4, 12), (3, 9, 1)])
    f.compressed(literals("raw", d), d, [(40, 4, 300 + 3), (3, 9, 2), (0, 5, 3)], ("repeat", "repeat", "repeat"))
    add("repeat_mode_after_predefined", f)
    f = Frame()
    f.raw(_dna(100, 17))
    f.compressed(literals("raw", d), d, [(5, 7, 16 + 3), (5, 7, 17 + 3)], ("rle", "rle", "rle"))
    f.compressed(literals("raw", d), d, [(5, 7, 30), (5, 7, 31), (5, 7, 18)], ("repeat", "repeat", "repeat"))
    f.compressed(literals("raw", d), d, [(0, 3, 24)], ("predefined", "repeat", "predefined"))
    add("repeat_mode_after_rle", f)
    # a block without sequences between does not touch the tables
    f = Frame()
    f.compressed(literals("raw", d), d, [(20, 7, 16 + 3)], ("predefined", "rle", "predefined"))
    f.compressed(literals("raw", d[:50]), d[:50])
    f.compressed(literals("raw", d), d, [(5, 7, 20 + 3), (1, 3, 17 + 3)], ("repeat", "repeat", "repeat"))
    add("repeat_mode_over_a_block_without_sequences", f)
    # treeless literals two blocks behind their table, a raw block between
    d1, d2 = _dna(2000, 8), _dna(5000, 9)
    f = Frame()
    f.compressed(literals("huffman", d1, DNA, 4), d1, [(100, 30, 64 + 3)])
    f.raw(b"@read\n")
    f.compressed(literals("treeless", d2, DNA, 4), d2, [(10, 30, 2000 + 3), (0, 12, 3)])
    f.compressed(literals("treeless", d1[:700], DNA, 1), d1[:700])
    add("treeless_two_blocks_behind", f)
    # frames
    f = Frame(window_log=10, content_size=False)
    f.raw(_dna(500, 10))
    f.compressed(literals("raw", d), d, [(7, 100, 480 + 3)])
    add("no_content_size", f)
    add("no_content_size_no_checksum", _frame_plain(_dna(300, 11), window_log=12, content_size=False, checksum=False))
    add("empty_frame", Frame())
    add("empty_frame_between", _frame_plain(_dna(100, 12)), Frame(checksum=False), _frame_plain(_dna(90, 13)))
    add("skippable_before_between_behind", _frame_plain(_dna(200, 14)), _frame_plain(_dna(100, 15), checksum=False),
        around=(Z.skippable(b"head", 0), Z.skippable(b"", 7), Z.skippable(b"t" * 70, 15)))
    add("rle_block_then_match_into_it", _rle_then_match())
    return out


def _frame_plain(data, **kw):
    f = Frame(**kw)
    f.raw(data)
    return f


def _rle_then_match():
    f = Frame(window_log=17)
    f.rle(ord("T"), 1000)
    f.compressed(literals("raw", b"AC"), b"AC", [(2, 500, 700 + 3), (0, 100, 1 + 3)])
    return f


_KEPT = None
_DROPPED = None


def _split():
    global _KEPT, _DROPPED
    if _KEPT is None:
        _KEPT, _DROPPED = [], []
        for name, data, plain in _all():
            (_KEPT if Z.decompress(data) == plain else _DROPPED).append((name, data, plain))
    return _KEPT, _DROPPED


def cases():
    """(name, zstd bytes, plain bytes) of the streams libzstd decodes to the text the writer intended"""
    return _split()[0]


def dropped():
    """names of the streams libzstd does not decode to that text"""
    return [c[0] for c in _split()[1]]
