"""A writer of .xz files from the format's descriptions (xz-file-format-1.0.4, the LZMA specification), for the tests of the
block-parallel xz decode: the container (streams, block headers with and without the size fields, the three checks, index, footer,
padding) around LZMA2 payloads, and a small LZMA range ENCODER over an explicit packet list -- literal, match(distance, length),
rep0..3(length), short rep -- so the tests hold forms that liblzma's encoder never or rarely writes.  test_xz_twin.py proves that
liblzma decodes every stream written here to the intended bytes (test_writer_keeps_its_streams)."""
import lzma
import random
import struct
import zlib

MAGIC = b"\xfd7zXZ\x00"
CHECK_NONE, CHECK_CRC32, CHECK_CRC64, CHECK_SHA256 = 0, 1, 4, 10
CHECK_SIZE = {0: 0, 1: 4, 4: 8, 10: 32}

_CRC64 = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0xC96C5795D7870F42 if _c & 1 else _c >> 1
    _CRC64.append(_c)


def crc64(data):
    c = 0xFFFFFFFFFFFFFFFF
    for b in data:
        c = _CRC64[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFFFFFFFFFF


def crc32(data):
    return struct.pack("<I", zlib.crc32(data) & 0xFFFFFFFF)


def vli(v):
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def check_of(kind, data):
    if kind == CHECK_CRC32:
        return crc32(data)
    if kind == CHECK_CRC64:
        return struct.pack("<Q", crc64(data))
    if kind == CHECK_SHA256:
        import hashlib
        return hashlib.sha256(data).digest()
    return b""


def dict_byte(size):
    """the smallest dictionary size byte that holds `size`"""
    for b in range(41):
        if (2 | (b & 1)) << (b // 2 + 11) >= size:
            return b
    return 40


def block_header(dict_b=dict_byte(1 << 20), csize=None, usize=None, flags_extra=0, filters=None):
    body = bytearray([flags_extra | (0x40 if csize is not None else 0) | (0x80 if usize is not None else 0)])
    if csize is not None:
        body += vli(csize)
    if usize is not None:
        body += vli(usize)
    body += filters if filters is not None else vli(0x21) + vli(1) + bytes([dict_b])
    while (len(body) + 1) % 4:
        body.append(0)
    hdr = bytes([(len(body) + 1 + 4) // 4 - 1]) + bytes(body)
    return hdr + crc32(hdr)


def stream(blocks, check=CHECK_CRC32, sizes=True, dict_b=dict_byte(1 << 20)):
    """blocks: [(LZMA2 payload with its end byte, plain)]; the whole stream"""
    flags = bytes([0, check])
    out = bytearray(MAGIC + flags + crc32(flags))
    records = []
    for payload, plain in blocks:
        hdr = block_header(dict_b, len(payload) if sizes else None, len(plain) if sizes else None)
        unpadded = len(hdr) + len(payload) + CHECK_SIZE[check]
        out += hdr + payload + b"\0" * (-len(payload) % 4) + check_of(check, plain)
        records.append((unpadded, len(plain)))
    out += index_and_footer(records, flags)
    return bytes(out)


def index_and_footer(records, flags):
    idx = bytearray(b"\0" + vli(len(records)))
    for u, n in records:
        idx += vli(u) + vli(n)
    idx += b"\0" * (-len(idx) % 4)
    idx += crc32(bytes(idx))
    tail = struct.pack("<I", len(idx) // 4 - 1) + flags
    return bytes(idx) + crc32(tail) + tail + b"YZ"


def raw_payload(data, preset=6, dict_size=1 << 20, lc=3, lp=0, pb=2):
    """liblzma's own LZMA2 chunks for `data`, end byte included"""
    f = {"id": lzma.FILTER_LZMA2, "preset": preset, "dict_size": dict_size, "lc": lc, "lp": lp, "pb": pb}
    return lzma.compress(data, format=lzma.FORMAT_RAW, filters=[f])


def xz_of(data, block_bytes, check=CHECK_CRC32, sizes=True, **kw):
    """`data` cut into blocks of block_bytes, each compressed by liblzma, in one stream"""
    parts = [data[i:i + block_bytes] for i in range(0, len(data), block_bytes)]
    return stream([(raw_payload(p, **kw), p) for p in parts], check, sizes, dict_byte(kw.get("dict_size", 1 << 20)))


# ---- the range encoder and the LZMA packets ----
P_IS_MATCH, P_IS_REP, P_G0, P_G1, P_G2, P_REP0_LONG, P_POS_SLOT, P_SPEC_POS, P_ALIGN, P_LEN, P_REP_LEN, P_LITERAL = 0, 192, 204, 216, 228, 240, 432, 688, 802, 818, 1332, 1846


class Rc:
    def __init__(self):
        self.low, self.range, self.cache, self.cache_size, self.out = 0, 0xFFFFFFFF, 0, 1, bytearray()

    def shift_low(self):
        if self.low < 0xFF000000 or self.low >> 32:
            carry = self.low >> 32
            while True:
                self.out.append((self.cache + carry) & 0xFF)
                self.cache = 0xFF
                self.cache_size -= 1
                if not self.cache_size:
                    break
            self.cache = (self.low >> 24) & 0xFF
        self.cache_size += 1
        self.low = (self.low & 0x00FFFFFF) << 8

    def bit(self, probs, i, b):
        p = probs[i]
        bound = (self.range >> 11) * p
        if b:
            self.low += bound
            self.range -= bound
            probs[i] = p - (p >> 5)
        else:
            self.range = bound
            probs[i] = p + ((2048 - p) >> 5)
        while self.range < 1 << 24:
            self.range = (self.range << 8) & 0xFFFFFFFF
            self.shift_low()

    def direct(self, v, n):
        for i in range(n - 1, -1, -1):
            self.range >>= 1
            if (v >> i) & 1:
                self.low += self.range
            while self.range < 1 << 24:
                self.range = (self.range << 8) & 0xFFFFFFFF
                self.shift_low()

    def finish(self):
        for _ in range(5):
            self.shift_low()
        return bytes(self.out)


class Block:
    """the LZMA2 payload of one block, built chunk by chunk; .plain is what it decodes to"""

    def __init__(self):
        self.payload, self.plain, self.dict_at = bytearray(), bytearray(), 0
        self.lc = self.lp = self.pb = None
        self.probs, self.state, self.reps = None, 0, [0, 0, 0, 0]
        self.controls = []
        self.lenient = False                 # True: a distance beyond the bytes in front copies zeros (for streams a decoder must refuse)

    # -- packets
    def _tree(self, rc, base, bits, v):
        m = 1
        for i in range(bits - 1, -1, -1):
            b = (v >> i) & 1
            rc.bit(self.probs, base + m, b)
            m = m << 1 | b

    def _tree_rev(self, rc, base, bits, v):
        m = 1
        for i in range(bits):
            b = (v >> i) & 1
            rc.bit(self.probs, base + m, b)
            m = m << 1 | b

    def _len(self, rc, base, n, ps):
        n -= 2
        if n < 8:
            rc.bit(self.probs, base, 0)
            self._tree(rc, base + 2 + (ps << 3), 3, n)
        elif n < 16:
            rc.bit(self.probs, base, 1)
            rc.bit(self.probs, base + 1, 0)
            self._tree(rc, base + 130 + (ps << 3), 3, n - 8)
        else:
            rc.bit(self.probs, base, 1)
            rc.bit(self.probs, base + 1, 1)
            self._tree(rc, base + 258, 8, n - 16)

    def _copy(self, dist0, n):
        assert self.lenient or dist0 < len(self.plain) - self.dict_at, "a distance beyond the bytes since the dictionary reset"
        for _ in range(n):
            self.plain.append(self.plain[-1 - dist0] if dist0 < len(self.plain) else 0)

    def _packet(self, rc, p):
        dpos = len(self.plain) - self.dict_at
        ps = dpos & ((1 << self.pb) - 1)
        st, P = self.state, self.probs
        if p[0] == "lit":
            b = p[1]
            rc.bit(P, P_IS_MATCH + (st << 4) + ps, 0)
            prev = self.plain[-1] if dpos else 0
            pl = P_LITERAL + 0x300 * (((dpos & ((1 << self.lp) - 1)) << self.lc) + (prev >> (8 - self.lc)))
            sym = 1
            if st < 7:
                for i in range(7, -1, -1):
                    rc.bit(P, pl + sym, (b >> i) & 1)
                    sym = sym << 1 | (b >> i) & 1
            else:
                mb, offs = (self.plain[-1 - self.reps[0]] if self.reps[0] < len(self.plain) else 0), 0x100
                for i in range(7, -1, -1):
                    mb <<= 1
                    mbit, bit = mb & offs, (b >> i) & 1
                    rc.bit(P, pl + offs + mbit + sym, bit)
                    sym = sym << 1 | bit
                    offs &= mbit if bit else ~mbit
            self.state = 0 if st < 4 else st - 3 if st < 10 else st - 6
            self.plain.append(b)
            return
        rc.bit(P, P_IS_MATCH + (st << 4) + ps, 1)
        if p[0] == "match":
            dist0, n = p[1] - 1, p[2]
            rc.bit(P, P_IS_REP + st, 0)
            self._len(rc, P_LEN, n, ps)
            self.state = 7 if st < 7 else 10
            if dist0 < 4:
                slot = dist0
            else:
                k = dist0.bit_length() - 1
                slot = 2 * k + ((dist0 >> (k - 1)) & 1)
            self._tree(rc, P_POS_SLOT + (min(n - 2, 3) << 6), 6, slot)
            if slot >= 4:
                nb = (slot >> 1) - 1
                base = (2 | (slot & 1)) << nb
                if slot < 14:
                    self._tree_rev(rc, P_SPEC_POS + base - slot - 1, nb, dist0 - base)
                else:
                    rc.direct((dist0 - base) >> 4, nb - 4)
                    self._tree_rev(rc, P_ALIGN, 4, (dist0 - base) & 15)
            self.reps = [dist0] + self.reps[:3]
            if dist0 != 0xFFFFFFFF:
                self._copy(dist0, n)
            return
        rc.bit(P, P_IS_REP + st, 1)
        if p[0] == "srep":
            rc.bit(P, P_G0 + st, 0)
            rc.bit(P, P_REP0_LONG + (st << 4) + ps, 0)
            self.state = 9 if st < 7 else 11
            self._copy(self.reps[0], 1)
            return
        idx, n = p[1], p[2]
        if idx == 0:
            rc.bit(P, P_G0 + st, 0)
            rc.bit(P, P_REP0_LONG + (st << 4) + ps, 1)
        else:
            rc.bit(P, P_G0 + st, 1)
            rc.bit(P, P_G1 + st, 0 if idx == 1 else 1)
            if idx > 1:
                rc.bit(P, P_G2 + st, idx - 2)
            d = self.reps.pop(idx)
            self.reps.insert(0, d)
        self._len(rc, P_REP_LEN, n, ps)
        self.state = 8 if st < 7 else 11
        self._copy(self.reps[0], n)

    # -- chunks
    def lzma(self, packets, control, props=None, first_byte=0, usize_delta=0, extra=b""):
        """one LZMA chunk.  control: 0xE0 (dictionary reset, new properties, state reset), 0xC0 (new properties, state reset), 0xA0
        (state reset), 0x80.  props: (lc, lp, pb) for 0xC0 / 0xE0.  For streams a decoder must refuse: first_byte is XORed into the
        range coder's first byte, usize_delta added to the stated uncompressed size, extra appended to the compressed bytes"""
        if control >= 0xE0:
            self.dict_at = len(self.plain)
        if control >= 0xC0:
            self.lc, self.lp, self.pb = props
        if control >= 0xA0:
            self.probs, self.state, self.reps = [1024] * (1846 + (768 << (self.lc + self.lp))), 0, [0, 0, 0, 0]
        start = len(self.plain)
        rc = Rc()
        for p in packets:
            self._packet(rc, p)
        data = bytearray(rc.finish() + extra)
        data[0] ^= first_byte
        usize = len(self.plain) - start + usize_delta
        assert 1 <= usize <= 1 << 21 and 1 <= len(data) <= 1 << 16, (usize, len(data))
        self.payload += bytes([control | (usize - 1) >> 16]) + struct.pack(">HH", (usize - 1) & 0xFFFF, len(data) - 1)
        if control >= 0xC0:
            self.payload.append((self.pb * 5 + self.lp) * 9 + self.lc)
        self.payload += data
        self.controls.append(control)
        return self

    def raw(self, data, reset):
        """one uncompressed chunk: control 1 (dictionary reset) or 2"""
        assert 1 <= len(data) <= 1 << 16
        if reset:
            self.dict_at = len(self.plain)
        self.payload += bytes([1 if reset else 2]) + struct.pack(">H", len(data) - 1) + data
        self.plain += data
        self.controls.append(1 if reset else 2)
        return self

    def done(self):
        return bytes(self.payload) + b"\0", bytes(self.plain)


def lits(data):
    return [("lit", b) for b in data]


def _noise(n, seed):
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGTACGTNacgt\n@+IIIIFFF#") for _ in range(n))


def random_packets(rng, n, have, limit):
    """n packets that stay valid given `have` bytes since the dictionary reset and at most `limit` bytes of output"""
    out, made, reps = [], 0, 0
    for _ in range(n):
        room = limit - made
        if room < 300:
            break
        r = rng.random()
        if have + made == 0 or r < 0.35:
            out.append(("lit", rng.choice(b"ACGTN\n!I")))
            made += 1
            continue
        length = rng.choice((2, 3, 5, 9, 10, 17, 18, 19, 64, 65, 100, 272, 273)) if rng.random() < 0.5 else rng.randint(2, 273)
        if r < 0.7 or not reps:
            top = have + made
            d = rng.choice((1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 127, 128, 129, 3000, 3072, 3073, 4095, 4096, 4097, top))
            d = min(d, top) if rng.random() < 0.7 else rng.randint(1, top)
            out.append(("match", d, length))
            reps = min(4, reps + 1)
            made += length
        elif r < 0.8:
            out.append(("srep",))
            made += 1
        else:
            out.append(("rep", rng.randrange(reps), length))
            made += length
    return out


def _slots_block():
    """every distance-slot class behind a 0x01 chunk: slots 0-3, the reverse bit trees of slots 4-13, direct and align bits from 14"""
    b = Block().raw(_noise(60_000, 1), True)
    pk = []
    for d0 in list(range(0, 130)) + [191, 192, 255, 256, 1023, 1024, 4095, 4096, 8191, 16383, 16384, 32768, 49151, 59_999]:
        for n in (2, 3, 4, 5, 6):                       # (the slot's tree is chosen by the length: 2, 3, 4, 5 and above)
            pk.append(("match", d0 + 1, n))
        pk.append(("lit", 65 + d0 % 20))
    return b.lzma(pk, 0xC0, (3, 0, 2))


def _lengths_block():
    """lengths in the low, mid and high coder at every pos_state (pb = 4), by matches and by reps"""
    b = Block()
    pk = lits(_noise(40, 2))
    for n in list(range(2, 40)) + [127, 128, 129, 271, 272, 273]:
        for shift in range(16):
            pk += [("match", 7 + shift, n), ("lit", 71)] + [("lit", 84)] * (shift % 3)
            pk += [("rep", 0, n)]
    return b.lzma(pk, 0xE0, (0, 0, 4))


def _reps_block():
    """all four reps and the short rep in every state group, a matched literal after each kind of match"""
    b = Block()
    pk = lits(_noise(200, 3))
    kinds = [("match", 11, 4), ("match", 23, 5), ("match", 37, 6), ("match", 53, 7), ("rep", 3, 3), ("rep", 2, 4), ("rep", 1, 5), ("rep", 0, 6), ("srep",)]
    rng = random.Random(4)
    for a in kinds:                                      # every pair, with none, one and many literals between: every state is reached
        for c in kinds:
            for gap in (0, 1, 2, 5):
                pk += [("match", 11, 4), ("match", 23, 5), ("match", 37, 6), ("match", 53, 7)]
                pk += [a] + [("lit", rng.choice(b"ACGT"))] * gap + [c, ("lit", rng.choice(b"ACGT"))]
    return b.lzma(pk, 0xE0, (3, 0, 2))


def _controls_block():
    """0xA0 and 0xC0 mid-block with new lc / lp / pb, 0x02 followed by 0x80, 0x01 mid-block, a chunk of one byte"""
    rng = random.Random(5)
    b = Block()
    b.lzma(lits(_noise(300, 6)) + random_packets(rng, 200, 300, 20_000), 0xE0, (3, 0, 2))
    b.lzma(random_packets(rng, 200, len(b.plain), 20_000), 0x80)
    b.lzma(random_packets(rng, 200, len(b.plain), 20_000), 0xA0)
    b.lzma(random_packets(rng, 200, len(b.plain), 20_000), 0xC0, (0, 4, 4))
    b.raw(_noise(5000, 7), False)
    b.lzma(random_packets(rng, 200, len(b.plain), 20_000), 0x80)
    b.lzma([("lit", 90)], 0x80)
    b.lzma(random_packets(rng, 200, len(b.plain), 20_000), 0xC0, (2, 2, 0))
    b.raw(_noise(3000, 8), True)
    b.lzma(random_packets(rng, 300, 3000, 30_000), 0xC0, (4, 0, 1))
    b.raw(b"Z", False)
    b.lzma(random_packets(rng, 100, len(b.plain) - b.dict_at, 20_000), 0xA0)
    b.lzma(random_packets(rng, 300, 0, 30_000), 0xE0, (1, 3, 3))
    return b


def _random_block(seed, props, packets=1500):
    rng = random.Random(seed)
    b = Block()
    b.lzma(random_packets(rng, packets, 0, 400_000), 0xE0, props)
    b.lzma(random_packets(rng, packets, len(b.plain), 400_000), 0x80)
    return b


def _two_mib_block():
    """a chunk of exactly 2 MiB uncompressed: one literal line, then long reps"""
    pk = lits(b"ACGTTGCAAC\n") + [("match", 11, 273)]
    made = 11 + 273
    while (1 << 21) - made >= 273:
        pk.append(("rep", 0, 273))
        made += 273
    rest = (1 << 21) - made
    if rest == 1:
        pk.append(("srep",))
    elif rest:
        pk.append(("rep", 0, rest))
    b = Block().lzma(pk, 0xE0, (3, 0, 2))
    assert len(b.plain) == 1 << 21
    return b.lzma(lits(b"tail\n"), 0x80)


_CASES = None


def cases(big=True):
    """(name, xz bytes, plain)"""
    global _CASES
    if _CASES is None:
        out = []
        blocks = {"slot_classes": _slots_block(), "lengths_every_pos_state": _lengths_block(), "reps_every_state": _reps_block(),
                  "controls_mid_block": _controls_block(), "random_lc0_lp0_pb0": _random_block(10, (0, 0, 0)), "random_lc4_lp0_pb2": _random_block(11, (4, 0, 2)),
                  "random_lc0_lp4_pb4": _random_block(12, (0, 4, 4)), "random_lc2_lp2_pb0": _random_block(13, (2, 2, 0))}
        done = {k: v.done() for k, v in blocks.items()}
        for i, (name, (payload, plain)) in enumerate(done.items()):
            out.append((name, stream([(payload, plain)], (CHECK_CRC32, CHECK_CRC64, CHECK_NONE)[i % 3], sizes=bool(i % 2), dict_b=dict_byte(1 << 20)), plain))
        # the container: three blocks of liblzma's own, every check, with and without the size fields; empty streams; padding
        text = _noise(30_000, 20)
        for check, nm in ((CHECK_NONE, "none"), (CHECK_CRC32, "crc32"), (CHECK_CRC64, "crc64")):
            for sizes in (True, False):
                out.append(("three_blocks_%s_%s" % (nm, "sizes" if sizes else "nosizes"), xz_of(text, 10_000, check, sizes), text))
        all_blocks = stream(list(done.values()), CHECK_CRC64)
        out.append(("all_writer_blocks_one_stream", all_blocks, b"".join(p for _, p in done.values())))
        empty = stream([], CHECK_CRC32)
        a, bb = xz_of(text[:7000], 4000, CHECK_CRC32), xz_of(text[7000:9000], 1500, CHECK_CRC64, sizes=False)
        out.append(("empty_stream_between", a + empty + bb, text[:9000]))
        out.append(("streams_with_padding", a + b"\0" * 4 + bb + b"\0" * 12 + empty + b"\0" * 8, text[:9000]))
        _CASES = out
    if big:
        return _CASES + [("chunk_of_2_mib", stream([_big()], CHECK_CRC32), _big()[1])]
    return _CASES


_BIG = None


def _big():
    global _BIG
    if _BIG is None:
        _BIG = _two_mib_block().done()
    return _BIG


def by_name(name):
    return next(c for c in cases() if c[0] == name)
