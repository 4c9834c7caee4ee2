"""Plain numpy models of the primitives in lrge_amd/csrc/k_prims.h -- the exclusive scan, the stable LSD radix sorts, the unpack of
packed anchors, the slot gather, the segment-packed index sort, the run heads, hash_to_sig / sig_to_hash -- and the case families that
tests/test_gpu_prims.py runs on the device.  The models know nothing of tiles, wavefronts or LDS.  Every model takes the name of a NEAR MISS (a plausible wrong
kernel); tests/test_prims_ref.py proves on the CPU that each family holds a case on which the near miss and the truth differ, so that
the device comparison could tell them apart.  No wrong kernel ever runs on a GPU."""
import numpy as np

U64 = np.uint64
M64 = (1 << 64) - 1
SCAN_TILE = 4096          # items per block of the device scan
SCAN_GROUP = 8192         # block sums one second-level pass covers
RS_TILE = 4096            # items per tile of the device sorts
LSORT_CAP = (2048, 8192, 16384)     # capacity of the three LDS sort variants


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def mask(bits):
    return (1 << bits) - 1 if bits < 64 else M64


def shr(a, s):
    return a >> U64(s) if s < 64 else np.zeros_like(a)


def shl(a, s):
    return a << U64(s) if s < 64 else np.zeros_like(a)


# ------------------------------------------------------------------------------------------
# scan
# ------------------------------------------------------------------------------------------
SCAN_MISSES = ("inclusive", "no_tile_carry", "no_group_carry")


def scan_exclusive(a, miss=None):
    """(out, total) of the exclusive scan of u32 items; the total must stay below 2^32"""
    a = np.asarray(a, dtype=np.uint32)
    n = a.size
    if n == 0:
        return np.zeros(0, dtype=np.uint32), 0
    c = np.cumsum(a.astype(np.uint64))
    total = int(c[-1])
    assert total < 1 << 32
    if miss == "inclusive":
        return c.astype(np.uint32), total
    out = np.concatenate([np.zeros(1, dtype=np.uint64), c[:-1]])
    if miss in ("no_tile_carry", "no_group_carry"):
        step = SCAN_TILE if miss == "no_tile_carry" else SCAN_TILE * SCAN_GROUP
        for s in range(step, n, step):                  # what came before the item's tile / group is forgotten
            out[s:s + step] -= out[s]
    return out.astype(np.uint32), total


# ------------------------------------------------------------------------------------------
# sorts: a permutation of the input positions
# ------------------------------------------------------------------------------------------
def n_passes(nbits):
    return (nbits + 7) // 8


def digit(keys, begin_bit, nbits, d, whole_bytes):
    """digit d (8 bits, the last one what is left of nbits -- or whole when the sort rounds up to bytes)"""
    w = 8 if whole_bytes else min(8, nbits - 8 * d)
    return shr(keys, begin_bit + 8 * d) & U64(mask(w))


def composed_key(keys, begin_bit, nbits, reverse_digits, whole_bytes):
    """what a whole sort orders by: the bits [begin_bit, begin_bit + nbits) (rounded up to bytes for the pair sort), the byte string reversed
    when reverse_digits"""
    p = n_passes(nbits)
    if not reverse_digits:
        return shr(keys, begin_bit) & U64(mask(min(64, 8 * p) if whole_bytes else nbits))
    f = np.zeros(keys.size, dtype=np.uint64)
    for d in range(p):
        w = 8 if whole_bytes else min(8, nbits - 8 * d)
        f = shl(f, w) | digit(keys, begin_bit, nbits, d, whole_bytes)
    return f


def stable_order(k, unstable=False):
    if not unstable:
        return np.argsort(k, kind="stable")
    return np.lexsort((-np.arange(k.size), k))          # ties in DESCENDING input order: a sort that is correct but not stable


SORT_MISSES = ("unstable", "other_mask", "digits_not_reversed")
RANGE_MISSES = ("begin_plus_1", "begin_minus_1", "end_plus_1", "end_minus_1")


def sort_whole(keys, begin_bit, nbits, reverse_digits, whole_bytes, miss=None):
    """permutation of a whole sort: ONE stable sort on the composed key"""
    keys = u64(keys)
    if keys.size <= 1 or nbits <= 0:
        return np.arange(keys.size)
    if miss == "other_mask":
        whole_bytes = not whole_bytes
    if miss == "digits_not_reversed":
        reverse_digits = False
    return stable_order(composed_key(keys, begin_bit, nbits, reverse_digits, whole_bytes), miss == "unstable")


def sort_passes(keys, begin_bit, nbits, reverse_digits, whole_bytes, pass_begin=0, pass_end=-1, miss=None):
    """permutation after the LSD passes [pass_begin, pass_end): one stable sort per pass on that pass's digit"""
    keys = u64(keys)
    perm = np.arange(keys.size)
    if keys.size <= 1 or nbits <= 0:
        return perm
    p = n_passes(nbits)
    end = p if pass_end < 0 else min(pass_end, p)
    if miss == "begin_plus_1":
        pass_begin += 1
    if miss == "begin_minus_1":
        pass_begin = max(0, pass_begin - 1)
    if miss == "end_plus_1":
        end = min(end + 1, p)
    if miss == "end_minus_1":
        end -= 1
    if miss == "other_mask":
        whole_bytes = not whole_bytes
    for q in range(pass_begin, end):
        d = (p - 1 - q) if (reverse_digits and miss != "digits_not_reversed") else q
        perm = perm[stable_order(digit(keys[perm], begin_bit, nbits, d, whole_bytes), miss == "unstable")]
    return perm


# ------------------------------------------------------------------------------------------
# packed anchors: [self 1 | span 8 | qpos bits_qy | sort bits sb]
# ------------------------------------------------------------------------------------------
def unpack(pk, seg, sb, bits_qy, sh_q, miss=None):
    """(key, value) of packed words of segment `seg` (scalar or array)"""
    if miss == "swap_shq_sb":
        sb, sh_q = sh_q, sb
    pk = u64(pk)
    seg = np.asarray(seg, dtype=np.uint64)
    key = shl(seg, sh_q) | (pk & U64(mask(sb)))
    val = shl(shr(pk, sb + bits_qy + 8) & U64(1), 43) | shl(shr(pk, sb + bits_qy) & U64(0xff), 32) | (shr(pk, sb) & U64(mask(bits_qy)))
    return key, val


def anchor_sort(pk, segs, nbits, sb, bits_qy, sh_q, miss=None):
    """segs: (src, length, segment id) in output order.  Every segment stably sorted on its low nbits bits, unpacked, laid out densely."""
    ks, vs = [], []
    for src, ln, sid in segs:
        s = u64(pk[src:src + ln])
        s = s[stable_order(s & U64(mask(nbits)), miss == "unstable")]
        k, v = unpack(s, sid, sb, bits_qy, sh_q, miss)
        ks.append(k)
        vs.append(v)
    if not ks:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)
    return np.concatenate(ks), np.concatenate(vs)


# ------------------------------------------------------------------------------------------
# slots: chunk c holds counts[c] entries at slots[c * cap ...)
# ------------------------------------------------------------------------------------------
def slots_dense(slots, counts, cap, miss=None):
    counts = np.asarray(counts, dtype=np.int64)
    if miss is None:
        parts = [slots[c * cap:c * cap + counts[c]] for c in range(counts.size)]
        return u64(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.uint64)
    assert miss == "first_chunk_of_equal_offsets"
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    i = np.arange(int(counts.sum()))
    c = np.searchsorted(offs, i, side="right") - 1          # the last chunk with offs <= i ...
    c = np.searchsorted(offs, offs[c], side="left")         # ... replaced by the FIRST of those that share its offset
    return u64(slots[c * cap + i - offs[c]])


# ------------------------------------------------------------------------------------------
# run heads
# ------------------------------------------------------------------------------------------
HEAD_MISSES = ("no_head_at_0", "forced_ignored", "forced_at_n", "line_start_missed")


def heads(keys, shift, forced=None, miss=None):
    keys = u64(keys)
    n = keys.size
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    r = shr(keys, shift)
    h = np.flatnonzero(r[1:] != r[:-1]) + 1
    if miss == "line_start_missed":
        h = h[h % 16 != 0]
    parts = [h] if miss == "no_head_at_0" else [[0], h]
    if forced is not None and miss != "forced_ignored":
        f = np.asarray(forced, dtype=np.int64)
        parts.append(f[f <= n] if miss == "forced_at_n" else f[f < n])
    out = np.unique(np.concatenate(parts).astype(np.int64))
    if miss == "no_head_at_0":
        out = out[out != 0]
    return out.astype(np.uint32)


# ------------------------------------------------------------------------------------------
# the significance string of an nbits-bit hash, byte by byte
# ------------------------------------------------------------------------------------------
def hash_to_sig(h, nbits):
    m = (nbits + 7) // 8
    tb = nbits - 8 * (m - 1)
    b = [(h >> (8 * j)) & 0xff for j in range(m)]       # b[0] = low byte = most significant
    s = 0
    for j in range(m - 1):
        s = s << 8 | b[j]
    return s << tb | b[m - 1]


def sig_to_hash(s, nbits):
    m = (nbits + 7) // 8
    tb = nbits - 8 * (m - 1)
    h = (s & mask(tb)) << (8 * (m - 1))
    s >>= tb
    for j in range(m - 2, -1, -1):
        h |= (s & 0xff) << (8 * j)
        s >>= 8
    return h


# ------------------------------------------------------------------------------------------
# the segment-packed index sort: entries (hash h, y = rid << 32 | pos << 1 | strand) in, one packed word per entry out
# ------------------------------------------------------------------------------------------
def sig_of(h, nbits):
    """hash_to_sig over an array"""
    h = u64(h)
    m = (nbits + 7) // 8
    tb = nbits - 8 * (m - 1)
    s = np.zeros(h.size, dtype=np.uint64)
    for j in range(m - 1):
        s = shl(s, 8) | (shr(h, 8 * j) & U64(0xff))
    return shl(s, tb) | (shr(h, 8 * (m - 1)) & U64(0xff))


def y_fields(y, pos1):
    y = u64(y)
    return shr(y, 32), y & U64(mask(pos1))


def segw_entries(h, y, nbits, ybits, pos1):
    """(word, DIG) of the SEGW form: the string's top 16 bits apart, the rest on top of the squeezed position"""
    S = sig_of(h, nbits)
    rid, low = y_fields(y, pos1)
    return u64(shl(S & U64(mask(nbits - 16)), ybits) | shl(rid, pos1) | low), shr(S, nbits - 16).astype(np.uint32)


INDEX_SORT_MISSES = ("unstable", "raw_hash_R", "e_plus_1", "e_minus_1", "rid_at_32", "no_last_start", "a2_low_bits")


def index_sort(h, y, nbits, ybits, pos1, e, miss=None):
    """(words, seg_start): the words R << ybits | rid << pos1 | low in stable order of the significance string S, R its low
    nbits - 8 - e bits; seg_start[s] = entries whose segment S >> (nbits - 8 - e) is smaller, seg_start[256 << e] = n"""
    h, y = u64(h), u64(y)
    if miss == "e_plus_1":
        e += 1
    if miss == "e_minus_1":
        e = max(0, e - 1)
    nr = nbits - 8 - e
    S = sig_of(h, nbits)
    seg = shr(S, nr)
    R = (h if miss == "raw_hash_R" else S) & U64(mask(nr))
    rid, low = y_fields(y, pos1)
    word = shl(R, ybits) | (shl(rid, 32) if miss == "rid_at_32" else shl(rid, pos1)) | low
    key = S
    if miss == "a2_low_bits":           # pass A2 ranks by the low e bits of the second byte b1 = bits [nbits - 16, nbits - 8) of S
        seg = shl(shr(S, nbits - 8), e) | (shr(S, nbits - 16) & U64(mask(e)))
        key = shl(seg, nr) | R
    order = stable_order(key, miss == "unstable")
    starts = np.searchsorted(seg[order], np.arange((256 << e) + 1, dtype=np.uint64), side="left").astype(np.uint32)
    if miss == "no_last_start":
        starts[-1] = 0
    return u64(word[order]), starts


# ==========================================================================================
# case families (fixed seeds)
# ==========================================================================================
SCAN_SMALL_N = (0, 1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 5)
SCAN_BIG_N = (33554432, 33554433)           # the last single-level size and the first two-level size
SCAN_FILLS = ("random", "zeros", "ends", "max_total")
SS_N = (1, 31, 32, 33, 8191, 8192, 8193, 3 * 8192 + 5)


def scan_input(n, fill, seed=1):
    rng = np.random.Generator(np.random.PCG64(seed + n))
    if fill == "random":
        return rng.integers(0, 1000, n, dtype=np.uint32)
    if fill == "big":
        return rng.integers(0, 4, n, dtype=np.uint32)      # totals of 33 M items stay below 2^32
    a = np.zeros(n, dtype=np.uint32)
    if n and fill == "ends":
        a[0] = 7
        a[-1] += 11
    if n and fill == "max_total":                        # a total of exactly 2^32 - 1
        a[:] = ((1 << 32) - 1) // n
        a[n // 2] += ((1 << 32) - 1) - int(a.astype(np.uint64).sum())
    return a


SORT_N = (0, 1, 2, 63, 64, 65, 4095, 4096, 4097) + tuple(t * 4096 - 5 for t in range(1, 18)) + (65 * 4096 + 17,)
SORT_BITS = ((0, 30), (0, 38), (0, 46), (32, 1), (32, 17), (0, 16), (0, 1), (0, 7), (0, 9), (0, 64), (13, 51))
SORT_RANGES = ((0, 1), (1, -1), (0, -1), (2, 3), (1, 1))
KEY_KINDS = ("uniform", "all_equal", "two_digits", "all_ones", "ascending", "descending", "row_same_digit", "lane_distinct_digit",
             "third_repeated", "differ_above")


def sort_keys_of(kind, n, begin_bit, nbits, seed=2):
    """n keys whose sort field is of the given kind; the input position fills the bits outside the field (directly above the field first, the
    rest below begin_bit), so that a stable sort is told from an unstable one -- and so that keys differ above begin_bit + nbits."""
    rng = np.random.Generator(np.random.PCG64(seed * 1000003 + n * 131 + begin_bit * 7 + nbits))
    pos = np.arange(n, dtype=np.uint64)
    fm = U64(mask(nbits))
    if kind == "all_ones":
        return np.full(n, M64, dtype=np.uint64)
    if kind == "uniform":
        f = rng.integers(0, 1 << 63, n, dtype=np.uint64) * U64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    elif kind in ("all_equal", "differ_above"):
        f = np.full(n, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    elif kind == "two_digits":
        f = np.where(rng.integers(0, 2, n) == 1, U64(0x0101010101010101), U64(0xFEFEFEFEFEFEFEFE))
    elif kind == "ascending":
        f = pos * U64(max(1, mask(nbits) // max(1, n)))
    elif kind == "descending":
        f = (U64(n) - pos) * U64(max(1, mask(nbits) // max(1, n + 1)))
    elif kind == "row_same_digit":
        f = ((pos // U64(64)) % U64(251)) * U64(0x0101010101010101)
    elif kind == "lane_distinct_digit":
        f = ((pos % U64(64)) * U64(4) + (pos // U64(64)) % U64(4)) * U64(0x0101010101010101)
    elif kind == "third_repeated":
        f = rng.integers(0, 1 << 63, n, dtype=np.uint64) * U64(2) + rng.integers(0, 2, n, dtype=np.uint64)
        pool = rng.integers(0, 1 << 63, 37, dtype=np.uint64)
        rep = rng.integers(0, 3, n) == 0
        f[rep] = pool[rng.integers(0, 37, int(rep.sum()))]
    else:
        raise ValueError(kind)
    hi_free = 64 - begin_bit - nbits
    k = shl(f & fm, begin_bit) | (shr(pos, hi_free) & U64(mask(begin_bit)))
    if hi_free:
        k |= shl(pos & U64(mask(hi_free)), begin_bit + nbits)
    return u64(k)


def slot_tables():
    """(name, cap, counts): chunk tables for the three paths of rs_for_slot_items, with runs of empty chunks in front, in the middle
    and at the end, and totals that are a multiple of RS_TILE and one more than a multiple"""
    rng = np.random.Generator(np.random.PCG64(77))
    out = []

    def finish(name, cap, counts, want_total):
        counts = list(int(c) for c in counts)
        # runs of empty chunks: first, middle, last
        mid = len(counts) // 2
        counts = [0] * 5 + counts[:mid] + [0] * 9 + counts[mid:]
        tot = sum(counts)
        while tot < want_total:                         # top up with chunks of the table's own kind
            c = min(cap, want_total - tot)
            counts.append(c)
            tot += c
        while tot > want_total:
            j = max(i for i, c in enumerate(counts) if c)
            d = min(counts[j], tot - want_total)
            counts[j] -= d
            tot -= d
        counts += [0] * 7
        out.append((name, cap, np.array(counts, dtype=np.uint32)))

    for extra in (0, 1):
        finish("cap8_search_%d" % extra, 8, rng.integers(0, 9, 2200), 2 * RS_TILE + extra)                       # a tile spans ~1 000 chunks: per-entry search
        finish("cap64_43_%d" % extra, 64, rng.integers(38, 49, 280), 3 * RS_TILE + extra)                       # ~95 chunks a tile: offsets cached in LDS
        finish("cap64_full_empty_%d" % extra, 64, [64 if i % 3 == 0 else 0 for i in range(600)], 3 * RS_TILE + extra)
        finish("cap1024_desc_%d" % extra, 1024, rng.choice([0, 1, 700, 1024], 40, p=[0.2, 0.2, 0.3, 0.3]), 5 * RS_TILE + extra)   # some tiles within six slots, some not
        finish("cap4096_desc_%d" % extra, 4096, rng.choice([0, 1, 700, 4096], 24, p=[0.25, 0.25, 0.25, 0.25]), 6 * RS_TILE + extra)
        finish("cap1024_seventh_%d" % extra, 1024, [700] * 16, 3 * RS_TILE + extra)                               # 4096 / 700: a tile spans six slots or needs a seventh
    return out


def slots_fill(cap, counts, dense):
    """the slot array: the dense keys chunk by chunk, every unused word a value no key has"""
    counts = np.asarray(counts, dtype=np.int64)
    slots = (U64(0xDEAD000000000000) | np.arange(counts.size * cap, dtype=np.uint64))
    o = 0
    for c in range(counts.size):
        slots[c * cap:c * cap + counts[c]] = dense[o:o + counts[c]]
        o += counts[c]
    return u64(slots)


def slot_tile_spans(cap, counts):
    """per tile of RS_TILE dense entries, how many chunks lie between the one holding its first entry and the one holding its last"""
    counts = np.asarray(counts, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    total = int(counts.sum())
    spans = []
    for t0 in range(0, total, RS_TILE):
        last = min(total, t0 + RS_TILE) - 1
        spans.append(int(np.searchsorted(offs, last, side="right") - np.searchsorted(offs, t0, side="right")) + 1)
    return spans


SEG_LENS = (1, 2, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 16383, 16384)
SEG_NBITS = (1, 7, 8, 9, 17, 18, 27, 34, 36)
SEG_KINDS = ("uniform", "all_ones", "one_digit", "two_values")


def seg_payload_bits(nbits):
    """(sb, bits_qy, sh_q): the sort bits, a payload that reaches the word's top, and the segment shift (the product's sh_q == sb at the
    even widths; two more at the odd ones, so that swapping the two is visible)"""
    return nbits, 64 - 9 - nbits, nbits + (2 if nbits & 1 else 0)


def seg_words(kind, lens, nbits, slack=0, seed=5):
    """packed anchors of the given segment lengths, segment after segment (`slack` unused words behind every segment: the sparse layout
    of the dead-pair filter).  qpos holds the position inside the segment, so stability shows; self and span are random."""
    rng = np.random.Generator(np.random.PCG64(seed * 7919 + nbits * 31 + slack))
    sb, bits_qy, _ = seg_payload_bits(nbits)
    words, segs, src = [], [], 0
    for sid, ln in enumerate(lens):
        pos = np.arange(ln, dtype=np.uint64)
        if kind == "uniform":
            f = rng.integers(0, 1 << 62, ln, dtype=np.uint64)
        elif kind == "all_ones":
            f = np.full(ln, M64, dtype=np.uint64)
        elif kind == "one_digit":
            f = np.full(ln, 0x2A2A2A2A2A2A2A2A, dtype=np.uint64)
        elif kind == "two_values":
            f = np.where(rng.integers(0, 2, ln) == 1, U64(M64), U64(0))
        else:
            raise ValueError(kind)
        qpos = (pos | shl(rng.integers(0, 1 << 40, ln, dtype=np.uint64), 14)) & U64(mask(bits_qy))
        top = rng.integers(0, 512, ln, dtype=np.uint64)                     # span 8 | self 1
        w = (f & U64(mask(sb))) | shl(qpos, sb) | shl(top, sb + bits_qy)
        words.append(u64(w))
        if slack:
            words.append(U64(0xBAD0000000000000) | np.arange(slack, dtype=np.uint64))
        segs.append((src, ln, sid))
        src += ln + slack
    return np.concatenate(words), segs


def plan_anchor_sort(segs, local_class):
    """OverlapRun::plan_anchor_sort: local_class(length) = 0, 1, 2 for a segment sorted in LDS, None for the tiled global sort.  Returns
    (SegDesc words per class, SegTile words, n_local)."""
    h_local = [[], [], []]
    tiles = []
    off = tb = n_local = 0
    for src, c, sid in segs:
        cls = local_class(c) if c else None
        if cls is not None:
            h_local[cls].append((off, c, sid, src))
            off += c
            n_local += c
            continue
        nt = (c + RS_TILE - 1) // RS_TILE
        for lt in range(nt):
            tiles.append((off + lt * RS_TILE, min(RS_TILE, c - lt * RS_TILE), 256 * tb + lt, nt, sid, n_local, src + lt * RS_TILE, 0))
        off += c
        tb += nt
    return [np.array(v, dtype=np.uint32).reshape(-1, 4) for v in h_local], np.array(tiles, dtype=np.uint32).reshape(-1, 8), n_local


HEAD_N = (0, 1, 15, 16, 17, 4095, 4096, 4097, 5 * 4096 + 9)
HEAD_SHIFTS = (0, 13, 63)
HEAD_STREAMS = ("one_run", "all_distinct", "every_16", "every_4096", "last_alone", "random")


def head_stream(kind, n, shift, seed=9):
    """n keys whose (key >> shift) changes where the kind says; the bits below `shift` are random and must not matter"""
    rng = np.random.Generator(np.random.PCG64(seed + n * 17 + shift))
    i = np.arange(n, dtype=np.uint64)
    if kind == "one_run":
        run = np.zeros(n, dtype=np.uint64)
    elif kind == "all_distinct":
        run = i
    elif kind == "every_16":
        run = i // U64(16)
    elif kind == "every_4096":
        run = i // U64(4096)
    elif kind == "last_alone":
        run = (i == U64(max(0, n - 1))).astype(np.uint64)
    elif kind == "random":
        run = np.cumsum(rng.integers(0, 8, n) == 0).astype(np.uint64)
    else:
        raise ValueError(kind)
    run &= U64(mask(64 - shift))                       # (shift 63: the runs alternate between 0 and 1)
    low = rng.integers(0, 1 << 62, n, dtype=np.uint64) & U64(mask(shift))
    return u64(shl(run, shift) | low)


def head_boundaries(keys, shift, n_seg, seed=11):
    """n_seg + 1 ascending forced boundaries: 0 and n, natural heads, positions inside runs of equal keys, repeats (empty segments)"""
    n = keys.size
    rng = np.random.Generator(np.random.PCG64(seed + n + n_seg))
    nat = heads(keys, shift).astype(np.int64)
    pick = [np.array([0, n, n], dtype=np.int64)]
    if nat.size:
        pick.append(rng.choice(nat, min(nat.size, n_seg // 4)))
    if n:
        pick.append(rng.integers(0, n, n_seg // 4))                          # mostly inside runs
        pick.append(np.array([min(n - 1, 16), min(n - 1, 4096), n - 1], dtype=np.int64))
    b = np.concatenate(pick)
    b = np.concatenate([b, rng.choice(b, n_seg + 1 - b.size)]) if b.size < n_seg + 1 else b[:n_seg + 1]
    b = np.sort(b)
    b[0] = 0
    b[-1] = n
    return b.astype(np.uint32)


INDEX_N = (1, 255, 4095, 4096, 4097, 3 * 4096 + 5, 17 * 4096 - 5)
INDEX_NBITS = (24, 30, 38)
INDEX_E = (0, 1, 6, 7)
HASH_KINDS = ("uniform", "one_b0", "one_per_segment", "all_equal", "a2_bits_only", "below_a2_only")


def index_layout(nbits, e, tight):
    """(ybits, pos1): the tight word has no bit to spare, nbits - 8 - e + ybits == 64; the loose one leaves the top unused.  The read
    number takes ybits - pos1 <= 32 bits, and pos1 < 32, so that a read number left at bit 32 shows."""
    ybits = 64 - (nbits - 8 - e) if tight else 30
    return ybits, max(12, ybits - 32)


def index_entries(kind, n, nbits, ybits, pos1, e, seed=13):
    """(h, y): n hashes of the given kind and positions that hold the input index (stability shows) under random bits up to the top of
    the read number"""
    rng = np.random.Generator(np.random.PCG64(seed * 7919 + n * 31 + nbits * 5 + e))
    i = np.arange(n, dtype=np.uint64)
    u = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    base = U64(0x2A5A5A5A5A5A5A5A)
    if kind == "uniform":
        h = u
    elif kind == "one_b0":                  # one of pass A's segments spans every tile, 255 are empty
        h = (u & ~U64(0xff)) | U64(0x5A)
    elif kind == "one_per_segment":         # n < 256 distinct low bytes in shuffled order: empty segments between
        assert n < 256
        b0 = rng.permutation(256)[:n].astype(np.uint64)
        h = (u & ~U64(0xff)) | b0
    elif kind == "all_equal":
        h = np.full(n, base, dtype=np.uint64)
    elif kind == "a2_bits_only":            # equal but for the top e bits of the second byte: what pass A2 ranks by
        m = U64(mask(e) << (16 - e))
        h = (base & ~m) | (u & m)
    elif kind == "below_a2_only":           # equal but for the bits of the second byte below those: the top of R
        m = U64(mask(8 - e) << 8)
        h = (base & ~m) | (u & m)
    else:
        raise ValueError(kind)
    h &= U64(mask(nbits))
    rbits = ybits - pos1
    low = i & U64(mask(pos1))
    rid = (shr(i, pos1) | shl(rng.integers(0, 1 << 32, n, dtype=np.uint64), 5)) & U64(mask(rbits))       # (n < 2^17, pos1 >= 12: five bits hold the rest of i)
    return u64(h), u64(shl(rid, 32) | low)


INDEX_GROUPS = ("layouts", "sizes") + HASH_KINDS


def index_cases(group):
    """(kind, n, nbits, e, tight) of one group: every nbits x e x layout at a few tiles; every size (with and without pass A2, the narrowest
    and the widest R); every hash kind at every e"""
    if group == "layouts":
        return [("uniform", 3 * 4096 + 5, nbits, e, tight) for nbits in INDEX_NBITS for e in INDEX_E for tight in (False, True)]
    if group == "sizes":
        return [c for n in INDEX_N for c in (("uniform", n, 30, 0, False), ("uniform", n, 38, 6, True), ("all_equal", n, 24, 7, False))]
    n = 255 if group == "one_per_segment" else 2 * 4096 + 5
    return [c for e in INDEX_E for c in ((group, n, 38, e, False), (group, n, 24, e, True))]


def index_forms(h, y, nbits, ybits, pos1, cap, counts):
    """the same entries as the sort's three sources: the pairs, the dense SEGW arrays, the wave-dense slots (words, DIG members, counts)"""
    w, d = segw_entries(h, y, nbits, ybits, pos1)
    return (h, y), (w, d), (slots_fill(cap, counts, w), slots_fill(cap, counts, d.astype(np.uint64)).astype(np.uint32), np.asarray(counts, dtype=np.uint32))


def wave_table_for(n, cap=2816, seed=21):
    """per-wavefront counts of a wave-dense sketch that holds n entries: slots of `cap` (a multiple of 64), 2 000 to cap entries in
    each, an empty wavefront now and then, the last one taking what is left"""
    rng = np.random.Generator(np.random.PCG64(seed + n))
    counts, left = [0], n
    while left:
        c = min(left, int(rng.integers(2000, cap + 1)))
        counts.append(c)
        left -= c
        if rng.integers(0, 4) == 0:
            counts.append(0)
    return cap, np.array(counts + [0], dtype=np.uint32)


def index_slot_tables():
    """the chunk tables a wave-dense sketch could have left: cap a multiple of 64 and at most RS_TILE"""
    return [t for t in slot_tables() if t[1] % 64 == 0 and t[1] <= RS_TILE]


SIG_NBITS = (30, 38, 8, 9, 16, 17, 63)


def sort_cases(group):
    """(kind, n, begin_bit, nbits, reverse_digits) of one group of whole-sort cases"""
    out = []
    if group == "sizes":
        for n in SORT_N:
            out += [("third_repeated", n, 0, 30, True), ("uniform", n, 13, 51, False)]
    elif group == "bits":
        for b, nb in SORT_BITS:
            for rev in (False, True):
                for n in (4097, 3 * 4096 - 5):
                    out += [("third_repeated", n, b, nb, rev), ("differ_above", n, b, nb, rev)]
    elif group == "kinds":
        for kind in KEY_KINDS:
            for b, nb in SORT_BITS:
                for rev in (False, True):
                    out.append((kind, 2 * 4096 - 5, b, nb, rev))
    else:
        raise ValueError(group)
    return out


SORT_GROUPS = ("sizes", "bits", "kinds")


def range_cases():
    """(n, begin_bit, nbits, reverse_digits, pass_begin, pass_end) of the partial sorts"""
    return [(3 * 4096 - 5, b, nb, rev, pb, pe) for b, nb in SORT_BITS for rev in (False, True) for pb, pe in SORT_RANGES]


def head_cases():
    return [(kind, n, shift) for kind in HEAD_STREAMS for n in HEAD_N for shift in HEAD_SHIFTS]
