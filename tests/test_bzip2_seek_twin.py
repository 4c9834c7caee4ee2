"""The seek map of bzip2 without a GPU (lrge_amd/csrc/fx_seek.h FX_SEEK_BZIP2, bz_round.h BzSeekRec, bz_core.h BzMarkRec /
bz_segment_lane): the host twin runs the census with the recorder and the mark sinks the device uses, enters every
block at every mark with the body the kernel runs lane by lane, plans with the planner the device uses and runs the mapped pass over
the sub-text the seeded decodes give.  The reference is libbz2, the text itself and a plain simulation of the run-length layer made
from the writer's own rle1 output."""
import bz2
import ctypes as C
import random

import numpy as np
import pytest

import bzip2_writer as BW
import gzip_corpus as G
from test_bzip2_twin import btwin, run as bz_inflate   # noqa: F401  (fixture)
from test_fastx_select_twin import OK, UNPROVEN, FxRec, selected
from test_fastx_select_twin import twin as _select_twin   # noqa: F401  (fixture)
from test_fastx_seek_twin import bind as bind_seek

MARKS = 64
E_ENTRY = 16        # bz_core.h BZ_E_ENTRY


def bind(L):
    """the prototypes of the twin's bzip2 map entries (the GPU suite binds them too)"""
    bind_seek(L)
    L.fastx_twin_bz_census_map.argtypes = [C.c_char_p] + [C.c_uint64] * 7 + [C.POINTER(C.c_uint64 * 4)]
    L.fastx_twin_bz_stats.argtypes = [C.POINTER(C.c_uint64 * 5)]
    L.fastx_twin_gz_text.argtypes = [C.c_char_p]
    L.fastx_twin_gz_text.restype = C.c_uint64
    L.fastx_twin_bz_entries.argtypes = [C.c_void_p, C.c_uint64]
    L.fastx_twin_bz_entries.restype = C.c_uint64
    L.fastx_twin_bz_blocks.argtypes = [C.c_void_p, C.c_uint64]
    L.fastx_twin_bz_blocks.restype = C.c_uint64
    L.fastx_twin_bz_marks.argtypes = [C.c_uint64, C.c_void_p]
    L.fastx_twin_bz_poke_mark.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
    L.fastx_twin_bz_segment.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_char_p, C.POINTER(C.c_uint64)]
    L.fastx_twin_bz_mapped.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)]
    L.fastx_twin_plan_stats.argtypes = [C.POINTER(C.c_uint64 * 4)]
    return L


@pytest.fixture(scope="module")
def twin(_select_twin):
    return bind(_select_twin)


def stream(plain=b"", size=1500, level=1, parts=None):
    """bzip2_writer.stream's bytes, every block written into a bit string of its own and joined once (the writer's single bit string
    costs time quadratic in the file).  parts: [(pre, plain)] as the writer's raw_blocks"""
    parts = parts if parts is not None else [(BW.rle1(plain[i:i + size]), plain[i:i + size]) for i in range(0, len(plain), size)]
    head = BW.Bits()
    for ch in b"BZh":
        head.put(ch, 8)
    head.put(48 + level, 8)
    v, n, combined = head.v, head.n, 0
    for pre, text in parts:
        b = BW.Bits()
        BW.block(b, pre, text)
        v, n = (v << b.n) | b.v, n + b.n
        combined = (((combined << 1) | (combined >> 31)) & 0xFFFFFFFF) ^ BW.crc(text)
    tail = BW.Bits()
    tail.put(BW.END_MAGIC, 48)
    tail.put(combined, 32)
    v, n = (v << tail.n) | tail.v, n + tail.n
    return (v << (-n % 8)).to_bytes((n + 7) // 8, "big")


def census(L, data, spacing, round_blocks=0, window=20000, stride=512, tile=64):
    """(verdict, counts, blocks [(bit, end bit, off, len, n, orig, crc, entry)], entries [(b0, b1, off, len, f0, f1)], text) of the
    twin's census with a map on bzip2 bytes; blocks, entries and text are there whether or not the text is FASTA / FASTQ"""
    out = (C.c_uint64 * 4)()
    rc = L.fastx_twin_bz_census_map(data, len(data), round_blocks, spacing, tile, window, 4096, stride, C.byref(out))
    k = L.fastx_twin_bz_blocks(None, 0)
    b = np.zeros((max(1, k), 8), dtype=np.uint64)
    L.fastx_twin_bz_blocks(b.ctypes.data, k)
    ke = L.fastx_twin_bz_entries(None, 0)
    e = np.zeros((max(1, ke), 6), dtype=np.uint64)
    L.fastx_twin_bz_entries(e.ctypes.data, ke)
    text = C.create_string_buffer(max(1, L.fastx_twin_gz_text(None)))
    n = L.fastx_twin_gz_text(text)
    return rc, list(out), [tuple(int(x) for x in r) for r in b[:k]], [tuple(int(x) for x in r) for r in e[:ke]], text.raw[:n]


def marks_of(L, b):
    """[(at, state, text offset, CRC register)] * 64 of block b"""
    m = np.zeros((MARKS, 4), dtype=np.uint32)
    L.fastx_twin_bz_marks(b, m.ctypes.data)
    return [tuple(int(x) for x in r) for r in m]


def segment(L, data, b, j, skew=0, cap=1 << 20):
    """(status, text) of lane j of block b alone from its mark; j = 64: the block by all lanes"""
    buf, ln = C.create_string_buffer(cap), C.c_uint64()
    rc = L.fastx_twin_bz_segment(data, len(data), b, j, skew, buf, C.byref(ln))
    return rc, buf.raw[:ln.value]


def mapped(L, data, text, window, piece, sel, tile=64):
    """(verdict, [(name, sequence)], store, select stats, block status) of the mapped pass on the last map, read as `selected` reads"""
    a = np.ascontiguousarray(sel, dtype=np.uint32)
    st = C.c_uint32()
    rc = L.fastx_twin_bz_mapped(data, len(data), tile, window, piece, a.ctypes.data if a.size else None, a.size, C.byref(st))
    if rc != OK:
        return rc, None, None, None, st.value
    n = L.fastx_twin_windowed_count()
    tab = (FxRec * max(1, n))()
    L.fastx_twin_windowed_table(tab)
    ss = (C.c_uint64 * 4)()
    L.fastx_twin_select_stats(C.byref(ss))
    out, at, buf = [], 0, C.create_string_buffer(max(1, max((tab[i].seq_len for i in range(n)), default=0)))
    for i in range(n):
        r = tab[i]
        assert L.fastx_twin_windowed_seq(i, buf) == r.seq_len
        out.append((text[r.name_off:r.name_off + r.name_len], buf.raw[:r.seq_len]))
        at += r.seq_len
    store = C.create_string_buffer(max(1, at))
    assert L.fastx_twin_windowed_store(store, at) == at
    return rc, out, store.raw[:at], list(ss), 0


def plan_stats(L):
    out = (C.c_uint64 * 4)()
    L.fastx_twin_plan_stats(C.byref(out))
    return tuple(int(x) for x in out)


# ---- the reference: the run-length layer and the walk in plain Python ----
def seg_of(n):
    return max(4, 4 * -(-n // 256))


def sim_marks(pre):
    """[(state, text offset, CRC register)] in front of every step j * seg of `pre`, and the text length"""
    seg, prev, run, off, c, out = seg_of(len(pre)), 256, 0, 0, 0xFFFFFFFF, []
    for i, b in enumerate(pre):
        if i % seg == 0:
            out.append((prev | run << 16, off, c))
        if run == 4:
            for _ in range(b):
                c = ((c << 8) & 0xFFFFFFFF) ^ BW._CRC[(c >> 24) ^ prev]
            off, run, prev = off + b, 0, 256
            continue
        prev, run = (prev, run + 1) if b == prev else (b, 1)
        c = ((c << 8) & 0xFFFFFFFF) ^ BW._CRC[(c >> 24) ^ b]
        off += 1
    return out, off


def walk_ats(pre):
    """the walk pointer in front of every step j * seg, from the BWT column of `pre` by a stable sort"""
    col, at = BW.bwt(pre)
    nxt = sorted(range(len(col)), key=lambda i: (col[i], i))
    seg, out = seg_of(len(pre)), []
    for i in range(len(pre)):
        if i % seg == 0:
            out.append(at)
        at = nxt[at]
    assert at == BW.bwt(pre)[1]
    return out


def unrle(pre):
    out, prev, run = bytearray(), None, 0
    for b in pre:
        if run == 4:
            out += bytes([prev]) * b
            prev, run = None, 0
            continue
        prev, run = (prev, run + 1) if b == prev else (b, 1)
        out.append(b)
    assert run != 4
    return bytes(out)


def filler(rng, n, alphabet=b"CGT\n"):
    """n bytes without four equal in a row"""
    out = bytearray()
    while len(out) < n:
        b = rng.choice(alphabet)
        if len(out) < 3 or not (out[-1] == out[-2] == out[-3] == b):
            out.append(b)
    return bytes(out)


RUNS = {"run4": b"AAAA\x00", "run5": b"AAAA\x01", "run259": b"AAAA\xff", "run260": b"AAAA\xffA", "count0": b"AAAA\x00G"}


def shaped_blocks():
    """[(name, pre)]: every block length of the issue, and every run shape shifted through every residue of the segment length, at
    segment lengths 4 and 8"""
    rng = random.Random(29)
    out = [("n%d" % n, filler(rng, n, b"ACGT\n")) for n in (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 260, 1500)]
    for kind, enc in RUNS.items():
        for total in (40, 300):                                   # seg 4 and seg 8
            for shift in range(seg_of(total)):
                pre = filler(rng, shift) + enc + b"C" + filler(rng, total - shift - len(enc) - 1)
                out.append(("%s_seg%d_shift%d" % (kind, seg_of(total), shift), pre))
    return out


@pytest.fixture(scope="module")
def shaped(twin):
    blocks = shaped_blocks()
    parts = [(pre, unrle(pre)) for _, pre in blocks]
    data = stream(parts=parts)
    assert bz2.decompress(data) == b"".join(t for _, t in parts)
    return blocks, parts, data


def check_block(L, data, b, blk, pre, text, what, skews=(0,)):
    """block b of the last map against the simulation of `pre`: every mark, every lane alone, the block by all lanes"""
    bit, end_bit, off, ln, n, orig, crc, ent = blk
    assert (n, ln, crc) == (len(pre), len(text), BW.crc(text)), what
    want, total = sim_marks(pre)
    assert total == ln and len(want) == -(-n // seg_of(n)) <= MARKS, what
    got = marks_of(L, b)
    assert [m[1:] for m in got[:len(want)]] == want, what
    assert all(m == (0, 0, 0, 0) for m in got[len(want):]), what
    offs = [w[1] for w in want] + [ln]
    for j in range(MARKS):
        rc, seg = segment(L, data, b, j, skew=(j + skews[0]) & 3)
        assert rc == 0 and seg == (text[offs[j]:offs[j + 1]] if j < len(want) else b""), (what, j, rc)
    for skew in skews:
        rc, whole = segment(L, data, b, MARKS, skew=skew)
        assert rc == 0 and whole == text, (what, skew, rc)
    return got[:len(want)]


def test_recorder_changes_nothing(twin, btwin):
    """the census with the recorder gives the bytes and the counts of the twin's inflate without one, at every round size"""
    text = G.fastq(600)[:250000]
    for data in (bz2.compress(text, 1), stream(text[:40000], size=1500)):
        for round_blocks in (0, 1, 2, 7):
            rc0, plain, st, _ = bz_inflate(btwin, data, round_blocks)
            assert rc0 == 0 and plain == bz2.decompress(data)
            rc, out, blocks, ents, got = census(twin, data, 1, round_blocks=round_blocks, window=1 << 30, stride=65536, tile=4096)
            assert rc == OK and got == plain
            s = (C.c_uint64 * 5)()
            twin.fastx_twin_bz_stats(C.byref(s))
            assert dict(zip(("blocks", "candidates", "rejected_candidates", "rounds", "bytes_out"), list(s))) == st
            assert len(blocks) == st["blocks"]


def test_libbz2_level_1(twin):
    """about 250 KB at level 1: three blocks of seg 1564; entries and blocks tile libbz2's text, every mark's state, offset and CRC
    register equal the simulation (libbz2's run-length layer is the writer's rule), every segment alone is its slice of the text"""
    text = G.fastq(600)[:250000]
    data = bz2.compress(text, 1)
    rc, out, blocks, ents, got = census(twin, data, 1, window=1 << 30, stride=65536, tile=4096)
    assert rc == OK and got == text == bz2.decompress(data) and len(blocks) == 3 and len(ents) == 3
    assert blocks[0][0] == 32 and seg_of(blocks[0][4]) == 1564
    at = 0
    for b, blk in enumerate(blocks):
        assert blk[2] == at and (b == 0 or blk[0] == blocks[b - 1][1]) and blk[7] == b
        at += blk[3]
    assert at == len(text) and blocks[-1][1] + 80 + 7 >> 3 == len(data)
    for i, (b0, b1, off, ln, f0, f1) in enumerate(ents):
        assert (b0, b1, off, ln) == (i, i + 1, blocks[i][2], blocks[i][3]) and (f0, f1) == (blocks[i][0] >> 3, blocks[i][1] + 7 >> 3)
    for b, blk in enumerate(blocks):
        t = text[blk[2]:blk[2] + blk[3]]
        marks = check_block(twin, data, b, blk, BW.rle1(t), t, ("libbz2", b), skews=(b,))
        assert marks[0][0] == blk[5]                          # mark 0 stands at origPtr


def test_block_shapes(twin, shaped):
    """block lengths with idle lanes and seg 4 and 8, runs of 4, 5, 259 and 260 and a count of 0 at every residue of the segment: marks
    equal the simulation, `at` the walk of the writer's BWT column, every segment its slice.  The corpus must show every run state 0..4
    at some mark and a count byte as the first byte of some segment"""
    blocks, parts, data = shaped
    rc, out, got_blocks, ents, got = census(twin, data, 1, window=1 << 30, stride=65536, tile=4096)
    assert rc in (OK, UNPROVEN) and got == b"".join(t for _, t in parts) and len(got_blocks) == len(blocks)      # (the text is no FASTA / FASTQ)
    states, segs = set(), set()
    for b, ((name, pre), (_, text)) in enumerate(zip(blocks, parts)):
        marks = check_block(twin, data, b, got_blocks[b], pre, text, name, skews=(0, 1, 2, 3) if b % 7 == 0 else (b & 3,))
        assert [m[0] for m in marks] == walk_ats(pre), name
        states |= {m[1] >> 16 for m in marks}
        segs.add(seg_of(len(pre)))
    assert states == {0, 1, 2, 3, 4}, states                   # (4: the segment's first byte is a count byte)
    assert {4, 8} <= segs and any(len(pre) < 64 for _, pre in blocks)


def entries_by_rule(blocks, spacing):
    out = []
    for b, blk in enumerate(blocks):
        if not out or blk[2] >= out[-1][2] + spacing:
            out.append([b, b, blk[2], 0])
        out[-1][1] += 1
        out[-1][3] += blk[3]
    return [tuple(e) for e in out]


@pytest.fixture(scope="module")
def fq():
    text = G.fastq(130)
    return text, stream(text, size=1500)


def test_spacings_group_blocks(twin, fq):
    text, data = fq
    seen = {}
    for spacing in (1, 2000, 7000, 40000, len(text) + 1):
        rc, out, blocks, ents, got = census(twin, data, spacing)
        assert rc == OK and got == text and out[0] == 130 and len(blocks) == -(-len(text) // 1500)
        assert [e[:4] for e in ents] == entries_by_rule(blocks, spacing), spacing
        assert all((e[4], e[5]) == (blocks[e[0]][0] >> 3, blocks[e[1] - 1][1] + 7 >> 3) for e in ents)
        assert [blk[7] for blk in blocks] == [i for i, e in enumerate(ents) for _ in range(e[0], e[1])]
        assert twin.fastx_twin_bz_enterable() == (1 if len(ents) > 1 else 0)
        seen[spacing] = len(ents)
    assert seen[1] == len(blocks) and seen[len(text) + 1] == 1 and seen[1] > seen[2000] > seen[7000] > seen[40000] > 1, seen
    # a file of one block is one entry and is entered
    one = stream(text[:1200], size=1500)
    rc, out, blocks, ents, got = census(twin, one, 1 << 19)
    assert len(blocks) == len(ents) == 1 and twin.fastx_twin_bz_enterable() == 1


def test_mapped_equals_selected(twin, fq):
    """selections of 0, 1, 7 and all records at spacings that put one and several blocks into an entry: the mapped pass gives the
    records, the store and the statistics of the selecting pass over the whole text, and decodes what the planner counts"""
    text, data = fq
    rng = np.random.default_rng(3)
    for spacing in (1, 7000):
        rc, out, blocks, ents, got = census(twin, data, spacing)
        n = out[0]
        for sel in ([], [n // 2], sorted(rng.permutation(n)[:7].tolist()), list(range(n))):
            want = selected(twin, text, 20000, 4096, sel)
            rc, rec, store, ss, _ = mapped(twin, data, text, 20000, 4096, sel)
            assert rc == OK and (rec, store, ss) == (want[1], want[2], want[3]), (spacing, len(sel))
            st = plan_stats(twin)
            assert (st[0] > 0) == bool(sel) and st[3] <= len(ents) and st[2] <= len(data)
            if len(sel) == 1:
                assert 1 <= st[3] <= 2 and st[2] < len(data) // 2 and st[1] < len(text) // 4, st     # (a run of one cell lies in one entry or across one seam)


def test_changed_byte_in_a_needed_range(twin, fq):
    """a byte of a needed block changes after the census: the block fails its decode or arrives elsewhere than its marks say
    (BZ_E_ENTRY) -- or the byte was none of the block's bits and the reads are the same; never other text"""
    text, data = fq
    rc, out, blocks, ents, got = census(twin, data, 1)
    sel = [out[0] // 2]
    want = mapped(twin, data, text, 20000, 4096, sel)
    assert want[0] == OK
    (b0, b1, off, ln, f0, f1), = [ents[i] for i in range(len(ents)) if ents[i][2] <= text.index(b"\n@read%05d " % sel[0]) + 1 < ents[i][2] + ents[i][3]]
    refused = set()
    for at in range(f0, f1, 3):
        for flip in (0x01, 0x40):
            bad = bytearray(data)
            bad[at] ^= flip
            rc, rec, store, ss, status = mapped(twin, bytes(bad), text, 20000, 4096, sel)
            if rc == OK:
                assert (rec, store, ss) == want[1:4] and at in (f0, f1 - 1), at     # (bits of the neighbouring block in a shared byte)
            else:
                assert rc == UNPROVEN and status != 0, (at, rc, status)
                refused.add(status)
    assert E_ENTRY in refused or len(refused) > 1, refused
    # a damaged map: one word of one mark of the needed block
    for word in range(4):
        rc, out, blocks, ents, got = census(twin, data, 1)
        twin.fastx_twin_bz_poke_mark(b0, 1, word, 0x00030041 if word == 1 else 7)
        rc, rec, store, ss, status = mapped(twin, data, text, 20000, 4096, sel)
        assert rc == UNPROVEN and status == E_ENTRY, (word, rc, status)


def test_abi_and_kernels():
    """the seeded decode and the recording forms are kernels of the library; the status has its message"""
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "lrge_amd", "csrc", "k_bzip2.h")).read()
    for k in ("k_bz_marks_text", "k_bz_walk_rec", "k_bz_rle_write_rec"):
        assert "void %s(" % k in src
    assert "FX_SEEK_BZIP2 = 5" in open(os.path.join(here, "..", "lrge_amd", "csrc", "fx_seek.h")).read()
