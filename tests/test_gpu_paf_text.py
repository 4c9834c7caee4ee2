"""GPU: overlaps.paf written on the device (lrge_hip_paf_text).  The model is lrge_amd/paf.py: paf_lines over
Index.chains + Index.paf_stats, which tests/test_gpu_parity.py::test_paf_lines holds to the oracle; the device text must be the
same multiset of lines (the record order of a run is undefined, as in the reference), whatever the pieces, the slices, the first
capacity of the record buffer, the names, and the parts of the index."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import to_arrays

pytestmark = pytest.mark.gpu

PRESETS = {"ont": 0, "pb": 1}
FIXED_BOUND = 170      # PAF_FIXED_BOUND of csrc/paf_core.h


class Cfg:
    """One pair of read sets on the device and the model's lines for it."""

    def __init__(self, ctx, qseqs, qnames, tseqs, tnames, preset, dual):
        from lrge_amd import engine, paf
        self.ctx, self.preset, self.dual = ctx, PRESETS[preset], dual
        self.qnames, self.tnames = list(qnames), list(tnames)
        self.qlens, self.tlens = [len(s) for s in qseqs], [len(s) for s in tseqs]
        self.t_bases = sum(self.tlens)
        qr, tr = engine.name_ranks(qnames, tnames)
        qb, qo = to_arrays(qseqs)
        tb, to = to_arrays(tseqs)
        self.Qd, self.Td = ctx.upload(qb, qo, qr), ctx.upload(tb, to, tr)
        ix = engine.Index(ctx, self.Td, self.preset)
        self.chains = ix.chains(self.Qd, dual=dual)
        self.stats = ix.paf_stats(self.Qd)
        ix.free()
        self.model = self.lines_for(self.qnames, self.tnames)

    def lines_for(self, qnames, tnames):
        from lrge_amd import paf
        rl, ss, nk = self.stats
        return sorted((l + "\n").encode() for l in paf.paf_lines(self.chains, qnames, self.qlens, tnames, self.tlens, rl, ss, nk))

    def index(self, knobs=None, parts=1):
        from lrge_amd import engine
        if parts > 1:
            knobs.set("PART_BASES", str(self.t_bases // parts + 1))
        return engine.Index(self.ctx, self.Td, self.preset)

    def bound(self, qnames=None, tnames=None):
        return max(map(len, qnames or self.qnames)) + max(map(len, tnames or self.tnames)) + FIXED_BOUND


@pytest.fixture(scope="module")
def cfgs(ctx, edge_set, tiny_hifi):
    qseqs, qnames, tseqs, tnames = edge_set
    keep = [i for i, s in enumerate(qseqs) if len(s)]      # (an empty query is LRGE_ERR_MAP for every overlap call)
    qseqs, qnames = [qseqs[i] for i in keep], [qnames[i] for i in keep]
    hq = tiny_hifi.q.seqs()[:10] + qseqs[-10:], list(tiny_hifi.q.names[:10]) + qnames[-10:]      # the mix of test_paf_lines
    ht = tiny_hifi.t.seqs() + tseqs[-10:], list(tiny_hifi.t.names) + tnames[-10:]
    return {
        "edge-ont": Cfg(ctx, qseqs, qnames, tseqs, tnames, "ont", True),
        "edge-ont-ava": Cfg(ctx, tseqs, tnames, tseqs, tnames, "ont", False),
        "hifi-mix-pb": Cfg(ctx, hq[0], hq[1], ht[0], ht[1], "pb", True),
    }


def split_lines(text):
    assert text == b"" or text.endswith(b"\n")
    return sorted(l + b"\n" for l in text.split(b"\n")[:-1])


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("name", ["edge-ont", "edge-ont-ava", "hifi-mix-pb"])
def test_device_text_is_the_model(ctx, cfgs, knobs, name, parts):
    c = cfgs[name]
    ix = c.index(knobs, parts)
    text = ix.paf_text(c.Qd, c.qnames, c.tnames, dual=c.dual)
    st = ctx.last_paf_stats()
    n_parts = ctx.counters()["index_parts"]
    assert n_parts >= parts if parts > 1 else n_parts == 0      # (PART_BASES = total / 3 + 1: the cut falls between reads, so 3 or 4 parts)
    ix.free()
    got = split_lines(text)
    assert len(c.model) > 50 and len(got) == len(c.model)
    bad = [i for i, (a, b) in enumerate(zip(got, c.model)) if a != b]
    assert not bad, "first differing PAF line:\n%r\n%r" % (got[bad[0]], c.model[bad[0]])
    assert (st["lines"], st["bytes"], st["records"], st["unproven"], st["chain_runs"]) == (len(got), len(text), len(got), 0, 1)
    assert st["slices"] == st["pieces"] == 1
    if name == "hifi-mix-pb":
        assert any(b"dv:f:0." in l for l in got) and any(not l.endswith(b"rl:i:0\n") for l in got)


def test_pieces_and_slices(ctx, cfgs, knobs):
    c = cfgs["edge-ont"]
    ix = c.index()
    n = len(c.model)
    for piece, per_slice in [(1, 1), (5 * c.bound(), 5), (5 * c.bound() + c.bound() - 1, 5)]:
        knobs.set("PAF_PIECE_BYTES", str(piece))
        pieces = []
        ix.paf_text_to(pieces.append, c.Qd, c.qnames, c.tnames, dual=c.dual)
        st = ctx.last_paf_stats()
        assert all(p.endswith(b"\n") and p.count(b"\n") <= per_slice for p in pieces)
        assert [p.count(b"\n") for p in pieces[:-1]] == [per_slice] * (len(pieces) - 1)
        assert len(pieces) == -(-n // per_slice) == st["slices"] == st["pieces"]
        assert split_lines(b"".join(pieces)) == c.model
        assert (st["lines"], st["bytes"]) == (n, sum(map(len, pieces)))
    ix.free()


def test_a_small_first_capacity_runs_the_chains_twice(ctx, cfgs):
    c = cfgs["hifi-mix-pb"]
    ix = c.index()
    text = ix.paf_text(c.Qd, c.qnames, c.tnames, dual=c.dual, chain_hint=1)
    st = ctx.last_paf_stats()
    assert st["chain_runs"] == 2 and st["records"] == len(c.model) and split_lines(text) == c.model
    text = ix.paf_text(c.Qd, c.qnames, c.tnames, dual=c.dual, chain_hint=len(c.model))      # exactly enough: one run
    assert ctx.last_paf_stats()["chain_runs"] == 1 and split_lines(text) == c.model
    ix.free()


def renamed(names, lens, tag):
    out = []
    for i in range(len(names)):
        l = lens[i % len(lens)]
        stem = (b"%s%d_" % (tag, i))[:l]
        out.append(stem + bytes([ord("a") + (i + j) % 26 for j in range(l - len(stem))]))
    return out


@pytest.mark.parametrize("parts", [1, 3])
def test_long_and_awkward_names(ctx, cfgs, knobs, parts):
    c = cfgs["edge-ont"]
    lens = [1, 63, 64, 65, 255]
    qn, tn = renamed(c.qnames, lens, b"q"), renamed(c.tnames, lens[::-1], b"T")
    assert sorted(set(map(len, qn))) == lens and sorted(set(map(len, tn))) == lens
    model = c.lines_for(qn, tn)
    ix = c.index(knobs, parts)
    for piece in (1 << 26, 1):
        knobs.set("PAF_PIECE_BYTES", str(piece))
        assert split_lines(ix.paf_text(c.Qd, qn, tn, dual=c.dual)) == model
    ix.free()
    used = {len(l.split(b"\t")[0]) for l in model} | {len(l.split(b"\t")[5]) for l in model}
    assert used == set(lens)


def test_refusals_and_errors(ctx, cfgs, knobs):
    from lrge_amd import _ffi, engine
    c = cfgs["edge-ont"]
    ix = c.index()
    calls = []
    # an identifier of 1025 bytes: unproven, nothing delivered; 1024 is taken
    qn = list(c.qnames)
    qn[3] = b"x" * 1025
    with pytest.raises(engine.UnprovenInput):
        ix.paf_text_to(calls.append, c.Qd, qn, c.tnames)
    assert calls == [] and ctx.last_paf_stats()["lines"] == 0
    qn[3] = b"x" * 1024
    assert split_lines(ix.paf_text(c.Qd, qn, c.tnames)) == c.lines_for(qn, c.tnames)
    # a sink that fails on its second call
    knobs.set("PAF_PIECE_BYTES", "1")

    def failing(piece):
        calls.append(piece)
        return len(calls) < 2
    with pytest.raises(engine.LrgeHipError) as e:
        ix.paf_text_to(failing, c.Qd, c.qnames, c.tnames)
    assert e.value.code == _ffi.ERR_PAF_WRITE and len(calls) == 2 and "Error writing PAF file" in str(e.value)
    knobs.unset("PAF_PIECE_BYTES")
    # offsets that do not ascend: invalid, before any device work
    blob = b"".join(c.qnames)
    off = np.zeros(len(c.qnames) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in c.qnames], out=off[1:])
    off[2], off[3] = off[3], off[2]
    toff = np.zeros(len(c.tnames) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in c.tnames], out=toff[1:])
    hit = []
    cb = _ffi.GZIP_SINK(lambda u, p, n: hit.append(n) or 0)
    rc = ctx._lib.lrge_hip_paf_text(ctx.h, ix.h, c.Qd.h, 1, blob, off.ctypes.data, b"".join(c.tnames), toff.ctypes.data, 0, cb, None)
    assert rc == _ffi.ERR_INVALID and hit == []
    ix.free()
    # sets without an overlap: OK, the sink is never called
    rng = np.random.Generator(np.random.PCG64(5))
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 3000)) for _ in range(8)]
    names = [b"lonely%d" % i for i in range(8)]
    qr, tr = engine.name_ranks(names[:4], names[4:])
    Qd, Td = ctx.upload(*to_arrays(seqs[:4]), qr), ctx.upload(*to_arrays(seqs[4:]), tr)
    ix2 = engine.Index(ctx, Td, 0)
    calls.clear()
    ix2.paf_text_to(calls.append, Qd, names[:4], names[4:])
    st = ctx.last_paf_stats()
    assert calls == [] and (st["lines"], st["bytes"], st["pieces"], st["chain_runs"]) == (0, 0, 0, 1)
    ix2.free()


def test_other_entry_points_are_unchanged(ctx, cfgs):
    c = cfgs["hifi-mix-pb"]
    ix = c.index()

    def snapshot():
        ch = ix.chains(c.Qd, dual=c.dual)
        counts, has = ix.overlap_twoset(c.Qd)
        return sorted(map(tuple, ch.tolist())), [a.tolist() for a in ix.paf_stats(c.Qd)], counts.tolist(), has.tolist()
    before = snapshot()
    assert before[0] == sorted(map(tuple, c.chains.tolist())) and len(before[0]) > 50
    assert split_lines(ix.paf_text(c.Qd, c.qnames, c.tnames, dual=c.dual)) == c.model
    assert snapshot() == before
    ix.free()


def test_cli_gpu_paf_writes_the_same_file(tmp_path):
    """-C --gpu-paf and -C alone: the same multiset of lines in overlaps.paf and the same estimate, all-vs-all and two-set."""
    from lrge_amd import build as B, synth
    cli = B.build_cli()
    _, reads, _ = synth.make_config("tiny_ava")
    fa = tmp_path / "reads.fa"
    with open(fa, "wb") as fh:
        for n, s in zip(reads.names, reads.seqs()):
            fh.write(b">" + n + b" some description\n" + s + b"\n")
    for mode in (["-n", str(reads.n)], ["-T", "150", "-Q", "50", "-s", "1"]):
        outs = {}
        for flag in ([], ["--gpu-paf"]):
            d = tmp_path / ("%s%s" % (mode[0].strip("-"), "_gpu" if flag else "_host"))
            d.mkdir()
            r = subprocess.run([cli] + mode + ["-f", "-C", "-D", str(d)] + flag + [str(fa)], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr
            assert ("gpu-paf: device" in r.stderr) == bool(flag)
            outs[bool(flag)] = (r.stdout, sorted(open(d / "overlaps.paf", "rb").read().split(b"\n")))
        assert outs[True] == outs[False] and len(outs[True][1]) > 100
    # without -C the flag has no effect
    r = subprocess.run([cli, "-n", str(reads.n), "-f", "--gpu-paf", str(fa)], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0 and "gpu-paf" not in r.stderr and not (tmp_path / "overlaps.paf").exists()
