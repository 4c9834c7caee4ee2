"""The deflate decoders on legal streams that zlib's encoder never writes (tests/deflate_corpus.py, made by the spec-only
writer tests/deflate_writer.py), without a GPU: the host twins of k_inflate and of the speculative gzip decode against zlib's
inflate, which decides the bytes and accept / reject alike; the finder's property over the writer's files; derandomised
hypothesis streams through both twins; a guard that the corpus really holds what it is for."""
import ctypes as C
import random
import time

import pytest
from hypothesis import given, settings, strategies as st

import bgzf_writer as W
import deflate_corpus as K
from test_bgzf_twin import twin, twin_bgzf  # noqa: F401  (twin: fixture)
from test_gzip_twin import CHUNKS, gtwin, run  # noqa: F401  (gtwin: fixture)


def twin_raw(L, raw, cap):
    out = C.create_string_buffer(max(1, cap))
    rc = L.inflate_twin_raw(raw, len(raw), out, cap)
    return rc, out.raw[:cap]


def test_corpus_is_not_vacuous():
    raw, gz = K.raw_cases(), K.gzip_cases()
    assert K.STATS["max_lit_len"] == 15 and K.STATS["max_dist_len"] == 15
    assert K.STATS["stored_align"] == set(range(8))
    assert K.STATS["len258"] == {"285", "284+31"}
    rejected = [c.name for c in raw if c.expected is None] + [n for n, _, e in gz[len(raw):] if e is None]
    accepted = [c.name for c in raw if c.expected is not None]
    assert len(rejected) >= 30 and len(accepted) >= 40, (len(rejected), len(accepted))
    assert K.STATS["blocks"] > 8000
    assert sum(1 for _, _, e in K.bgzf_cases() if e is None) >= 25
    assert len(K.DENSE) <= 3 and all(n in K.BY_NAME for n in K.DENSE)
    assert max(len(c.raw) for c in raw) < 1 << 20


def test_raw_cases_twin_equals_zlib(twin):   # noqa: F811
    for c in K.raw_cases():
        if len(c.claimed) > 65536 and c.expected is None:
            continue
        t0 = time.perf_counter()
        rc, out = twin_raw(twin, c.raw, len(c.claimed))
        assert time.perf_counter() - t0 < 5.0, c.name
        if c.expected is None:
            assert rc != 0, "zlib rejects %s, the twin decodes it" % c.name
        else:
            assert rc == 0, (c.name, rc)
            assert out == c.expected, c.name


def test_bgzf_cases_twin_equals_zlib(twin):   # noqa: F811
    cases = K.bgzf_cases()
    for name, block, exp in cases:
        rc, out, _ = twin_bgzf(twin, block + W.EOF_BLOCK)
        if exp is None:
            assert rc > 0, "zlib rejects %s, the twin decodes it" % name
        else:
            assert rc == 0 and out == exp, (name, rc)
    # the blocks of every case in one file: statuses are per block, the first bad block is the one reported
    good = [(b, e) for _, b, e in cases if e is not None]
    f = b"".join(b for b, _ in good) + W.EOF_BLOCK
    rc, out, _ = twin_bgzf(twin, f)
    assert rc == 0 and out == b"".join(e for _, e in good)
    for k, (name, block, exp) in enumerate(cases):
        if exp is None:
            head = b"".join(b for b, _ in good[:k % len(good)])
            rc, _, bad = twin_bgzf(twin, head + block + good[0][0] + W.EOF_BLOCK)
            assert rc > 0 and bad == len(head), name
    for name, data, off in K.bgzf_reach_files():
        rc, _, bad = twin_bgzf(twin, data)
        assert rc > 0 and bad == off, name


@pytest.mark.parametrize("chunk", CHUNKS)
def test_gzip_cases_twin_equals_zlib(gtwin, chunk):   # noqa: F811
    for name, data, exp in K.gzip_cases():
        t0 = time.perf_counter()
        rc, out, stats = run(gtwin, data, chunk, rnd=max(4 * chunk, 1 << 16), ratio=64)
        assert time.perf_counter() - t0 < 20.0, name
        if exp is None:
            assert rc > 0, "zlib rejects %s, the twin ends with %d" % (name, rc)
            continue
        if rc == -1 and name in K.DENSE:
            continue
        assert rc == 0, (name, chunk, rc, stats)
        assert out == exp, (name, chunk)


def test_gzip_cases_small_rounds(gtwin):   # noqa: F811
    """512-byte chunks in 8 KiB rounds (what the device test runs): the reference into an earlier member is refused when the
    member header lies in an earlier round, and the provenance case resolves its markers through hundreds of windows"""
    for name, data, exp in K.gzip_cases():
        rc, out, stats = run(gtwin, data, 512, rnd=8192, ratio=64)
        if exp is None:
            assert rc > 0, "zlib rejects %s, the twin ends with %d" % (name, rc)
        elif not (rc == -1 and name in K.DENSE):
            assert rc == 0 and out == exp, (name, rc, stats)
        if name == "provenance_chains_of_distance_32768":
            assert stats["speculative"] > 100, stats
        if name.startswith("member_reaches_into_previous_member"):
            assert rc == 14, (name, rc)                      # GZ_E_MARKER: the chunk could not know, the window check did


def test_writer_fastq_files(twin, gtwin):   # noqa: F811
    """the FASTQ files of the device ingest test: both twins decode them, the slots suffice, zlib rejects the bad one"""
    for name, (data, fq) in K.fastq_files().items():
        assert K.zlib_gzip(data) == fq, name
        if name.startswith("bgzf"):
            assert twin_bgzf(twin, data)[:2] == (0, fq), name
        for chunk, ratio in K.SLOTS:
            assert K.max_piece_output(data, chunk) <= ratio * chunk, (name, chunk, ratio)
        for chunk, rnd in ((512, 8192), (512 << 10, 256 << 20)):
            rc, out, _ = run(gtwin, data, chunk, rnd, ratio=64 if chunk == 512 else 8)
            assert rc == 0 and out == fq, (name, chunk, rc)
    bad = K.fastq_rejected()
    assert K.zlib_gzip(bad) is None
    assert run(gtwin, bad, 512, 8192, 64)[0] > 0 and run(gtwin, bad)[0] > 0


def test_finder_property_over_writer_files(gtwin):   # noqa: F811
    """test_gzip_twin.py::test_finder_property over the writer's files: on each chunk the candidate is never past the first
    true member-header / canonical stored / dynamic boundary at or after the chunk's start.  A legal non-final dynamic header
    that inf_dynamic accepts and gz_is_dynamic refuses would show here as a candidate past a true boundary."""
    checked = 0
    names = ["lit_walk_eob15", "lit_walk_eob1", "precode_all_19_symbols_7_bits_hclen19", "clen_16_and_18_runs_span_lit_dist_boundary",
             "clen_header_encodings_vary", "dynamic_only_eob_between_data", "stored_len0_midstream_and_len65535",
             "stored_at_8_alignments_pad_zero", "stored_at_8_alignments_pad_ones", "stored_at_8_alignments_pad_random",
             "stored_payload_is_a_gzip_member", "5000_tiny_blocks_types_alternate", "runs_of_1000_empty_blocks",
             "multi_member_writer_made_some_empty", "multi_member_80_empty_members", "same_reference_within_one_member_far"]
    files = {n: d for n, d, e in K.gzip_cases() if e is not None}
    kinds = set()
    for name in names:
        f = files[name]
        cap = 200000
        bits = (C.c_uint32 * cap)()
        kind = (C.c_uint32 * cap)()
        nb = gtwin.gzip_twin_boundaries(f, len(f), bits, kind, cap)
        assert 0 < nb < cap, (name, nb)
        targets = sorted(bits[i] for i in range(nb) if kind[i] in (1, 2, 3))
        kinds |= {kind[i] for i in range(nb)}
        # every true non-final dynamic header is one the finder's predicate accepts
        for i in range(nb):
            if kind[i] == 3:
                assert gtwin.gzip_twin_find(f, len(f), bits[i], bits[i] + 1) == bits[i], (name, bits[i])
        import bisect
        for chunk in (512, 4096):
            for c0 in range(chunk, len(f), chunk):
                j = bisect.bisect_left(targets, 8 * c0)
                if j == len(targets):
                    continue
                cand = gtwin.gzip_twin_find(f, len(f), 8 * c0, min(8 * len(f), targets[j] + 1))
                assert cand != 0xFFFFFFFF and cand <= targets[j], (name, chunk, c0, cand, targets[j])
                checked += 1
    assert checked > 300 and kinds == {0, 1, 2, 3}


@settings(derandomize=True, max_examples=250, deadline=None, database=None)
@given(st.integers(0, 2 ** 32 - 1), st.sampled_from([20, 300, 2000]))
def test_property_streams_both_twins(twin, gtwin, seed, max_tokens):   # noqa: F811
    raw, plain, _ = K.random_stream(random.Random(seed), max_tokens)
    assert K.zlib_raw(raw) == plain
    rc, out = twin_raw(twin, raw, len(plain))
    assert rc == 0 and out == plain
    if K.bgzf_fits(K.Case("p", raw, plain, plain)):
        rc, out, _ = twin_bgzf(twin, W.bgzf_block(plain, comp=raw) + W.EOF_BLOCK)
        assert rc == 0 and out == plain
    gz = K.member(raw, plain)
    for chunk in (256, 512):
        if K.max_piece_output(gz, chunk) > 64 * chunk:
            continue                                   # (denser than the slot: TOO_MANY is the documented answer)
        rc, out, _ = run(gtwin, gz + gz, chunk, rnd=4096, ratio=64)
        assert rc == 0 and out == plain + plain, (seed, chunk, rc)
