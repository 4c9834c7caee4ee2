"""Unaligned SAM through the windows of the windowed ingest without a GPU (lrge_amd/csrc/fx_window.h): the
host twin runs the window driver over its passes (sam_twin_windowed) with the window and the appended piece as parameters,
against the host parser (lrge_hip_read_records) on the same bytes.  A window that is not the last is cut directly behind its last
line feed; a windowed scan gives the host's records or the unproven verdict, never other records."""
import ctypes as C

import pytest

import sam_corpus as S
from test_sam_twin import OK, UNPROVEN, FxRec, host_records, load_twin, twin_records

WINDOWS = [64, 257, 3001, 20000]


@pytest.fixture(scope="module")
def twin():
    L = load_twin()
    L.sam_twin_windowed.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64]
    L.sam_twin_windowed_count.restype = C.c_uint64
    L.sam_twin_windowed_table.argtypes = [C.c_void_p]
    L.sam_twin_windowed_stats.argtypes = [C.POINTER(C.c_uint64 * 4)]
    L.sam_twin_windowed_store.argtypes = [C.c_char_p]
    L.sam_twin_windowed_store.restype = C.c_uint64
    L.sam_twin_windowed_seq.argtypes = [C.c_uint64, C.c_char_p]
    L.sam_twin_windowed_seq.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """text -> (rc, [(name, sequence)], message) of the host parser, computed once per text"""
    d = tmp_path_factory.mktemp("sam_window_host")
    seen = {}

    def run(text):
        if text not in seen:
            seen[text] = host_records(d, text)
        return seen[text]
    return run


def windowed(L, data, window, piece):
    """(verdict, [(name, sequence)], (windows, store bytes, largest window, carried))"""
    rc = L.sam_twin_windowed(data, len(data), window, piece)
    if rc != OK:
        assert L.sam_twin_windowed_count() == 0             # (a refused call keeps no record of an earlier window)
        return rc, None, None
    n = L.sam_twin_windowed_count()
    tab = (FxRec * max(1, n))()
    L.sam_twin_windowed_table(tab)
    st = (C.c_uint64 * 4)()
    L.sam_twin_windowed_stats(C.byref(st))
    store = C.create_string_buffer(max(1, L.sam_twin_windowed_store(None)))
    n_store = L.sam_twin_windowed_store(store)
    out, at = [], 0
    buf = C.create_string_buffer(max(1, max((tab[i].seq_len for i in range(n)), default=0)))
    for i in range(n):
        r = tab[i]
        assert r.name_off + r.name_len <= len(data) and r.seq_off == at and r.seq_span == r.seq_len       # dense, in file order
        assert L.sam_twin_windowed_seq(i, buf) == r.seq_len
        assert buf.raw[:r.seq_len] == store.raw[at:at + r.seq_len]
        out.append((data[r.name_off:r.name_off + r.name_len], buf.raw[:r.seq_len]))
        at += r.seq_len
    assert n_store == at and st[1] == (at if st[0] else 0)
    return rc, out, tuple(int(x) for x in st)


def test_corpus_equals_host_parser(twin, host):
    """every well-formed case at every window and piece: proven, with the host's records; zero fall-backs"""
    n_rec = n_windowed = 0
    for name, data in S.well_formed():
        rc_h, rec_h, msg = host(data)
        assert rc_h == 0, (name, msg)
        for window in WINDOWS:
            for piece in sorted({1, 61, window, max(1, len(data))}):
                rc, rec, st = windowed(twin, data, window, piece)
                assert rc == OK, (name, window, piece, rc)
                assert rec == rec_h, (name, window, piece)
                text_bytes = len(data)
                assert st[2] <= text_bytes and st[1] <= text_bytes
                n_rec += len(rec)
                n_windowed += st[0] > 1
    # (not vacuous: all but the header-only cases are cut at least once at the two small windows and the three small pieces)
    assert n_rec > 40000 and n_windowed > 200


def test_unproven_list(twin):
    """what the resident scan leaves to the host stays unproven at every window and piece"""
    for name, data, _ in S.unproven():
        for window in [4, 17] + WINDOWS:
            for piece in (1, 61, window):
                assert twin.sam_twin_windowed(data, len(data), window, piece) == UNPROVEN, (name, window, piece)
                assert twin.sam_twin_windowed_count() == 0


def every_window(twin, host, data, what):
    n_multi = 0
    for window in range(4, len(data) + 2):
        rc, rec, st = windowed(twin, data, window, 1)
        assert rc == OK and rec == host(data)[1], (what, window)
        n_multi += st[0] > 1
    return n_multi


def test_crlf_cut_never_between_cr_and_lf(twin, host):
    """CRLF text with one byte appended per step: blocks end between the CR and the LF of every line, the cut lies behind the LF"""
    lines = [S.rec(b"r%d" % i, b"ACGT" * (1 + i % 3), eol=b"\r\n") for i in range(6)]
    data = S.HD.replace(b"\n", b"\r\n") + b"".join(lines)
    assert every_window(twin, host, data, "crlf") > 100
    assert every_window(twin, host, data + b"\r", "crlf and a final CR line") > 100


def test_no_final_line_feed(twin, host):
    lines = [S.rec(b"r%d" % i, b"ACGT" * (1 + i % 3)) for i in range(6)]
    data = S.sam(lines)[:-1]
    assert every_window(twin, host, data, "no final lf") > 100
    data = S.sam(lines[:5] + [S.rec(b"last", b"GGCC", qual=b"", eol=b"")])
    assert every_window(twin, host, data, "no final lf, empty quality") > 100


def test_co_and_empty_lines_at_a_cut(twin, host):
    """header lines, @CO and empty lines are skipped wherever they stand: a cut behind any of them"""
    lines = []
    for i in range(6):
        lines += [S.rec(b"r%d" % i, b"ACGT" * (1 + i % 3))] + [b"@CO\tbetween %d\n" % i, b"\n", b"\n\n@CO\n", b"@\n", b"\r\n", b"@HD\tagain\n"][i:i + 1]
    data = S.sam(lines, S.HD + b"\n")
    assert len(host(data)[1]) == 6
    assert every_window(twin, host, data, "co and empty lines") > 100


def test_a_read_named_at_x(twin, host):
    """a record line whose name starts with '@' is skipped by host and device alike, in any window"""
    lines = [S.rec(b"a", b"ACGT"), S.rec(b"@x", b"GGGG"), S.rec(b"b", b"TT"), S.rec(b"@HD", b"AC"), S.rec(b"c", b"CA")]
    data = S.sam(lines)
    assert [n for n, _ in host(data)[1]] == [b"a", b"b", b"c"]
    assert every_window(twin, host, data, "@x") > 100


def test_a_200_kb_record_across_windows_of_64(twin, host):
    """no cut inside a line: the block grows, doubling, until the line feed behind the record is there"""
    data = dict(S.well_formed())["long_200k"]
    for piece in (61, 4096):
        rc, rec, st = windowed(twin, data, 64, piece)
        assert rc == OK and rec == host(data)[1] and max(len(s) for _, s in rec) == 200000
        assert st[0] >= 2 and st[2] > 200000, st


def test_a_later_window_whose_first_line_starts_hd(twin, host):
    """the sniff belongs to the first window: a read named HD1 starts a later one, which is SAM by the run and not by its bytes"""
    first = S.HD + S.rec(b"r0", b"ACGT")
    data = first + S.rec(b"HD1", b"AC") + S.rec(b"SQ2", b"GGTT") + S.rec(b"RG3", b"T")
    rc, rec, st = windowed(twin, data, len(first), 1)
    assert rc == OK and st[0] >= 3 and [n for n, _ in rec] == [b"r0", b"HD1", b"SQ2", b"RG3"] and rec == host(data)[1]
    assert every_window(twin, host, data, "HD in a later window") > 100
    # without the magic in front the text is not SAM to the host's sniff either: unproven at every window
    for window in (4, 16, 64, 1000):
        assert twin.sam_twin_windowed(data[len(S.HD):], len(data) - len(S.HD), window, 1) == UNPROVEN


def test_mapped_record_in_a_later_window(twin, host):
    data = dict((n, d) for n, d, _ in S.unproven())["mapped_last_of_100"]
    assert twin.sam_twin_windowed(data, len(data), 257, 257) == UNPROVEN
    assert twin.sam_twin_windowed_count() == 0 and twin.sam_twin_windowed_store(None) == 0


def test_resident_equivalence(twin):
    """a window larger than the text: nothing is flushed, and the records are those of the resident twin"""
    for name, data in S.well_formed():
        rc, rec, st = windowed(twin, data, len(data) + 1, 61)
        assert rc == OK and st == (0, 0, 0, 0), name
        assert (rc, rec) == twin_records(twin, data), name


def test_arguments(twin):
    assert twin.sam_twin_windowed(S.HD, len(S.HD), 64, 0) == -1                 # a piece has bytes
