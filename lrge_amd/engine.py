"""Thin object wrappers over the C ABI: Context / SeqSet / Index.

The boundary mirrors liblrge's minimap2 wrapper (liblrge/src/minimap2/aligner.rs): an Index is
what AlignerWrapper::new builds (preset + dual + index over the target file), and the overlap
calls are the batched form of Aligner::map plus liblrge's counting shells.
"""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import LrgeHipError, Params, UnprovenInput


def name_ranks(*name_lists):
    """Lexicographic (strcmp) ranks over the union of several name lists; equal names share a rank.
    Returns one uint32 array per input list."""
    allnames = [n if isinstance(n, bytes) else n.encode() for lst in name_lists for n in lst]
    if not allnames:
        return [np.zeros(0, dtype=np.uint32) for _ in name_lists]
    arr = np.array(allnames, dtype=object)
    order = sorted(range(len(allnames)), key=lambda i: allnames[i])  # bytes compare == strcmp without NULs
    ranks = np.zeros(len(allnames), dtype=np.uint32)
    r = 0
    for j, i in enumerate(order):
        if j > 0 and allnames[i] != allnames[order[j - 1]]:
            r = j
        ranks[i] = r
    out, k = [], 0
    for lst in name_lists:
        out.append(ranks[k:k + len(lst)].copy())
        k += len(lst)
    return out


class Context:
    def __init__(self, device=0):
        self._lib = _ffi.lib()
        h = C.c_void_p()
        rc = self._lib.lrge_hip_ctx_create(device, C.byref(h))
        if rc != 0:
            raise LrgeHipError(rc, self._lib.lrge_hip_last_error(None).decode())
        self.h = h
        self.device = device

    def _check(self, rc):
        if rc != 0:
            raise LrgeHipError(rc, self._lib.lrge_hip_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self._lib.lrge_hip_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name, value):
        """Tuning / test option of this context; value None clears it.  The same names are
        read once from the environment (LRGE_HIP_<NAME>) when the context is created, except DEBUG_*."""
        self._check(self._lib.lrge_hip_ctx_set_option(self.h, name.encode(), None if value is None else str(value).encode()))

    def bgzf_inflate(self, data):
        """A BGZF buffer decompressed on the device (lrge_hip_bgzf_inflate); bytes in, bytes out.  Input that is not BGZF,
        or a damaged block, raises LrgeHipError with code ERR_PARSE."""
        data = bytes(data)
        n, total = C.c_uint64(), C.c_uint64()
        rc = self._lib.lrge_hip_bgzf_scan(data, len(data), C.byref(n), C.byref(total))
        if rc != 0:
            raise LrgeHipError(rc, self._lib.lrge_hip_last_error(None).decode())
        out = C.create_string_buffer(max(1, total.value))
        self._check(self._lib.lrge_hip_bgzf_inflate(self.h, data, len(data), out, total.value))
        return out.raw[:total.value]

    def _stream_inflate(self, fn, data, stat_names):
        """One round decoder's C entry `fn` over `data`, its rounds collected by a sink: (bytes, dict of its stats)."""
        data = bytes(data)
        parts = []

        def sink(_user, p, n):
            parts.append(C.string_at(p, n))
            return 0
        cb = _ffi.GZIP_SINK(sink)
        st = (C.c_uint64 * len(stat_names))()
        self._check(fn(self.h, data, len(data), cb, None, C.cast(st, C.c_void_p)))
        return b"".join(parts), dict(zip(stat_names, list(st)))

    def gzip_inflate(self, data, stats=False):
        """Any gzip buffer (plain, multi-member or BGZF) decompressed on the device (lrge_hip_gzip_inflate); bytes in, bytes
        out.  Damaged or trailing data raises LrgeHipError with code ERR_PARSE, a chunk beyond its slot ERR_TOO_MANY.
        stats=True returns (bytes, dict of lrge_hip_gzip_stats)."""
        out, st = self._stream_inflate(self._lib.lrge_hip_gzip_inflate, data, _ffi.GZIP_STAT_NAMES)
        return (out, st) if stats else out

    def bzip2_inflate(self, data):
        """A bzip2 buffer (one stream) decompressed on the device (lrge_hip_bzip2_inflate): bytes in, (bytes, dict of
        lrge_hip_bzip2_stats) out.  Input the device does not accept (damage, a second stream, trailing bytes, a randomised
        block) raises LrgeHipError with code ERR_PARSE."""
        return self._stream_inflate(self._lib.lrge_hip_bzip2_inflate, data, _ffi.BZIP2_STAT_NAMES)

    def zstd_inflate(self, data):
        """A Zstandard buffer (frames and skippable frames back to back) decompressed on the device (lrge_hip_zstd_inflate):
        bytes in, (bytes, dict of lrge_hip_zstd_stats) out.  Input the device does not accept (damage, a dictionary, a window
        above 2^27 bytes, trailing bytes) raises LrgeHipError with code ERR_PARSE; text above the device budget ERR_TOO_MANY."""
        return self._stream_inflate(self._lib.lrge_hip_zstd_inflate, data, _ffi.ZSTD_STAT_NAMES)

    def xz_inflate(self, data):
        """An .xz buffer (streams and stream padding back to back) decompressed on the device (lrge_hip_xz_inflate): bytes in,
        (bytes, dict of lrge_hip_xz_stats) out.  Input the device does not accept (damage, a filter other than LZMA2, a SHA-256
        check, trailing bytes, fewer blocks than option XZ_MIN_BLOCKS) raises LrgeHipError with code ERR_PARSE; a round's text
        above the device budget ERR_TOO_MANY."""
        return self._stream_inflate(self._lib.lrge_hip_xz_inflate, data, _ffi.XZ_STAT_NAMES)

    def rans_decode(self, streams, comp=None):
        """A batch of independent rANS streams decoded on the device (lrge_hip_rans_decode, the unit of the CRAM ingest).  streams:
        [(method, bytes, raw size)] (method 0: stored, 4: rANS 4x8, 5: rANS Nx16; the bytes are a CRAM block's body).  Returns
        ([output bytes per stream], [status per stream], dict of lrge_hip_cram_stats); status 16: the stream head was refused on
        the host, `rans_why` holds the first such reason."""
        body = bytearray()
        arr = (_ffi.RansStream * max(1, len(streams)))()
        for i, (method, data, raw) in enumerate(streams):
            arr[i] = _ffi.RansStream(len(body), len(data), int(raw), int(method), 0)
            body += data
        total = sum(int(r) for _, _, r in streams)
        out = C.create_string_buffer(max(1, total))
        st = (C.c_uint64 * len(_ffi.CRAM_STAT_NAMES))()
        self._check(self._lib.lrge_hip_rans_decode(self.h, bytes(body), len(body), arr, len(streams), out, total, C.cast(st, C.c_void_p)))
        self.rans_why = self._lib.lrge_hip_last_error(self.h).decode()
        raw, outs, o = out.raw, [], 0
        for _, _, r in streams:
            outs.append(raw[o:o + int(r)])
            o += int(r)
        return outs, [int(arr[i].status) for i in range(len(streams))], dict(zip(_ffi.CRAM_STAT_NAMES, [int(x) for x in st]))

    def open_reads(self, path_or_bytes, flags=_ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP):
        """A FASTA / FASTQ file (a path, or the bytes of the whole file) parsed on the device: plain, BGZF or any other gzip
        (| _ffi.GPU_INFLATE_BZIP2: bzip2 as well; | _ffi.GPU_INFLATE_ZSTD: Zstandard as well, resident unless | _ffi.GPU_INGEST_WINDOWED_ZSTD stands beside it and the windowed flag: then it passes through the windows too, DeviceReads.zstd_stats(); | _ffi.GPU_INFLATE_XZ: xz as well), by `flags` (lrge_hip_reads_open*); | _ffi.GPU_INGEST_BAM takes unaligned BAM as well, | _ffi.GPU_INGEST_SAM unaligned SAM, | _ffi.GPU_INGEST_CRAM (opt-in, implied by nothing) unaligned CRAM with its base blocks decoded on the device (DeviceReads.cram_stats); | _ffi.GPU_INGEST_WINDOWED lets FASTA / FASTQ text above option INGEST_WINDOW_BYTES pass through in windows with only the bases kept (DeviceReads.window_stats), and | _ffi.GPU_INGEST_WINDOWED_ALN beside it and the format's own flag does the same for unaligned BAM (its bases kept packed, 4 bits each) and SAM.  Returns a DeviceReads with names, lens and seqset().  Input the device does not
        prove raises UnprovenInput: read the file with the host readers (readio.load) instead."""
        return DeviceReads(self, path_or_bytes, flags)

    def census_reads(self, src, flags=_ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP):
        """The count pass of the sampled ingest (lrge_hip_reads_census*): the FASTA / FASTQ text of `src` (a path, or the bytes of
        the whole file) passes through the windows and is proven, nothing is kept.  Returns (records, sequence bases, text bytes,
        windows flushed); input the device does not prove raises UnprovenInput."""
        L = self._lib
        out = (C.c_uint64 * 4)()
        if isinstance(src, (bytes, bytearray, memoryview, np.ndarray)):
            buf = np.frombuffer(src, dtype=np.uint8) if not isinstance(src, np.ndarray) else np.ascontiguousarray(src, dtype=np.uint8)
            rc = L.lrge_hip_reads_census_mem(self.h, buf.ctypes.data if buf.size else None, buf.size, int(flags), C.byref(out))
        else:
            import os
            rc = L.lrge_hip_reads_census(self.h, os.fsencode(str(src)), int(flags), C.byref(out))
        if rc == _ffi.ERR_UNPROVEN:
            raise UnprovenInput(rc, L.lrge_hip_last_error(self.h).decode())
        self._check(rc)
        return tuple(int(x) for x in out)

    def open_reads_selected(self, src, sel, flags=_ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP):
        """The second pass of the sampled ingest (lrge_hip_reads_open_selected*): only records `sel` (strictly ascending ordinals
        in file order, 0-based) of the FASTA / FASTQ text of `src` are kept.  Returns a DeviceReads of len(sel) reads in file
        order, read j being record sel[j]; DeviceReads.select_stats() tells what the pass saw."""
        return DeviceReads(self, src, flags, sel)

    def census_map_reads(self, src, flags=_ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP):
        """census_reads that also leaves the seek map of the text (lrge_hip_reads_census_map*, option INGEST_SEEK_STRIDE_BYTES):
        returns (counts, ReadMap).  open_reads_mapped(src, map, sel) then brings only the runs that hold chosen reads."""
        L = self._lib
        out, h = (C.c_uint64 * 4)(), C.c_void_p()
        if isinstance(src, (bytes, bytearray, memoryview, np.ndarray)):
            buf = np.frombuffer(src, dtype=np.uint8) if not isinstance(src, np.ndarray) else np.ascontiguousarray(src, dtype=np.uint8)
            rc = L.lrge_hip_reads_census_map_mem(self.h, buf.ctypes.data if buf.size else None, buf.size, int(flags), C.byref(out), C.byref(h))
        else:
            import os
            rc = L.lrge_hip_reads_census_map(self.h, os.fsencode(str(src)), int(flags), C.byref(out), C.byref(h))
        if rc == _ffi.ERR_UNPROVEN:
            raise UnprovenInput(rc, L.lrge_hip_last_error(self.h).decode())
        self._check(rc)
        return tuple(int(x) for x in out), ReadMap(self, h)

    def last_stream_stats(self):
        """How the last open_reads / census_reads / open_reads_selected / census_map_reads of a path read its file
        (lrge_hip_last_stream_stats): (read calls issued, file bytes read, pinned host bytes held for file bytes at the peak, 1 if
        the pass streamed under _ffi.GPU_INGEST_STREAM -- pieces of option INGEST_STREAM_BYTES -- or 0 if it read the file whole)."""
        a = (C.c_uint64 * 4)()
        self._check(self._lib.lrge_hip_last_stream_stats(self.h, C.byref(a)))
        return tuple(int(x) for x in a)

    def open_reads_mapped(self, src, map, sel, flags=_ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP):
        """open_reads_selected of the input `map` was made of (lrge_hip_reads_open_mapped*): for plain and BGZF input only the runs
        that hold records `sel` are read, decoded and scanned; the DeviceReads is the one open_reads_selected gives, and
        DeviceReads.seek_stats() tells what was brought.  Input the map does not fit raises UnprovenInput."""
        return DeviceReads(self, src, flags, sel, map)

    def _name_ranks(self, blob, name_off, n_names, idx_lists):
        """lrge_hip_name_ranks over a table of identifiers; idx_lists None: every identifier in order, as one list"""
        if idx_lists is None:
            idx, n, sizes = None, n_names, [n_names]
        else:
            parts = [np.ascontiguousarray(ix, dtype=np.uint32).ravel() for ix in idx_lists]
            sizes = [int(p.size) for p in parts]
            idx = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
            n = int(idx.size)
        out = np.zeros(max(n, 1), dtype=np.uint32)
        st = (C.c_uint64 * 4)()
        rc = self._lib.lrge_hip_name_ranks(self.h, blob, name_off.ctypes.data, n_names, None if idx is None or not n else idx.ctypes.data, n,
                                           out.ctypes.data, C.cast(st, C.c_void_p))
        if rc == _ffi.ERR_UNPROVEN:
            raise UnprovenInput(rc, self._lib.lrge_hip_last_error(self.h).decode())
        self._check(rc)
        self.name_rank_stats = dict(zip(("sorts", "words", "distinct", "us"), [int(x) for x in st]))
        res, k = [], 0
        for m in sizes:
            res.append(out[k:k + m].copy())
            k += m
        return res

    def name_ranks(self, *name_lists):
        """engine.name_ranks on the device (lrge_hip_name_ranks): byte-wise ranks over the union of several name
        lists, equal names sharing a rank; one uint32 array per input list.  A name above option NAME_RANK_MAX_BYTES (default
        256) raises UnprovenInput: take engine.name_ranks.  `name_rank_stats` holds the call's sorts, words, distinct names and
        microseconds."""
        allnames = [n if isinstance(n, bytes) else n.encode() for lst in name_lists for n in lst]
        off = np.zeros(len(allnames) + 1, dtype=np.uint64)
        if allnames:
            np.cumsum(np.fromiter(map(len, allnames), dtype=np.uint64, count=len(allnames)), out=off[1:])
        (ranks,) = self._name_ranks(b"".join(allnames), off, len(allnames), None)
        out, k = [], 0
        for lst in name_lists:
            out.append(ranks[k:k + len(lst)].copy())
            k += len(lst)
        return out

    def set_timer_level(self, level):
        """0 = call total + chain stage only, 1 = every stage, 2 (default) = also every k_rs_scatter launch."""
        self._check(self._lib.lrge_hip_set_timer_level(self.h, int(level)))

    def timings(self):
        a = (C.c_float * len(_ffi.T_NAMES))()
        self._lib.lrge_hip_last_timings(self.h, C.byref(a))
        return dict(zip(_ffi.T_NAMES, [float(x) for x in a]))

    def counters(self):
        a = (C.c_uint64 * len(_ffi.C_NAMES))()
        self._lib.lrge_hip_last_counters(self.h, C.byref(a))
        return dict(zip(_ffi.C_NAMES, [int(x) for x in a]))

    def last_paf_stats(self):
        """The last Index.paf_text / paf_text_to of this context (lrge_hip_last_paf_stats): lines, bytes, chain_runs, slices, pieces,
        records (held on the device), unproven, format_us; and the host clock of its phases (lrge_hip_last_paf_phases)."""
        a, b = (C.c_uint64 * 8)(), (C.c_uint64 * 8)()
        self._check(self._lib.lrge_hip_last_paf_stats(self.h, C.byref(a)))
        self._check(self._lib.lrge_hip_last_paf_phases(self.h, C.byref(b)))
        d = dict(zip(_ffi.PAF_STAT_NAMES, [int(x) for x in a]))
        d.update(zip(_ffi.PAF_PHASE_NAMES, [int(x) for x in b]))
        return d

    def upload(self, bases, offsets, ranks=None, wait=True):
        """Read set -> 2-bit packed in HBM.  `bases`: numpy uint8 (pageable or pinned host memory, see host_alloc) or an
        int device pointer to ASCII already resident in HBM.  wait=False queues the transfer + pack on the copy stream
        and returns (lrge_hip_seqset_upload_async): later calls order themselves behind it on the device."""
        return SeqSet(self, bases, offsets, ranks, wait)

    def host_alloc(self, nbytes):
        """Pinned host buffer as a numpy uint8 array (lrge_hip_host_alloc): a DMA source without staging."""
        p = C.c_void_p()
        rc = self._lib.lrge_hip_host_alloc(int(nbytes), C.byref(p))
        if rc != 0:
            raise LrgeHipError(rc, self._lib.lrge_hip_last_error(None).decode())
        return PinnedBuffer(self._lib, p, int(nbytes))

    def estimates(self, counts, read_lens, avg_target_len, n_target_reads, overlap_thresh=100):
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        lens = np.ascontiguousarray(read_lens, dtype=np.uint32)
        out = np.zeros(max(counts.size, 1), dtype=np.float32)
        self._check(self._lib.lrge_hip_estimates(self.h, counts.ctypes.data, lens.ctypes.data, counts.size,
                                                 C.c_float(avg_target_len), int(n_target_reads), overlap_thresh,
                                                 out.ctypes.data))
        return out[:counts.size]


def median(estimates, finite=True, lower=None, upper=None):
    """estimate.rs:80-132 on the host side of the library."""
    v = np.ascontiguousarray(estimates, dtype=np.float32)
    out = (C.c_float * 3)()
    ok = (C.c_int * 3)()
    rc = _ffi.lib().lrge_hip_median(v.ctypes.data if v.size else None, v.size, int(finite),
                                    int(lower is not None), lower or 0.0, int(upper is not None), upper or 0.0,
                                    C.byref(out), C.byref(ok))
    if rc != 0:
        raise LrgeHipError(rc, "invalid quantile arguments")
    return tuple(np.float32(out[i]) if ok[i] else None for i in range(3))


class PinnedBuffer:
    """Pinned host memory owned by the library; `.array` is a numpy uint8 view of it."""

    def __init__(self, lib, ptr, nbytes):
        self._lib, self.ptr, self.nbytes = lib, ptr, nbytes
        self.array = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(max(nbytes, 1),))[:nbytes]

    def free(self):
        if getattr(self, "ptr", None):
            self.array = None
            self._lib.lrge_hip_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class SeqSet:
    def __init__(self, ctx, bases, offsets, ranks=None, wait=True):
        self.ctx = ctx
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.n = offsets.size - 1
        self._offsets, self._lens = offsets, None      # (lens: on first use -- 2 M reads cost 5 ms of host time per upload otherwise)
        if isinstance(bases, (int, np.integer)):          # device pointer to resident ASCII
            ptr, self._src = int(bases), None
        else:
            if isinstance(bases, PinnedBuffer):
                self._src, bases = bases, bases.array
            bases = np.ascontiguousarray(bases, dtype=np.uint8)
            ptr = bases.ctypes.data if bases.size else None
            self._src = (getattr(self, "_src", None), bases)   # an async upload reads the source until the set is consumed
        r = None if ranks is None else np.ascontiguousarray(ranks, dtype=np.uint32)
        h = C.c_void_p()
        fn = ctx._lib.lrge_hip_seqset_upload if wait else ctx._lib.lrge_hip_seqset_upload_async
        ctx._check(fn(ctx.h, ptr, offsets.ctypes.data, self.n, None if r is None else r.ctypes.data, C.byref(h)))
        self.h = h

    @property
    def lens(self):
        """read lengths (uint32), from the offsets the set was uploaded with"""
        if self._lens is None:
            self._lens = np.diff(self._offsets).astype(np.uint32)
        return self._lens

    def wait(self):
        self.ctx._check(self.ctx._lib.lrge_hip_seqset_wait(self.h))

    def free(self):
        if getattr(self, "h", None):
            self.ctx._lib.lrge_hip_seqset_free(self.h)     # (drains a pending upload before the source may go)
            self.h = None
        self._src = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def presketch(self, preset):
        """Hint (results unchanged): the next Index() built on this context sketches this set on a side stream beside its
        own sort and table passes; the next overlap call that streams the set uses it (lrge_hip_seqset_presketch)."""
        self.ctx._check(self.ctx._lib.lrge_hip_seqset_presketch(self.ctx.h, self.h, preset))

    def presketch_sharded(self, preset, comm):
        """Collective (every rank of `comm` holds the SAME set): this rank sketches its share of the reads, the minimizers are
        all-gathered, the next overlap call that streams the set uses them (lrge_hip_seqset_presketch_sharded)."""
        self.ctx._check(self.ctx._lib.lrge_hip_seqset_presketch_sharded(self.ctx.h, self.h, preset, comm.h))

    def sketch(self, preset):
        n = C.c_uint64()
        self.ctx._check(self.ctx._lib.lrge_hip_sketch_dump(self.ctx.h, self.h, preset, None, None, 0, C.byref(n)))
        x = np.zeros(max(n.value, 1), dtype=np.uint64)
        y = np.zeros(max(n.value, 1), dtype=np.uint64)
        self.ctx._check(self.ctx._lib.lrge_hip_sketch_dump(self.ctx.h, self.h, preset, x.ctypes.data, y.ctypes.data,
                                                           n.value, C.byref(n)))
        return x[:n.value], y[:n.value]


class ReadMap:
    """The seek map a census left of one input (lrge_hip_read_map, Context.census_map_reads): one point per cell of the text in
    which a record starts.  It belongs to no context and is freed with free() or with the object."""

    def __init__(self, ctx, h):
        self._lib, self.h = ctx._lib, h

    def stats(self):
        """(records, points, stride, text bytes)"""
        a = (C.c_uint64 * 4)()
        rc = self._lib.lrge_hip_read_map_stats(self.h, C.byref(a))
        if rc:
            raise _ffi.LrgeHipError(rc, "read_map_stats")
        return tuple(int(x) for x in a)

    def points(self):
        """[(ordinal, text offset, file offset of the BGZF block -- 0 for plain input)] of every point"""
        k = self.stats()[1]
        a = [np.zeros(max(1, k), dtype=np.uint64) for _ in range(3)]
        rc = self._lib.lrge_hip_read_map_points(self.h, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, k)
        if rc:
            raise _ffi.LrgeHipError(rc, "read_map_points")
        return list(zip(*(x[:k].tolist() for x in a)))

    def entries(self):
        """(entries, window bytes held, kind, spacing in force) of a gzip map; (entries, mark bytes held, 5, spacing) of a
        bzip2 map (section 29); (0, 0, kind, 0) of any other"""
        a = (C.c_uint64 * 4)()
        rc = self._lib.lrge_hip_read_map_entries(self.h, C.byref(a))
        if rc:
            raise _ffi.LrgeHipError(rc, "read_map_entries")
        return tuple(int(x) for x in a)

    def free(self):
        if self.h is not None:
            self._lib.lrge_hip_read_map_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceReads:
    """The reads of one input file resident in HBM as text (lrge_hip_reads): `names` (list of bytes) and `lens` (uint32) are
    on the host, the bases never are.  seqset(idx, ranks) is an ordinary SeqSet of the chosen reads."""

    def __init__(self, ctx, src, flags, sel=None, map=None):
        self.ctx, self.h = ctx, None
        h = C.c_void_p()
        L = ctx._lib
        if sel is not None:                                 # Context.open_reads_selected
            sel = np.ascontiguousarray(sel, dtype=np.uint32).ravel()
            sel_args = (sel.ctypes.data if sel.size else None, int(sel.size))
        if map is not None:                                 # Context.open_reads_mapped
            if sel is None:
                raise ValueError("a ReadMap needs a selection")
            if map.h is None:
                raise ValueError("the ReadMap was freed")
            sel_args = (map.h,) + sel_args
        if isinstance(src, (bytes, bytearray, memoryview, np.ndarray)):
            buf = np.frombuffer(src, dtype=np.uint8) if not isinstance(src, np.ndarray) else np.ascontiguousarray(src, dtype=np.uint8)
            if map is not None:
                rc = L.lrge_hip_reads_open_mapped_mem(ctx.h, buf.ctypes.data if buf.size else None, buf.size, int(flags), *sel_args, C.byref(h))
            elif sel is not None:
                rc = L.lrge_hip_reads_open_selected_mem(ctx.h, buf.ctypes.data if buf.size else None, buf.size, int(flags), *sel_args, C.byref(h))
            else:
                rc = L.lrge_hip_reads_open_mem(ctx.h, buf.ctypes.data if buf.size else None, buf.size, int(flags), C.byref(h))
        else:
            import os
            if map is not None:
                rc = L.lrge_hip_reads_open_mapped(ctx.h, os.fsencode(str(src)), int(flags), *sel_args, C.byref(h))
            elif sel is not None:
                rc = L.lrge_hip_reads_open_selected(ctx.h, os.fsencode(str(src)), int(flags), *sel_args, C.byref(h))
            else:
                rc = L.lrge_hip_reads_open(ctx.h, os.fsencode(str(src)), int(flags), C.byref(h))
        if rc == _ffi.ERR_UNPROVEN:
            raise UnprovenInput(rc, L.lrge_hip_last_error(ctx.h).decode())
        ctx._check(rc)
        self.h = h
        self.n = int(L.lrge_hip_reads_count(h))
        self.text_bytes = int(L.lrge_hip_reads_text_bytes(h))
        nb = int(L.lrge_hip_reads_name_bytes(h))
        self.lens = np.zeros(self.n, dtype=np.uint32)
        self.name_off = np.zeros(self.n + 1, dtype=np.uint64)
        blob = C.create_string_buffer(max(1, nb))
        ctx._check(L.lrge_hip_reads_table(h, self.lens.ctypes.data if self.n else None, self.name_off.ctypes.data, blob))
        self._blob = blob.raw[:nb]
        self._names = None

    @property
    def names(self):
        if self._names is None:
            o = self.name_off.tolist()
            self._names = [self._blob[o[i]:o[i + 1]] for i in range(self.n)]
        return self._names

    def timings(self):
        """milliseconds of the open call: text to HBM, record scan, identifiers and lengths to the host, total"""
        a = (C.c_float * 4)()
        self.ctx._check(self.ctx._lib.lrge_hip_reads_timings(self.h, C.byref(a)))
        return dict(zip(("text", "scan", "names", "total"), [float(x) for x in a]))

    @property
    def bam_stats(self):
        """the counts of the BAM record scan (lrge_hip_bam_stats) as a dict, summed over the windows of a windowed open; raises when the
        input was not scanned as BAM"""
        a = (C.c_uint64 * len(_ffi.BAM_STAT_NAMES))()
        self.ctx._check(self.ctx._lib.lrge_hip_reads_bam_stats(self.h, C.byref(a)))
        return dict(zip(_ffi.BAM_STAT_NAMES, [int(x) for x in a]))

    def cram_stats(self):
        """the counts of a handle opened from unaligned CRAM (lrge_hip_cram_stats) as a dict; raises when the input was not CRAM"""
        a = (C.c_uint64 * len(_ffi.CRAM_STAT_NAMES))()
        self.ctx._check(self.ctx._lib.lrge_hip_reads_cram_stats(self.h, C.byref(a)))
        return dict(zip(_ffi.CRAM_STAT_NAMES, [int(x) for x in a]))

    def window_stats(self):
        """(windows flushed -- 0: the text stayed resident --, bytes in the store: the bases, for BAM their packed bytes --, largest window
        in bytes, bytes carried over cuts)"""
        a = (C.c_uint64 * 4)()
        self.ctx._check(self.ctx._lib.lrge_hip_reads_window_stats(self.h, C.byref(a)))
        return tuple(int(x) for x in a)

    def select_stats(self):
        """(records seen, records kept, sequence bases seen, bases kept) of the pass behind Context.open_reads_selected; zeros for
        a handle of Context.open_reads"""
        a = (C.c_uint64 * 4)()
        self.ctx._check(self.ctx._lib.lrge_hip_reads_select_stats(self.h, C.byref(a)))
        return tuple(int(x) for x in a)

    def seek_stats(self):
        """(runs, text bytes brought, file bytes read, BGZF blocks decoded) of the pass behind Context.open_reads_mapped; zeros for
        a handle of every other open"""
        a = (C.c_uint64 * 4)()
        self.ctx._check(self.ctx._lib.lrge_hip_reads_seek_stats(self.h, C.byref(a)))
        return tuple(int(x) for x in a)

    def zstd_stats(self):
        """(rounds, largest history carried into a round, largest work text -- history plus round --, bytes of history moved) of the
        sliding Zstandard decode behind an open with GPU_INGEST_WINDOWED_ZSTD; zeros for a handle whose call did not slide"""
        a = (C.c_uint64 * 4)()
        self.ctx._check(self.ctx._lib.lrge_hip_reads_zstd_stats(self.h, C.byref(a)))
        return tuple(int(x) for x in a)

    def name_ranks(self, *idx_lists):
        """engine.name_ranks of the reads in idx_lists (each any order, repeats allowed) on the device, ranked together: one
        uint32 array per list (Context.name_ranks; from the identifier table as it came back, `names` is not built).  A selected
        identifier above option NAME_RANK_MAX_BYTES raises UnprovenInput."""
        return self.ctx._name_ranks(self._blob, self.name_off, self.n, idx_lists)

    def seqset(self, idx, ranks=None):
        """reads idx (any order, repeats allowed) as a SeqSet; ranks as Context.upload"""
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        r = None if ranks is None else np.ascontiguousarray(ranks, dtype=np.uint32)
        h = C.c_void_p()
        self.ctx._check(self.ctx._lib.lrge_hip_seqset_from_reads(self.ctx.h, self.h, idx.ctypes.data if idx.size else None, idx.size,
                                                                 None if r is None else r.ctypes.data, C.byref(h)))
        s = SeqSet.__new__(SeqSet)
        s.ctx, s.h, s.n, s._src = self.ctx, h, int(idx.size), None
        s._offsets, s._lens = None, self.lens[idx] if idx.size else np.zeros(0, dtype=np.uint32)
        return s

    def free(self):
        if getattr(self, "h", None):
            self.ctx._lib.lrge_hip_reads_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Index:
    """AlignerWrapper::new(target_file, threads, preset, dual) -- aligner.rs:310-328."""

    def __init__(self, ctx, targets, preset=_ffi.PRESET_AVA_ONT, streamed=None, comm=None, shard=None, tshard=False):
        """shard = (all_target_lens, all_target_ranks or None, shard_first): `targets` is this rank's contiguous share of the
        target reads and the build is the collective lrge_hip_index_build_sharded (the target sketch is sharded too).
        tshard (with comm): `targets` is this rank's share of the target reads and the index holds ALL of its entries, with the
        occurrence statistics of the whole target set (lrge_hip_index_build_tsharded): the caller maps ALL queries against it
        and sums the counts over the ranks."""
        self.ctx, self.targets, self.preset = ctx, targets, preset
        h = C.c_void_p()
        if tshard:
            self.streamed = None
            ctx._check(ctx._lib.lrge_hip_index_build_tsharded(ctx.h, targets.h, preset, comm.h, C.byref(h)))
            self.h = h
            self.build_timings = ctx.timings()
            self.build_counters = ctx.counters()
            a = (C.c_uint64 * 8)()
            ctx._lib.lrge_hip_last_shard_stats(ctx.h, C.byref(a))
            # (hashes_*: (key, count) pairs, one 8-byte word each; entries_*: the 16-byte minimizers a sharded presketch of the streamed
            # set moved just before this build -- lrge_hip_seqset_presketch_sharded -- else 0)
            self.shard_stats = dict(keyset_bytes=0, entries_sketched=0, entries_sent=int(a[2]), entries_recv=int(a[3]), hashes_sent=int(a[4]), hashes_recv=int(a[5]),
                                    entry_bytes=int(a[6]) & 0xFF or 8, entries_kept=0, hash_bytes=8)
            return
        if shard is not None:
            lens = np.ascontiguousarray(shard[0], dtype=np.uint32)
            ranks = None if shard[1] is None else np.ascontiguousarray(shard[1], dtype=np.uint32)
            self.streamed = streamed
            self.n_targets = lens.size
            ctx._check(ctx._lib.lrge_hip_index_build_sharded(ctx.h, lens.ctypes.data, None if ranks is None else ranks.ctypes.data, lens.size,
                                                             targets.h, int(shard[2]), preset, streamed.h, comm.h, C.byref(h)))
            self.h = h
            self.build_timings = ctx.timings()
            self.build_counters = ctx.counters()
            a = (C.c_uint64 * 8)()
            ctx._lib.lrge_hip_last_shard_stats(ctx.h, C.byref(a))
            self.shard_stats = dict(zip(["keyset_bytes", "entries_sketched", "entries_sent", "entries_recv", "hashes_sent", "hashes_recv",
                                         "entry_bytes", "entries_kept"], [int(x) for x in a]))
            self.shard_stats["hash_bytes"] = self.shard_stats["entry_bytes"] >> 8 or 8
            self.shard_stats["entry_bytes"] &= 0xFF
            return
        # streamed / comm: an index built for ONE streamed set, occurrence statistics still over all targets; with a
        # communicator every rank passes its own range of the streamed reads (lrge_hip_index_build_for)
        self.streamed = streamed
        if streamed is None and comm is None:
            ctx._check(ctx._lib.lrge_hip_index_build(ctx.h, targets.h, preset, C.byref(h)))
        else:
            ctx._check(ctx._lib.lrge_hip_index_build_for(ctx.h, targets.h, preset, None if streamed is None else streamed.h,
                                                         None if comm is None else comm.h, C.byref(h)))
        self.h = h
        self.build_timings = ctx.timings()
        self.build_counters = ctx.counters()

    def free(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):      # a closed context has already released everything the index held
                self.ctx._lib.lrge_hip_index_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def stats(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_int32()
        self.ctx._lib.lrge_hip_index_stats(self.h, C.byref(a), C.byref(b), C.byref(c))
        return dict(n_minimizers=a.value, n_keys=b.value, mid_occ=c.value)

    def dump(self):
        n = C.c_uint64()
        self.ctx._check(self.ctx._lib.lrge_hip_index_dump(self.ctx.h, self.h, None, None, 0, C.byref(n)))
        k = np.zeros(max(n.value, 1), dtype=np.uint64)
        p = np.zeros(max(n.value, 1), dtype=np.uint64)
        self.ctx._check(self.ctx._lib.lrge_hip_index_dump(self.ctx.h, self.h, k.ctypes.data, p.ctypes.data, n.value,
                                                          C.byref(n)))
        return k[:n.value], p[:n.value]

    def _params(self, remove_internal, ratio):
        return Params(int(bool(remove_internal)), float(ratio))

    def overlap_twoset(self, queries, remove_internal=False, max_overhang_ratio=0.2):
        counts = np.zeros(max(queries.n, 1), dtype=np.uint32)
        has = np.zeros(max(queries.n, 1), dtype=np.uint32)
        p = self._params(remove_internal, max_overhang_ratio)
        self.ctx._check(self.ctx._lib.lrge_hip_overlap_twoset(self.ctx.h, self.h, queries.h, C.byref(p),
                                                              counts.ctypes.data, has.ctypes.data))
        return counts[:queries.n], has[:queries.n]

    def overlap_twoset_tsharded(self, queries, comm, remove_internal=False, max_overhang_ratio=0.2):
        """Collective (every rank of `comm`, each with its own tshard=True index and the SAME queries): counts and has_mapping
        (0 / 1) of the whole job on every rank, a target name counted once per query whichever shards bear it
        (lrge_hip_overlap_twoset_tsharded; twoset.rs:286-317).  The all-reduce that closes the step is inside."""
        counts = np.zeros(max(queries.n, 1), dtype=np.uint32)
        has = np.zeros(max(queries.n, 1), dtype=np.uint32)
        p = self._params(remove_internal, max_overhang_ratio)
        self.ctx._check(self.ctx._lib.lrge_hip_overlap_twoset_tsharded(self.ctx.h, self.h, queries.h, C.byref(p), comm.h,
                                                                       counts.ctypes.data, has.ctypes.data))
        return counts[:queries.n], has[:queries.n]

    def overlap_inverse(self, streamed, remove_internal=False, max_overhang_ratio=0.2):
        counts = np.zeros(max(self.targets.n, 1), dtype=np.uint32)
        p = self._params(remove_internal, max_overhang_ratio)
        self.ctx._check(self.ctx._lib.lrge_hip_overlap_inverse(self.ctx.h, self.h, streamed.h, C.byref(p),
                                                               counts.ctypes.data))
        return counts[:self.targets.n]

    def overlap_ava(self, remove_internal=False, max_overhang_ratio=0.2, shard=None):
        """All-vs-all counts keyed by indexed read.  `shard`: a SeqSet holding a subset of the indexed reads (name
        ranks over the whole set) -> this shard's contribution; the sum over a partition is the full result."""
        counts = np.zeros(max(self.targets.n, 1), dtype=np.uint32)
        p = self._params(remove_internal, max_overhang_ratio)
        reads = self.targets if shard is None else shard
        self.ctx._check(self.ctx._lib.lrge_hip_overlap_ava(self.ctx.h, self.h, reads.h, C.byref(p),
                                                           counts.ctypes.data))
        return counts[:self.targets.n]

    def chains(self, queries, dual=True):
        n = C.c_uint64()
        self.ctx._check(self.ctx._lib.lrge_hip_chains(self.ctx.h, self.h, queries.h, int(dual), None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=_ffi.CHAIN)
        self.ctx._check(self.ctx._lib.lrge_hip_chains(self.ctx.h, self.h, queries.h, int(dual), out.ctypes.data,
                                                      n.value, C.byref(n)))
        return out[:n.value]

    def paf_stats(self, queries):
        """Per-query (rep_len, sum_span, n_kept): the rl tag and the ingredients of mm_est_err's avg_k."""
        n = max(queries.n, 1)
        rl = np.zeros(n, dtype=np.int32); ss = np.zeros(n, dtype=np.uint64); nk = np.zeros(n, dtype=np.uint32)
        self.ctx._check(self.ctx._lib.lrge_hip_paf_stats(self.ctx.h, self.h, queries.h, rl.ctypes.data, ss.ctypes.data,
                                                         nk.ctypes.data))
        return rl[:queries.n], ss[:queries.n], nk[:queries.n]

    def paf_text_to(self, write, queries, q_names, t_names, dual=True, chain_hint=0):
        """overlaps.paf formatted on the device (lrge_hip_paf_text): `write(bytes)` is called once per slice with
        whole lines -- those of paf.paf_lines over chains + paf_stats, each with its line feed, in the run's record order.  A falsy
        return of `write` other than None, or an exception in it, stops the call (ERR_PAF_WRITE; the exception is raised again).
        UnprovenInput, nothing written: an identifier above option PAF_NAME_MAX_BYTES, or a dv the device cannot prove -- take
        paf.paf_lines.  q_names / t_names: the identifiers of `queries` and of the indexed set (bytes or str)."""
        def blob(names):
            names = [n if isinstance(n, bytes) else n.encode() for n in names]
            off = np.zeros(len(names) + 1, dtype=np.uint64)
            if names:
                np.cumsum(np.fromiter(map(len, names), dtype=np.uint64, count=len(names)), out=off[1:])
            return b"".join(names), off
        if len(q_names) != queries.n or len(t_names) != self.targets.n:
            raise ValueError("paf_text: %d / %d names for %d queries and %d indexed reads" % (len(q_names), len(t_names), queries.n, self.targets.n))
        qb, qo = blob(q_names)
        tb, to = (qb, qo) if t_names is q_names else blob(t_names)
        failed = []

        def sink(_user, p, n):
            try:
                r = write(C.string_at(p, n))
            except BaseException as e:      # (an exception must not unwind through the C frames)
                failed.append(e)
                return 1
            return 0 if r is None or r else 1
        cb = _ffi.GZIP_SINK(sink)
        rc = self.ctx._lib.lrge_hip_paf_text(self.ctx.h, self.h, queries.h, int(bool(dual)), qb, qo.ctypes.data, tb, to.ctypes.data, int(chain_hint), cb, None)
        if failed:
            raise failed[0]
        if rc == _ffi.ERR_UNPROVEN:
            raise UnprovenInput(rc, self.ctx._lib.lrge_hip_last_error(self.ctx.h).decode())
        self.ctx._check(rc)

    def paf_text(self, queries, q_names, t_names, dual=True, chain_hint=0):
        """paf_text_to collected: the whole of overlaps.paf as bytes."""
        parts = []
        self.paf_text_to(parts.append, queries, q_names, t_names, dual, chain_hint)
        return b"".join(parts)

    def anchors(self, queries, q, dual=True):
        n = C.c_uint64()
        self.ctx._check(self.ctx._lib.lrge_hip_anchors_dump(self.ctx.h, self.h, queries.h, int(dual), q, None, None, 0,
                                                            C.byref(n)))
        x = np.zeros(max(n.value, 1), dtype=np.uint64)
        y = np.zeros(max(n.value, 1), dtype=np.uint64)
        self.ctx._check(self.ctx._lib.lrge_hip_anchors_dump(self.ctx.h, self.h, queries.h, int(dual), q, x.ctypes.data,
                                                            y.ctypes.data, n.value, C.byref(n)))
        return x[:n.value], y[:n.value]
