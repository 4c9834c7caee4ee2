"""Unaligned CRAM: the device open (lrge_hip_reads_open* | LRGE_GPU_INGEST_CRAM: host walk, base blocks decoded into HBM) against the
way to the same resident read set without the flag (lrge_hip_read_records on the host, then an upload of the bases), the decode
rate per block form (lrge_hip_rans_decode), and the block count from which the device wins.  Usage:
  python tools/cram_bench.py [--repeats 5] [--slice-kb 256] [--max-blocks 1024] [--sections files,forms] [--out profiles/cram_bench.json]

Files come from tests/cram_writer.py, whose Python encoder writes about 150 KB/s: one container of four distinct slices of
--slice-kb of bases each is encoded once per BA method (rANS 4x8 order 1, what CRAM 3.0 writers use for bases, and rANS Nx16 order 1,
CRAM 3.1) and repeated to 1, 2, 4, ... --max-blocks BA blocks; containers are independent, so the repeated file is a legal CRAM
whose reads repeat.  No third-party CRAM exists in this image.  Clock: from the file's bytes in memory (device) or on disk in the
page cache (host reader) to the read set resident on the device.  One warm-up of each, then `repeats` rounds that alternate the
sides in the same process; medians with ranges, and the stage times of lrge_hip_cram_stats (walk, decode)."""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RATE_FORMS = ["raw", "rans0", "rans1", "nx16_o0", "nx16_o1", "nx16_o0x32", "nx16_o1x32", "nx16_pack", "nx16_pack_o1", "nx16_packrle", "nx16_cat"]


def spread(v):
    return {"median_s": round(statistics.median(v), 5), "min_s": round(min(v), 5), "max_s": round(max(v), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slice-kb", type=int, default=256)
    ap.add_argument("--rate-kb", type=int, default=128)
    ap.add_argument("--rate-blocks", type=int, default=1024)
    ap.add_argument("--max-blocks", type=int, default=1024)
    ap.add_argument("--sections", default="files,forms")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cram_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import cram_writer as CW
    from lrge_amd import _ffi, engine
    rng = np.random.Generator(np.random.PCG64(7))
    read_len, per_slice = 8192, max(1, a.slice_kb * 1024 // 8192)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    reads = [(b"bench/%d" % i, bytes(rng.choice(acgt, read_len))) for i in range(4 * per_slice)]
    hdr = b"@HD\tVN:1.6\tSO:unsorted\n"
    head = 26 + len(CW.container(0, 0, 0, 0, 0, 0, [CW.block("raw", 0, 0, struct.pack("<i", len(hdr)) + hdr)], [0]))
    eof = CW.container(-1, 4542278, 0, 0, 0, 0, [CW.block("raw", 1, 0, b"\x01\x00\x01\x00\x01\x00")], [])
    ctx = engine.Context(0)
    ctx.set_option("CRAM_MIN_BLOCKS", "0")
    flags = _ffi.GPU_INFLATE_BGZF | _ffi.GPU_INFLATE_GZIP | _ffi.GPU_INGEST_CRAM
    L = _ffi.lib()
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64)
    L.lrge_hip_read_records.argtypes = [C.c_char_p, CB, C.c_void_p, C.c_char_p, C.c_uint64]
    out = {"repeats": a.repeats, "slice_bytes": per_slice * read_len, "read_len": read_len, "files": {}, "forms": {}}
    tmp = tempfile.mkdtemp()

    def host_way(path):
        """lrge_hip_read_records, then the upload of the bases: the parent commit's way to a resident read set"""
        t = time.perf_counter()
        seqs = []
        cb = CB(lambda u, n, nl, b, bl: seqs.append(C.string_at(b, bl)))
        err = C.create_string_buffer(512)
        assert L.lrge_hip_read_records(os.fsencode(path), cb, None, err, 512) == 0, err.value
        off = np.zeros(len(seqs) + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in seqs], out=off[1:])
        S = ctx.upload(np.frombuffer(b"".join(seqs), dtype=np.uint8), off)
        t = time.perf_counter() - t
        n = S.n
        S.free()
        return t, n

    def dev_way(data):
        t = time.perf_counter()
        dr = ctx.open_reads(data, flags)
        S = dr.seqset(np.arange(dr.n, dtype=np.uint32))
        t = time.perf_counter() - t
        st, n = dr.cram_stats(), S.n
        S.free(); dr.free()
        return t, n, st

    for method, minor in (("rans1", 0), ("nx16_o1", 1)) if "files" in a.sections else ():
        t0 = time.perf_counter()
        one = CW.write_cram(reads, method="gzip", slices_per_container=4, records_per_slice=per_slice, minor=minor, with_quality=False, with_tags=False, method_for={"BA": method})
        body = one[head:len(one) - len(eof)]
        print("%s: one container of 4 slices encoded in %.1f s, %d bytes" % (method, time.perf_counter() - t0, len(body)), flush=True)
        k = 4
        while k <= a.max_blocks:
            data = one[:head] + body * (k // 4) + eof
            path = os.path.join(tmp, "bench.cram")
            with open(path, "wb") as fh:
                fh.write(data)
            n_ref = host_way(path)[1]
            assert dev_way(data)[1] == n_ref == len(reads) * (k // 4)
            host, dev, stages = [], [], []
            for r in range(a.repeats):
                host.append(host_way(path)[0])
                t, _, st = dev_way(data)
                dev.append(t); stages.append(st)
            med = lambda key: round(statistics.median(s[key] for s in stages) / 1000.0, 3)
            row = {"blocks": k, "file_bytes": len(data), "bases": stages[-1]["raw_bytes"], "ba_comp_bytes": stages[-1]["comp_bytes"], "host_read_records_plus_upload": spread(host),
                   "device_open_plus_gather": spread(dev), "host_over_device": round(statistics.median(host) / statistics.median(dev), 3),
                   "stages_ms": {"walk": med("walk_us"), "decode": med("decode_us")}, "rounds": stages[-1]["rounds"],
                   "decode_mb_per_s": round(stages[-1]["raw_bytes"] / max(1.0, statistics.median(s["decode_us"] for s in stages)), 1)}
            out["files"]["%s_%d_blocks" % (method, k)] = row
            print(method, json.dumps(row), flush=True)
            k *= 2
    # the rate per block form: --rate-blocks copies of one block of --rate-kb in one batch (one launch), the decode time from the stats
    plain = bytes(rng.choice(acgt, a.rate_kb * 1024))
    for form in RATE_FORMS if "forms" in a.sections else ():
        body = CW.compress(plain, form)
        items = [(CW.METHODS[form], body, len(plain))] * a.rate_blocks
        outs, status, st = ctx.rans_decode(items[:2])
        assert status == [0, 0] and outs[0] == plain, form
        us = []
        for r in range(a.repeats + 1):
            _, status, st = ctx.rans_decode(items)
            assert not any(status)
            us.append(st["decode_us"])
        us = us[1:]
        m = statistics.median(us)
        out["forms"][form] = {"block_bytes": len(plain), "comp_bytes": len(body), "blocks": a.rate_blocks, "decode_us": {"median": m, "min": min(us), "max": max(us)},
                              "mb_per_s_all_blocks": round(len(plain) * a.rate_blocks / m, 1), "mb_per_s_one_block_alone": None}
        _, _, st1 = ctx.rans_decode(items[:1])
        one_us = []
        for r in range(a.repeats):
            one_us.append(ctx.rans_decode(items[:1])[2]["decode_us"])
        out["forms"][form]["mb_per_s_one_block_alone"] = round(len(plain) / statistics.median(one_us), 2)
        print(form, json.dumps(out["forms"][form]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
