#!/usr/bin/env python
"""Records shared_names_plain_counters.json: the work counters of the calls of tests/test_gpu_shared_names.py::test_the_path_is_not_taken
(forward two-set against a partitioned index without a target name shared across parts), as the library in the CURRENT DIRECTORY's tree
gives them.  The committed file was recorded on the commit before names shared across parts were counted, so that the test holds every
later commit to launching, for such calls, exactly what that one launched.  Needs the GPU.

    cd <checkout of the commit to record> && python <this file> --out shared_names_plain_counters.json
"""
import argparse
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.getcwd())      # lrge_amd of the tree to record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "shared_names_plain_counters.json"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("shared_names_cases", os.path.join(os.path.dirname(HERE), "test_gpu_shared_names.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    from lrge_amd import engine, synth
    ctx = engine.Context(0)
    out = {}
    for preset, cfg in (("ont", "tiny_twoset"), ("pb", "tiny_hifi")):
        _, q, t = synth.make_config(cfg)
        got = T.plain_cases(ctx, q, t, T.PRESETS[preset])
        for case, (cn, counts, ref) in got.items():
            assert (counts == ref).all(), (preset, case)
        out[preset] = {case: cn for case, (cn, _, _) in got.items()}
    ctx.close()
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
