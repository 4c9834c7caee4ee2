"""Build liblrge_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_DIR = os.path.join(_HERE, "_lib")
LIB_PATH = os.path.join(LIB_DIR, "liblrge_hip.so")
HOST_LIB_PATH = os.path.join(LIB_DIR, "liblrge_host.so")

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
               # comput_sc / per_read_estimate / quantiles are f32 with one rounding per operation
               "-ffp-contract=off", "-Wall", "-Wno-unused-function"]


def _newest(paths):
    return max(os.path.getmtime(p) for p in paths)


def _sources():
    out = []
    for root, _, files in os.walk(CSRC):
        out += [os.path.join(root, f) for f in files]
    out.append(os.path.join(os.path.dirname(_HERE), "include", "lrge_hip.h"))
    out.append(os.path.join(os.path.dirname(_HERE), "include", "lrge_rand.hpp"))
    out.append(os.path.join(os.path.dirname(_HERE), "include", "lrge_io.hpp"))
    out.append(os.path.join(os.path.dirname(_HERE), "include", "lrge_cram.hpp"))
    return out


def build_lib(force=False, verbose=False):
    os.makedirs(LIB_DIR, exist_ok=True)
    if not force and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= _newest(_sources()):
        return LIB_PATH
    cmd = ["hipcc"] + HIPCC_FLAGS + ["-o", LIB_PATH, os.path.join(CSRC, "lrge_hip.hip"), "-lz", "-ldl"]      # (zlib: the host-side readers of include/lrge_io.hpp)
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB_PATH


TWIN_PATH = os.path.join(LIB_DIR, "liblrge_inflate_twin.so")
GZIP_TWIN_PATH = os.path.join(LIB_DIR, "liblrge_gzip_twin.so")
FASTX_TWIN_PATH = os.path.join(LIB_DIR, "liblrge_fastx_twin.so")
BAM_TWIN_PATH = os.path.join(LIB_DIR, "liblrge_bam_twin.so")
SAM_TWIN_PATH = os.path.join(LIB_DIR, "liblrge_sam_twin.so")
NAMES_TWIN_PATH = os.path.join(LIB_DIR, "liblrge_names_twin.so")
BZIP2_TWIN_PATH = os.path.join(LIB_DIR, "liblrge_bzip2_twin.so")
NAMES_LSD_TWIN_PATH = os.path.join(LIB_DIR, "liblrge_names_lsd_twin.so")
ZSTD_TWIN_PATH = os.path.join(LIB_DIR, "liblrge_zstd_twin.so")
XZ_TWIN_PATH = os.path.join(LIB_DIR, "liblrge_xz_twin.so")
CRAM_TWIN_PATH = os.path.join(LIB_DIR, "liblrge_cram_twin.so")
PAF_TWIN_PATH = os.path.join(LIB_DIR, "liblrge_paf_twin.so")


def _build_twin(out, main, force, libs=()):
    """One host twin (g++) of csrc/<main>, for the CPU suite.  It is stale when any source of the main library is newer,
    whichever headers it includes today: a rebuild takes seconds, a stale twin gives a wrong test result."""
    os.makedirs(LIB_DIR, exist_ok=True)
    if not force and os.path.exists(out) and os.path.getmtime(out) >= _newest(_sources()):
        return out
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", out, os.path.join(CSRC, main)] + list(libs))
    return out


def build_twin(force=False):
    """The host twins, all twelve: of k_inflate (csrc/inflate_twin.cpp, the same bit-level core), and of the speculative gzip
    decode (build_gzip_twin), of the FASTA / FASTQ record scan (build_fastx_twin), of the BAM record scan (build_bam_twin), of
    the SAM record scan (build_sam_twin), of the identifier ranking by refinement (build_names_twin) and by fixed LSD passes (build_names_lsd_twin)
    and of the bzip2 decode (build_bzip2_twin), the Zstandard decode (build_zstd_twin) and the xz decode (build_xz_twin), and of the CRAM base-block ingest (build_cram_twin), and of the PAF writer (build_paf_twin)."""
    build_cram_twin(force)
    build_paf_twin(force)
    build_gzip_twin(force)
    build_fastx_twin(force)
    build_bam_twin(force)
    build_sam_twin(force)
    build_names_twin(force)
    build_names_lsd_twin(force)
    build_bzip2_twin(force)
    build_zstd_twin(force)
    build_xz_twin(force)
    return _build_twin(TWIN_PATH, "inflate_twin.cpp", force)


def build_gzip_twin(force=False):
    """The host twin of the speculative gzip decode (csrc/gzip_twin.cpp): the same core and round logic."""
    return _build_twin(GZIP_TWIN_PATH, "gzip_twin.cpp", force)


def build_fastx_twin(force=False):
    """The host twin of the device record scan (csrc/fastx_twin.cpp): the same core and passes."""
    return _build_twin(FASTX_TWIN_PATH, "fastx_twin.cpp", force)


def build_bam_twin(force=False):
    """The host twin of the device BAM record scan (csrc/bam_twin.cpp): the same core and the same driver of the rounds."""
    return _build_twin(BAM_TWIN_PATH, "bam_twin.cpp", force)


def build_sam_twin(force=False):
    """The host twin of the device SAM record scan (csrc/sam_twin.cpp): the same core and the same stepping."""
    return _build_twin(SAM_TWIN_PATH, "sam_twin.cpp", force)


def build_names_twin(force=False):
    """The identifier ranking by radix refinement as host code (csrc/names_twin.cpp over csrc/name_core.h)."""
    return _build_twin(NAMES_TWIN_PATH, "names_twin.cpp", force)


def build_names_lsd_twin(force=False):
    """The host twin of the device identifier ranking (csrc/names_lsd_twin.cpp over csrc/name_lsd.h and the pass loop of
    csrc/name_lsd_round.h), and the host sort it is measured against (names_lsd_host_sort_ranks)."""
    return _build_twin(NAMES_LSD_TWIN_PATH, "names_lsd_twin.cpp", force)


def build_bzip2_twin(force=False):
    """The host twin of the block-parallel bzip2 decode (csrc/bz_twin.cpp): the same core and the same driver of the rounds."""
    return _build_twin(BZIP2_TWIN_PATH, "bz_twin.cpp", force)


def build_zstd_twin(force=False):
    """The host twin of the block-parallel Zstandard decode (csrc/zs_twin.cpp): the same core and the same driver of the rounds."""
    return _build_twin(ZSTD_TWIN_PATH, "zs_twin.cpp", force)


def build_xz_twin(force=False):
    """The host twin of the block-parallel xz decode (csrc/xz_twin.cpp): the same core and the same driver of the rounds."""
    return _build_twin(XZ_TWIN_PATH, "xz_twin.cpp", force)


def build_cram_twin(force=False):
    """The host twin of the CRAM device ingest (csrc/cram_twin.cpp): the same walk, stream heads, rounds and block decode.  It
    includes the host readers (include/lrge_io.hpp), hence zlib and libdl."""
    return _build_twin(CRAM_TWIN_PATH, "cram_twin.cpp", force, libs=("-lz", "-ldl"))


def build_paf_twin(force=False):
    """The host twin of the device PAF writer (csrc/paf_twin.cpp over csrc/paf_core.h): the measure, scan and
    write steps as loops, the dv code of a float and the proof of a p."""
    return _build_twin(PAF_TWIN_PATH, "paf_twin.cpp", force)


PRIMS_CHECK_PATH = os.path.join(LIB_DIR, "libprims_check.so")


def build_prims_check(force=False):
    """The test harness over csrc/k_prims.h (tools/prims_check.hip, hipcc for gfx950): one exported call per primitive, for
    tests/test_gpu_prims.py.  Stale when the header, internal.h or the harness is newer."""
    os.makedirs(LIB_DIR, exist_ok=True)
    src = os.path.join(os.path.dirname(_HERE), "tools", "prims_check.hip")
    deps = [src, os.path.join(CSRC, "k_prims.h"), os.path.join(CSRC, "internal.h"), os.path.join(os.path.dirname(_HERE), "include", "lrge_hip.h")]
    if not force and os.path.exists(PRIMS_CHECK_PATH) and os.path.getmtime(PRIMS_CHECK_PATH) >= _newest(deps):
        return PRIMS_CHECK_PATH
    subprocess.check_call(["hipcc"] + HIPCC_FLAGS + ["-o", PRIMS_CHECK_PATH, src])
    return PRIMS_CHECK_PATH


SEED_CHECK_PATH = os.path.join(LIB_DIR, "libseed_check.so")


def build_seed_check(force=False):
    """The test harness over csrc/k_index.h and csrc/k_seed.h (tools/seed_check.hip, hipcc for gfx950): the table build, the lookup,
    the seed counts and both expansions, one exported call each, for tests/test_gpu_seed.py.  Stale when one of the headers it
    includes or the harness is newer."""
    os.makedirs(LIB_DIR, exist_ok=True)
    src = os.path.join(os.path.dirname(_HERE), "tools", "seed_check.hip")
    deps = [src] + [os.path.join(CSRC, h) for h in ("k_seed.h", "k_index.h", "k_prims.h", "internal.h")] + [os.path.join(os.path.dirname(_HERE), "include", "lrge_hip.h")]
    if not force and os.path.exists(SEED_CHECK_PATH) and os.path.getmtime(SEED_CHECK_PATH) >= _newest(deps):
        return SEED_CHECK_PATH
    subprocess.check_call(["hipcc"] + HIPCC_FLAGS + ["-o", SEED_CHECK_PATH, src])
    return SEED_CHECK_PATH


CLI_PATH = os.path.join(LIB_DIR, "lrge-hip")


def build_cli(force=False):
    """The C++ host mirror (include/lrge_hip.hpp) + lrge-compatible driver, linked against liblrge_hip.so."""
    src = os.path.join(os.path.dirname(_HERE), "tools", "lrge_hip_cli.cpp")
    inc = os.path.join(os.path.dirname(_HERE), "include")
    hdrs = [os.path.join(inc, h) for h in ("lrge_hip.hpp", "lrge_hip.h", "lrge_rand.hpp", "lrge_io.hpp", "lrge_cram.hpp")]
    if not force and os.path.exists(CLI_PATH) and os.path.getmtime(CLI_PATH) >= max([os.path.getmtime(src), os.path.getmtime(LIB_PATH)] +
                                                                                    [os.path.getmtime(h) for h in hdrs]):
        return CLI_PATH
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", CLI_PATH, src, "-L" + LIB_DIR, "-llrge_hip", "-lz", "-ldl",
                           "-Wl,-rpath,$ORIGIN"])
    return CLI_PATH


PAF_HOST_BENCH_PATH = os.path.join(LIB_DIR, "libpaf_host_bench.so")


def build_paf_host_bench(force=False):
    """The host path of overlaps.paf with a clock around each step (tools/paf_host_bench.cpp over include/lrge_hip.hpp), for
    tools/paf_bench.py; g++, links liblrge_hip.so."""
    src = os.path.join(os.path.dirname(_HERE), "tools", "paf_host_bench.cpp")
    inc = os.path.join(os.path.dirname(_HERE), "include")
    deps = [src, LIB_PATH] + [os.path.join(inc, h) for h in ("lrge_hip.hpp", "lrge_hip.h", "lrge_rand.hpp")]
    if not force and os.path.exists(PAF_HOST_BENCH_PATH) and os.path.getmtime(PAF_HOST_BENCH_PATH) >= _newest(deps):
        return PAF_HOST_BENCH_PATH
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", PAF_HOST_BENCH_PATH, src, "-L" + LIB_DIR, "-llrge_hip",
                           "-Wl,-rpath,$ORIGIN"])
    return PAF_HOST_BENCH_PATH


if __name__ == "__main__":
    print(build_lib(force=True, verbose=True))
