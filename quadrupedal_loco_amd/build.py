"""Build libqloco.so (HIP, gfx950) in-tree with hipcc.

No cmake / JIT: one hipcc line per translation unit, objects cached by
mtime under quadrupedal_loco_amd/lib/obj/, linked into
quadrupedal_loco_amd/lib/libqloco.so (git-ignored, travels to the GPU box).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
OBJDIR = os.path.join(LIBDIR, "obj")
LIB = os.path.join(LIBDIR, "libqloco.so")
INCLUDE = os.path.join(ROOT, "include")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"

SOURCES = [
    "qloco_capi.hip",
    "qloco_srbd.hip",
    "qloco_srbd_lit.hip",
    "qloco_srbd_place.hip",
    "qloco_srbd_build.hip",
    "qloco_kin.hip",
    "qloco_gi.hip",
    "qloco_gi_wide.hip",
    "qloco_force.hip",
    "qloco_body.hip",
    "qloco_rt.hip",
    "qloco_servo.hip",
    "qloco_go1_servo.hip",
    "qloco_a1qp.hip",
    "qloco_a1est.hip",
    "qloco_a1ctrl.hip",
    "qloco_nlp.hip",
    "qloco_nlp_tick.hip",
    "qloco_nlp_node.hip",
    "qloco_mgpu.hip",
    "qloco_gen.cpp",
    "qloco_srbd_tables.cpp",
]
# per-file extra flags: the fp64 active-set kernel keeps the restatement's
# exact operation sequence (no FMA contraction)
# The SRBD kernel keeps a 64-wide register row per lane: SLP vectorisation
# pairs unrelated columns across the unrolled row loops and inflates live
# ranges into scratch spills, so it is off there (the packed-fp32 matvec and
# Gauss-Jordan updates are written with explicit float2 ops).  Its pivot
# loops are unrolled in full (static register per pivot column); the two-wave
# inverse's body exceeds the default pragma-unroll budget, so it is raised.
NO_CONTRACT = {"qloco_a1qp.hip", "qloco_a1est.hip", "qloco_a1ctrl.hip", "qloco_nlp.hip",
               "qloco_nlp_tick.hip", "qloco_nlp_node.hip", "qloco_gi.hip", "qloco_gi_wide.hip",
               "qloco_force.hip", "qloco_body.hip", "qloco_rt.hip", "qloco_servo.hip",
               "qloco_go1_servo.hip", "qloco_kin.hip"}
SRBD_FLAGS = ["-fno-slp-vectorize", "-mllvm", "-pragma-unroll-threshold=200000"]
EXTRA = {**{src: ["-ffp-contract=off"] for src in NO_CONTRACT},
         "qloco_srbd.hip": SRBD_FLAGS, "qloco_srbd_lit.hip": SRBD_FLAGS}

COMMON = ["-O3", "-std=c++17", "-fPIC", "-I" + INCLUDE, "-I" + CSRC]


def _needs(obj, deps):
    if not os.path.exists(obj):
        return True
    t = os.path.getmtime(obj)
    return any(os.path.getmtime(d) > t for d in deps)


def build(verbose=False, jobs=8):
    os.makedirs(OBJDIR, exist_ok=True)
    headers = [os.path.join(INCLUDE, "qloco.h")] + [
        os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".h", ".inc"))]
    cmds, objs = [], []
    for src in SOURCES:
        path = os.path.join(CSRC, src)
        obj = os.path.join(OBJDIR, src + ".o")
        objs.append(obj)
        if not _needs(obj, [path] + headers):
            continue
        if src.endswith(".hip"):
            cmd = ([HIPCC, "--offload-arch=" + ARCH, "-x", "hip"] + COMMON + EXTRA.get(src, []) +
                   ["-c", path, "-o", obj])
        else:  # host-only C++ (generator, literal G^-1 tables): exact IEEE, no contraction
            cmd = [HIPCC, "-x", "c++"] + COMMON + ["-ffp-contract=off", "-c", path, "-o", obj]
        cmds.append(cmd)
    procs = []
    for cmd in cmds:
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        while len([p for _, p in procs if p.poll() is None]) >= jobs:
            procs[0][1].wait()
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            sys.stderr.write(out.decode())
            raise RuntimeError("hipcc failed: " + " ".join(cmd))
    if cmds or not os.path.exists(LIB) or _needs(LIB, objs):
        link = [HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs + ["-ldl"]
        if verbose:
            print(" ".join(link))
        subprocess.run(link, check=True)
    build_host(verbose)
    for name in HOST_EXES:
        build_host_exe(name, verbose)
    return LIB


HOST_SRC = os.path.join(HERE, "host", "qloco_host.cpp")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
# host-only C++ against the HIP runtime (no device code in these TUs)
HIP_HOST = ["-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include")]
HIP_LINK = ["-L" + os.path.join(ROCM, "lib"), "-lamdhip64"]
HOST_LIB = os.path.join(LIBDIR, "libqloco_host.so")


def build_host(verbose=False):
    """C++ shim with the reference's class signatures (include/qloco.hpp) ->
    libqloco_host.so, linked against libqloco.so (rpath $ORIGIN)."""
    deps = [HOST_SRC, os.path.join(INCLUDE, "qloco.hpp"), os.path.join(INCLUDE, "qloco.h"), LIB]
    if not _needs(HOST_LIB, deps):
        return HOST_LIB
    cmd = [HIPCC, "-x", "c++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + INCLUDE] + HIP_HOST + [
           HOST_SRC, "-o", HOST_LIB, "-L" + LIBDIR, "-lqloco", "-Wl,-rpath,$ORIGIN"] + HIP_LINK
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return HOST_LIB


# tests/cpp/<name>.cpp programs over the C++ shim that link no oracle
HOST_EXES = ("test_a1_est_host", "test_a1_ctrl_host", "test_nlp_host", "test_nlp_tick_host",
             "test_nlp_node_host", "test_go1_servo_host", "test_srbd_model_host",
             "test_a1qp_body_host", "test_force_body_host")


def build_host_exe(name, verbose=False, oracle_lib=None):
    """tests/cpp/<name>.cpp -> tests/cpp/_build/<name>, linked against the shim
    and libqloco.so; with `oracle_lib`, against the oracle as checker too."""
    src = os.path.join(ROOT, "tests", "cpp", name + ".cpp")
    outdir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(outdir, exist_ok=True)
    exe = os.path.join(outdir, name)
    if not _needs(exe, [src, HOST_LIB, LIB, oracle_lib or os.path.join(INCLUDE, "qloco.hpp")]):
        return exe
    inc = link = rpath = []
    if oracle_lib:
        inc = ["-I" + os.path.join(ROOT, "oracle")]
        link = ["-L" + os.path.dirname(oracle_lib), "-lqloco_oracle"]
        rpath = ["-Wl,-rpath,$ORIGIN/../../../oracle/_build"]
    cmd = ([HIPCC, "-x", "c++", "-O2", "-std=c++17", "-I" + INCLUDE] + HIP_HOST + inc +
           [src, "-o", exe, "-L" + LIBDIR, "-lqloco_host", "-lqloco"] + link +
           ["-Wl,-rpath,$ORIGIN/../../../quadrupedal_loco_amd/lib"] + rpath + HIP_LINK)
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return exe


def build_host_test(oracle_lib, verbose=False):
    """tests/cpp/test_host (test infrastructure: links the oracle as checker)."""
    return build_host_exe("test_host", verbose, oracle_lib)


if __name__ == "__main__":
    print(build(verbose="-v" in sys.argv))
