"""Build recipe for libclhip.so (hipcc, gfx950 only). In-tree output: clsurvey_amd/libclhip.so
so the built library travels with the repo snapshot to the GPU box."""
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libclhip.so")
SOURCES = ["elementwise.hip", "loss.hip", "lwf_wide.hip", "pool.hip", "conv3x3.hip", "wino.hip", "bsconv.hip", "bswgrad.hip", "bswgrad5.hip", "conv3x3_wgrad.hip", "conv2d.hip", "convkk.hip", "s2dconv.hip", "bn.hip", "gemm.hip", "fc_chain.hip",
           "packnet.hip", "hat.hip", "pathnet.hip", "gem.hip", "gem_wide.hip", "rehearsal.hip", "joint.hip", "augment.hip", "icarl.hip", "icarl_assemble.hip", "engine.hip"]
# -pragma-unroll-threshold: the software-pipelined conv loops are fully unrolled by `#pragma unroll` (one piece of
# staging work per MFMA slot, all register-array indices constant); at the default threshold hipcc silently stops
# unrolling the largest instance and its operand registers land in scratch / LDS.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wno-unused-function",
         "-mllvm", "-pragma-unroll-threshold=100000"]


# Per-source additions.  wino.hip: the SLP vectoriser packs neighbouring fp32 adds of the Winograd transforms into
# v_pk_add_f32, which costs ~13 cycles more than a plain v_add_f32 when issued beside MFMAs (MI355X_MICROARCH.md,
# per-instruction constants); measured -1.4 % on the conv time of a small_VGG9 pass, -0.5 % on wide_VGG9
# (profiles/r04_w16g_schedule_variants.txt).
EXTRA_FLAGS = {"wino.hip": ["-fno-slp-vectorize"]}


def _fingerprint(paths, flags):
    """sha256 over the compiler flags and the bytes of a source and the headers it includes: an object file is reused
    only when this matches the stamp written next to it (mtimes do not survive a repository snapshot)."""
    import hashlib
    h = hashlib.sha256(" ".join(flags).encode())
    for path in paths:
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def build(force=False, verbose=True):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    hdrs = sorted(glob.glob(os.path.join(CSRC, "*.hpp"))) + [os.path.join(HERE, "..", "include", "clhip.h")]
    procs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, src.replace(".hip", ".o"))
        stamp = o + ".sha256"
        objs.append(o)
        flags = FLAGS + EXTRA_FLAGS.get(src, [])
        want = _fingerprint([s] + hdrs, flags)
        have = open(stamp).read().strip() if os.path.exists(stamp) and os.path.exists(o) else ""
        if force or have != want:
            cmd = [hipcc] + flags + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            if os.path.exists(stamp):
                os.remove(stamp)
            procs.append((src, stamp, want, subprocess.Popen(cmd)))
    for src, stamp, want, p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed on " + src)
        with open(stamp, "w") as f:
            f.write(want + "\n")
    if force or procs or not os.path.exists(OUT):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return OUT


TEST_LIB_SRC = os.path.join(HERE, "..", "tests", "csrc", "debug_naive.hip")
TEST_LIB = os.path.join(HERE, "..", "tests", "libclhip_dbg.so")


def build_test_lib(force=False, verbose=True):
    """tests/libclhip_dbg.so: the naive triage kernels and the MFMA fragment probe of tests/csrc/debug_naive.hip — test
    infrastructure, deliberately not linked into the product library."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    stamp = TEST_LIB + ".sha256"
    want = _fingerprint([TEST_LIB_SRC, os.path.join(CSRC, "common.hpp"), os.path.join(HERE, "..", "include", "clhip.h")], FLAGS)
    have = open(stamp).read().strip() if os.path.exists(stamp) and os.path.exists(TEST_LIB) else ""
    if force or have != want:
        cmd = [hipcc] + FLAGS + ["-shared", "-o", TEST_LIB, TEST_LIB_SRC]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        with open(stamp, "w") as f:
            f.write(want + "\n")
    return TEST_LIB


def build_variant(name, src, defines, verbose=True, extra_flags=()):
    """Experimental variant: recompile ONE source with extra -D flags and link libclhip_<name>.so.
    Selected at run time with CLHIP_LIB=<path> (tools/ only; the product always loads libclhip.so)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    build(verbose=verbose)
    srcs = [src] if isinstance(src, str) else list(src)
    procs = []
    for s in srcs:
        o = os.path.join(CSRC, s.replace(".hip", ".%s.o" % name))
        cmd = [hipcc] + FLAGS + EXTRA_FLAGS.get(s, []) + list(extra_flags) + ["-D" + d for d in defines] + ["-c", os.path.join(CSRC, s), "-o", o]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append(subprocess.Popen(cmd))
    for p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed on variant " + name)
    objs = [os.path.join(CSRC, x.replace(".hip", ".%s.o" % name if x in srcs else ".o")) for x in SOURCES]
    out = os.path.join(HERE, "libclhip_%s.so" % name)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs)
    return out


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    build_test_lib(force="--force" in sys.argv)
