"""Is the device code of some csrc/*.hip files the same at a git revision and in the working tree?  CPU only.
    python tools/isa_diff.py <revision> wino.hip conv3x3.hip ...
Both sides are compiled to gfx950 assembly with the flags of clsurvey_amd/build.py (+ --cuda-device-only -S) and compared kernel by
kernel, in file order: the text from the kernel's label to its descriptor, and the .amdhsa_* descriptor block (registers, LDS,
scratch).  __hip_cuid_ lines are dropped and a kernel's own mangled name is replaced by a placeholder, so a kernel whose template
parameter list changed still compares equal when its code did.  Exit status 1 when anything differs."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clsurvey_amd import build as b  # noqa: E402


def assembly(tree, src):
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + b.FLAGS + b.EXTRA_FLAGS.get(src, []) + \
          ["--cuda-device-only", "-S", os.path.join(tree, "clsurvey_amd", "csrc", src), "-o", "-"]
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout          # (compiler messages pass through)


def kernels(asm):
    """[(mangled name, code text, descriptor text)] in file order, names replaced by a placeholder"""
    lines = [ln for ln in asm.splitlines() if "__hip_cuid_" not in ln]
    out = []
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        name = m.group(1)
        start = next(j for j, l2 in enumerate(lines) if l2.startswith(name + ":"))
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        out.append((name, "\n".join(lines[start:i]).replace(name, "<kernel>"), "\n".join(lines[i:end + 1]).replace(name, "<kernel>")))
    return out


def main():
    rev, srcs = sys.argv[1], sys.argv[2:]
    bad = 0
    with tempfile.TemporaryDirectory() as old:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "clsurvey_amd/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
        with ThreadPoolExecutor(max_workers=min(16, 2 * len(srcs))) as pool:
            jobs = [(s, pool.submit(assembly, old, s), pool.submit(assembly, ROOT, s)) for s in srcs]
            for src, fa, fb in jobs:
                ka, kb = kernels(fa.result()), kernels(fb.result())
                print("%s: %d kernels at %s, %d in the working tree" % (src, len(ka), rev, len(kb)))
                if len(ka) != len(kb):
                    bad += 1
                    continue
                for (na, ca, da), (nb, cb, db) in zip(ka, kb):
                    same = ca == cb and da == db
                    bad += not same
                    what = "identical" if same else "DIFFERENT:" + (" code" if ca != cb else "") + (" descriptor" if da != db else "")
                    print("  %-10s %s%s" % (what, nb, "" if na == nb else "   (was " + na + ")"))
    print("all kernels identical" if not bad else "%d DIFFERENCES" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
