#!/usr/bin/env python3
"""Is the gfx950 device code of two source trees the same?  `isa_diff.py OLD_TREE NEW_TREE [-- extra compiler flags]`

Every radar-sounder-crw_amd/csrc/*.hip of both trees is compiled with the Makefile's flags (device side only, no bundle),
disassembled with llvm-objdump -d, and the two listings are compared whole, minus the lines that name the object file.  (The
ELF bytes differ from build to build; the disassembly does not.)  One line per file; exit status 1 if any file differs or
exists in one tree only.  A refactor of the kernel sources that claims to be neutral shows it with this.
"""
import concurrent.futures as cf
import os
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CSRC = "radar-sounder-crw_amd/csrc"


def listing(tree, name, extra, tmp):
    obj = os.path.join(tmp, "%s.%s.o" % (abs(hash(tree)), name))
    cmd = [ROCM + "/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-I" + os.path.join(tree, "include"),
           "-Wall", "-Wno-unused-function", *extra, "--cuda-device-only", "--no-gpu-bundle-output", "-c",
           os.path.join(tree, CSRC, name), "-o", obj]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    if cc.returncode:
        return "COMPILE ERROR\n" + cc.stderr
    dis = subprocess.run([ROCM + "/llvm/bin/llvm-objdump", "-d", obj], capture_output=True, text=True)
    if dis.returncode:
        return "OBJDUMP ERROR\n" + dis.stderr
    return "\n".join(l for l in dis.stdout.splitlines() if obj not in l and "file format" not in l)


def main():
    args, extra = sys.argv[1:], []
    if "--" in args:
        args, extra = args[:args.index("--")], args[args.index("--") + 1:]
    if len(args) != 2:
        sys.exit(__doc__)
    old, new = (os.path.abspath(a) for a in args)
    names = sorted({f for t in (old, new) for f in os.listdir(os.path.join(t, CSRC)) if f.endswith(".hip")})
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(int(os.environ.get("JOBS", "8"))) as pool:
        jobs = {(t, n): pool.submit(listing, t, n, extra, tmp) for t in (old, new) for n in names
                if os.path.exists(os.path.join(t, CSRC, n))}
        for n in names:
            a, b = (jobs[(t, n)].result() if (t, n) in jobs else None for t in (old, new))
            if a is None or b is None:
                verdict = "ONLY IN " + ("NEW" if a is None else "OLD")
            elif "ERROR" in a.split("\n", 1)[0] or "ERROR" in b.split("\n", 1)[0]:
                verdict = (a if "ERROR" in a.split("\n", 1)[0] else b).strip()
            else:
                verdict = "identical" if a == b else "DIFFERENT"
            bad += verdict != "identical"
            lines = 0 if a is None else sum(1 for l in a.splitlines() if l.startswith("\t"))
            print("%-22s %-10s %7d instructions" % (n, verdict, lines))
    print("flags: %s    %d files, %d not identical" % (" ".join(extra) or "(default)", len(names), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
