#!/usr/bin/env python3
"""Is the gfx950 device code of two source trees the same?  `isa_diff.py OLD_TREE NEW_TREE [-- extra compiler flags]`

Every radar-sounder-crw_amd/csrc/*.hip of both trees is compiled with the Makefile's flags (device side only, no bundle),
disassembled with llvm-objdump -d, and the two listings are compared whole, minus the lines that name the object file.  (The
ELF bytes differ from build to build; the disassembly does not.)  One line per file; exit status 1 if any file differs or
exists in one tree only.  A refactor of the kernel sources that claims to be neutral shows it with this.

`isa_diff.py --functions FILE.hip [--added ARGS] OLD_TREE NEW_TREE`: one file, function by function -- for a change that adds
kernels to a file and claims to leave the others as they were.  A function of OLD is looked up in NEW under its demangled name;
a kernel template that gained trailing template parameters under its old arguments followed by ARGS (e.g. `--added false`).
Compared: every instruction's text and encoding (not its address; a branch target by its offset in the function).
"""
import concurrent.futures as cf
import os
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CSRC = "radar-sounder-crw_amd/csrc"


def listing(tree, name, extra, tmp, demangle=False):
    obj = os.path.join(tmp, "%s.%s.o" % (abs(hash(tree)), name))
    cmd = [ROCM + "/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-I" + os.path.join(tree, "include"),
           "-Wall", "-Wno-unused-function", *extra, "--cuda-device-only", "--no-gpu-bundle-output", "-c",
           os.path.join(tree, CSRC, name), "-o", obj]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    if cc.returncode:
        return "COMPILE ERROR\n" + cc.stderr
    dis = subprocess.run([ROCM + "/llvm/bin/llvm-objdump", "-d", *(["-C"] if demangle else []), obj], capture_output=True, text=True)
    if dis.returncode:
        return "OBJDUMP ERROR\n" + dis.stderr
    return "\n".join(l for l in dis.stdout.splitlines() if obj not in l and "file format" not in l)


def functions(text):
    """{key: [instruction lines]} of a demangled listing.  key: the name with its template arguments and without its parameter
    list; an instruction line keeps its text and its encoding, not its address, and a branch target keeps its offset only."""
    import re

    def key(d):
        depth, out = 0, ""
        for ch in d.replace("(anonymous namespace)", "{anon}"):
            if ch == "(" and depth == 0:
                break
            depth += (ch == "<") - (ch == ">")
            out += ch
        return out.split(" ", 1)[-1] if out.startswith("void ") else out

    funcs, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = funcs.setdefault(key(m.group(1)), [])
        elif cur is not None and line.startswith("\t"):
            ins, _, enc = line.partition("//")
            cur.append(ins.rstrip() + " //" + re.sub(r" <.*?(\+0x[0-9a-f]+)?>$", r" <\1>", enc.split(":", 1)[-1].rstrip()))
    return funcs


def by_function(old, new, name, extra, added):
    """One line per function of OLD's `name`: is its instruction stream in NEW the same?  A kernel template that gained trailing
    parameters is found under its old arguments followed by `added` (e.g. "false")."""
    with tempfile.TemporaryDirectory() as tmp:
        a, b = (listing(t, name, extra, tmp, demangle=True) for t in (old, new))
    for t in (a, b):
        if "ERROR" in t.split("\n", 1)[0]:
            sys.exit(t)
    fa, fb = functions(a), functions(b)
    bad, seen = 0, set()
    for k in sorted(fa):
        k2 = k if k in fb or not k.endswith(">") or not added else k[:-1] + ", " + added + ">"
        seen.add(k2)
        verdict = "MISSING" if k2 not in fb else "identical" if fa[k] == fb[k2] else "DIFFERENT"
        bad += verdict != "identical"
        print("%-10s %6d instructions  %s%s" % (verdict, len(fa[k]), k, "" if k2 == k else "   (now %s)" % k2))
    for k in sorted(set(fb) - seen):
        print("%-10s %6d instructions  %s" % ("NEW", len(fb[k]), k))
    print("%s: %d functions of the old tree, %d not identical, %d new" % (name, len(fa), bad, len(set(fb) - seen)))
    return 1 if bad else 0


def main():
    args, extra = sys.argv[1:], []
    if "--" in args:
        args, extra = args[:args.index("--")], args[args.index("--") + 1:]
    if len(args) >= 4 and args[0] == "--functions":  # --functions FILE.hip [--added ARGS] OLD_TREE NEW_TREE
        added = args[args.index("--added") + 1] if "--added" in args else ""
        return by_function(os.path.abspath(args[-2]), os.path.abspath(args[-1]), args[1], extra, added)
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
