#!/usr/bin/env python3
"""Are the kernels two builds have in common the same device code?  Takes the gfx950 assembly of two builds of
gigapaxos_amd/csrc/gpx_engine.hip (hipcc's product flags plus --save-temps leaves gpx_engine-hip-amdgcn-amd-amdhsa-
gfx950.s beside the source; no GPU needed) and compares them function by function, comments and debug directives
dropped and the numbers of local labels - which count the functions in front - made equal.  Prints the kernels only one
build has and those that differ; exit status 1 if any differs."""
import difflib
import re
import sys


def functions(path):
    fn, cur = {}, None
    for ln in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+|k_\w+):\s", ln)
        if m:
            cur = m.group(1)
            fn[cur] = []
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
            continue
        if re.match(r"\s*(\.loc|\.file|;)", ln):
            continue
        s = ln.split(";")[0].rstrip()
        s = re.sub(r"\.LBB\d+_", ".LBB_", s)
        s = re.sub(r"\.Ltmp\d+", ".Ltmp", s)
        fn[cur].append(s)
    return fn


def main():
    if len(sys.argv) != 3:
        sys.exit("usage: isa_compare.py PARENT.s NEW.s")
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    both = [k for k in a if k in b]
    diff = [k for k in both if a[k] != b[k]]
    print("functions: %d and %d; in both %d, identical %d, different %d" % (len(a), len(b), len(both), len(both) - len(diff), len(diff)))
    print("lines compared: %d" % sum(len(a[k]) for k in both))
    for k in a:
        if k not in b:
            print("only in the first: " + k)
    for k in b:
        if k not in a:
            print("only in the second: " + k)
    for k in diff:
        print("DIFFERENT: " + k)
        print("\n".join(list(difflib.unified_diff(a[k], b[k], lineterm=""))[:20]))
    sys.exit(1 if diff else 0)


if __name__ == "__main__":
    main()
