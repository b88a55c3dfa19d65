"""Single-line correctness mutants of elect_group (gigapaxos_amd/csrc/gpx_elect.hip.h), each built into a library of its
own from a COPY of the sources: the tree is never touched.  profiles/r23_elect_enum_tests.txt holds what the election
tests made of them.

  python scripts/elect_mutants.py OUTDIR [name ...]     ->  OUTDIR/<name>/libgpx_hip.so
  GPX_HIP_LIB=OUTDIR/<name>/libgpx_hip.so python -m pytest tests/test_election_gpu.py tests/test_elect_enum_gpu.py -m gpu

Every mutant computes a wrong answer and nothing else: none indexes outside the per-lane arrays for the windows and
slots the election tests use (each substitution is annotated)."""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gigapaxos_amd", "csrc")

# name -> (old, new); `old` occurs exactly once in gpx_elect.hip.h
MUTANTS = {
    "majority-ge": ("if (__popc(wait & 0xffffu) > k / 2) {", "if (__popc(wait & 0xffffu) >= k / 2) {"),
    "pmax-ge": ("ballot_cmp(bn, bc, cb[EI(x)], cc[EI(x)]) > 0) {", "ballot_cmp(bn, bc, cb[EI(x)], cc[EI(x)]) >= 0) {"),
    "minslot-signed": ("if (jsub(s, ms) < 0) ms = s;", "if (s < ms) ms = s;"),
    "dup-not-removed": ("                        hn = ph;\n                      }\n                      removed |= 1ull << d; /* remove even if duplicate */",
                        "                        hn = ph;\n                        removed |= 1ull << d;\n                      }"),
    "preactives-plain-order": ("    for_signed_order(lo, pcount, [&](int32_t j) {\n      const int32_t s = (int32_t)((uint32_t)lo + (uint32_t)j);\n      const int64_t o =",
                               "    for (int32_t j = 0; j < pcount; j++) [&](int32_t j) {\n      const int32_t s = (int32_t)((uint32_t)lo + (uint32_t)j);\n      const int64_t o ="),
    # R == W walks one position past the window: position W <= 63 of arrays of 64 for every window below 64, and the
    # election tests carry at most six consecutive slots, so that R == 64 does not occur at window 64
    "span-gt": ("if (R >= W || R == INT32_MIN) {", "if (R > W || R == INT32_MIN) {"),
    "append-after-stop": ("                    if (pos > 0 && last_stop) return; /* nothing goes after a stop */\n", ""),
    # a 32-bit shift by x >= 32 sets another bit of the mask: wrong entries are taken for carried, all indices stay masked
    "cmask-32bit": ("                cmask |= 1ull << x;\n                co_dirty |= 1ull << x;", "                cmask |= 1u << x;\n                co_dirty |= 1ull << x;"),
    "wait-15-members": ("if (__popc(wait & 0xffffu) > k / 2) {", "if (__popc(wait & 0x7fffu) > k / 2) {"),
    "slice-ge": ("(int64_t)o + m > (int64_t)I.pv_total;", "(int64_t)o + m >= (int64_t)I.pv_total;"),
    "recorded-min-plain": ("if (q < k && mem[q] == acceptor && jsub(ns[q], ms) < 0) {", "if (q < k && mem[q] == acceptor && ns[q] < ms) {"),
    "maxmin-first-member": ("if (q < k && jsub(ns[q], maxMin) > 0) maxMin = ns[q];", "if (q < k && q > 0 && jsub(ns[q], maxMin) > 0) maxMin = ns[q];"),
}
# the closing of the lambda the plain-order mutant turned into an immediately called one
FIXUPS = {"preactives-plain-order": ("      cnt++;\n    });\n    return cnt;", "      cnt++;\n    }(j);\n    return cnt;")}


def build(outdir, name):
    old, new = MUTANTS[name]
    dst = os.path.join(outdir, name)
    shutil.rmtree(dst, ignore_errors=True)
    src = os.path.join(dst, "gigapaxos_amd", "csrc")   # (the sources include ../../include/gpx.h)
    shutil.copytree(CSRC, src, ignore=shutil.ignore_patterns("*.so", "*.o"))
    shutil.copytree(os.path.join(ROOT, "include"), os.path.join(dst, "include"))
    path = os.path.join(src, "gpx_elect.hip.h")
    text = open(path).read()
    for a, b in [(old, new)] + ([FIXUPS[name]] if name in FIXUPS else []):
        assert text.count(a) == 1, (name, text.count(a))
        text = text.replace(a, b)
    open(path, "w").write(text)
    so = os.path.join(dst, "libgpx_hip.so")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-result", "-o", so,
                           os.path.join(src, "gpx_engine.hip")], cwd=src)
    shutil.rmtree(os.path.join(dst, "gigapaxos_amd")), shutil.rmtree(os.path.join(dst, "include"))
    return so


if __name__ == "__main__":
    out = os.path.abspath(sys.argv[1])
    for nm in sys.argv[2:] or list(MUTANTS):
        print(nm, build(out, nm), flush=True)
