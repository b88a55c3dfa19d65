#!/usr/bin/env python3
"""Registers and scratch of every k_scatter_tiles instantiation, and the `nt` modifiers of the stream sites
(GPX_NT_STREAMS, gigapaxos_amd/csrc/gpx_kernels.hip.h): compiles gigapaxos_amd/csrc/gpx_engine.hip for gfx950 with the
Makefile's flags (no GPU needed), once for the resource remarks and once for the device listing.
    python scripts/scatter_resources.py [-DGPX_NT_STREAMS=31 ...]
Exit status 1 when an instantiation that tile_shape() picks by itself (<1024, 3>, <1024, 2>, <512, 2>) has scratch.  <1024, 4>
(a forced shape only) has had scratch since round 6 and is reported, not judged."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gigapaxos_amd", "csrc")
FLAGS = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-w"]
PICKED = ("k_scatter_tiles<1024, 3>", "k_scatter_tiles<1024, 2>", "k_scatter_tiles<512, 2>")
STREAM_KERNELS = r"k_scatter_tiles|k_propose_one|k_propose_pers|k_bucket_ar16_tiles"


def demangle(sym):
    return subprocess.run(["c++filt", "-p", sym], stdout=subprocess.PIPE, text=True).stdout.strip() or sym


def main():
    extra = sys.argv[1:]
    with tempfile.TemporaryDirectory() as tmp:
        err = subprocess.run(FLAGS + ["-shared", "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(tmp, "x.so"),
                                      "gpx_engine.hip"] + extra, cwd=CSRC, stderr=subprocess.PIPE, text=True, check=True).stderr
        asm = os.path.join(tmp, "x.s")
        subprocess.run(FLAGS + ["-S", "--cuda-device-only", "-o", asm, "gpx_engine.hip"] + extra, cwd=CSRC, check=True)
        listing = open(asm).read()
    rows, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|[A-Za-z ]+(?:\[[^\]]*\])?):\s*(\S+)", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = rows.setdefault(demangle(val), {})
        elif cur is not None:
            cur[key] = val
    bad = 0
    print(f"{'kernel':30s}{'VGPR':>6s}{'scratch':>9s}{'vspill':>8s}   private_segment_fixed_size")
    for name in sorted(rows):
        if not name.startswith("k_scatter_tiles"):
            continue
        r = rows[name]
        scratch = r.get("ScratchSize [bytes/lane]", "?")
        print(f"{name:30s}{r.get('VGPRs', '?'):>6s}{scratch:>9s}{r.get('VGPRs Spill', '?'):>8s}   {scratch}"
              + ("" if name in PICKED else "   (forced shapes only)"))
        bad += name in PICKED and scratch != "0"
    print()
    print(f"{'kernel':30s}{'loads':>7s}{'nt':>5s}{'stores':>8s}{'nt':>5s}")
    for body in re.split(r"\n(?=\S+:\s*; @)", listing):
        m = re.match(r"(\S+):", body)
        if not m or not re.search(STREAM_KERNELS, m.group(1)):
            continue
        ld, st = re.findall(r"global_load_\w+ .*", body), re.findall(r"global_store_\w+ .*", body)
        nt = lambda xs: sum(1 for x in xs if re.search(r"\bnt\b", x))  # noqa: E731
        print(f"{demangle(m.group(1))[:30]:30s}{len(ld):7d}{nt(ld):5d}{len(st):8d}{nt(st):5d}")
    print(f"# {bad} of the picked scatter instantiations with scratch (required: 0)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
