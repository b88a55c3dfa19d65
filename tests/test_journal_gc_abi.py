"""The journal compaction (include/gpx_journal_gc.h), the part that needs no GPU: the header, the exported symbols, the
binding, the JNI twin and the build lists; the argument checks, which come before any device work; and the kernels in
lockstep emulation under AddressSanitizer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import journal_gc_model as GM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("gpx_journal_gc", "gpx_journal_gc_dev")
EINVAL, ECAPACITY = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from gigapaxos_amd import load_hip

    return load_hip()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx_journal_gc.h")).read(), flags=re.S)


def test_header_library_binding_and_jni_agree(lib):
    from gigapaxos_amd import _abi, journal_gc

    src = header()
    assert set(re.findall(r"\b(gpx_[a-z_]+)\s*\(", src)) == set(CALLS)
    raw = ctypes.CDLL(lib.path)
    sigs = []
    for name in CALLS:
        assert hasattr(raw, name), name
        assert name[4:] in _abi.EXPORTED_SYMBOLS and name[4:] in _abi._DEV_SIGS and name[4:] in lib.fn
        assert callable(getattr(journal_gc, name[4:]))
        # twenty-six arguments in the header, twenty-five after the handle in the binding
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(args) == 26 and len(_abi._DEV_SIGS[name[4:]]) == 25
        sigs.append([re.sub(r"\s+", " ", a).strip() for a in args])
    assert sigs[0] == sigs[1]                         # the two forms take the same arguments
    # the pack's header keeps its pinned set of names; the two headers whose symbols need an oracle twin stay free of the word
    pack = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx_journal.h")).read(), flags=re.S)
    assert "journal_gc" not in pack
    for hdr in ("gpx.h", "gpx_wire.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", hdr)).read(), flags=re.S)
        assert "journal" not in text
    fields = ["n_usable", "n_keep", "n_done", "n_bad", "n_unjudged", "n_runs_done", "unchanged", "reserved", "keep_bytes",
              "bytes_done", "named_bytes", "reserved2"]
    assert ctypes.sizeof(journal_gc.JournalGcCounts) == 64 == journal_gc.COUNTS_BYTES
    assert [f for f, _ in journal_gc.JournalGcCounts._fields_] == fields == list(GM.COUNT_FIELDS)
    assert re.search(r".*".join(r"int%s_t %s;" % ("32" if i < 8 else "64", f) for i, f in enumerate(fields)), src, flags=re.S)
    # flags and verdicts: the header, the binding, the model
    for name, b, m in (("COUNT_ONLY", journal_gc.JG_COUNT_ONLY, GM.COUNT_ONLY), ("SKIP_UNCHANGED", journal_gc.JG_SKIP_UNCHANGED, GM.SKIP_UNCHANGED),
                       ("DROP", journal_gc.JG_DROP, GM.DROP), ("KEEP", journal_gc.JG_KEEP, GM.KEEP),
                       ("KEEP_UNJUDGED", journal_gc.JG_KEEP_UNJUDGED, GM.KEEP_UNJUDGED), ("BAD", journal_gc.JG_BAD, GM.BAD)):
        assert int(re.search(r"#define GPX_JG_%s (\d+)" % name, src).group(1)) == b == m, name
    assert (GM.COUNT_ONLY, GM.SKIP_UNCHANGED, GM.DROP, GM.KEEP, GM.KEEP_UNJUDGED, GM.BAD) == (1, 2, 0, 1, 2, 3)
    assert [c for c, _ in journal_gc.ROW_COLS] == list(GM.ROW_COLS)
    # what is out of scope, the deviation and the n_bad rule stand where a reader of the header sees them
    full = open(os.path.join(ROOT, "include", "gpx_journal_gc.h")).read()
    for phrase in ("MUST NOT REPLACE A FILE WHEN", "Out of scope", "LogIndex.java:331-345", "SQLPaxosLogger.java:1481-1482",
                   "One deviation", "PREPARE", "LOGFILE_AGE_THRESHOLD", "isRemovable", "LAZY_COMPACTION", "mergeLogfiles",
                   "round_up(in_bytes, 16)", "3427-3431", "3432-3436"):
        assert phrase in full, phrase
    # the JNI twin: env, class, handle, then the twenty-five arguments of the call; it compiles against the header
    shim = os.path.join(ROOT, "gigapaxos_amd", "jni", "gpx_jni.c")
    m = re.search(r"JFN\(jint, journalGc\)\(([^)]*)\)", open(shim).read())
    assert m and len(m.group(1).split(",")) == 28
    subprocess.check_call(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-DGPX_HAVE_JNI", "-I",
                           os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"), shim])
    # the build lists know the header
    for f in ("Makefile", "__graft_entry__.py"):
        assert "gpx_journal_gc.h" in open(os.path.join(ROOT, f)).read(), f
    # the C struct is 64 bytes for a C compiler too
    subprocess.check_call(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c",
                           os.path.join(ROOT, "tests", "journal_gc_sizeof.h")])


def test_argument_errors_come_before_any_device_work(lib):
    """No engine exists here (there is no GPU): every refusal below is decided from the arguments alone.  The handle of
    the later cases is a GpxConfig-shaped block - of a handle the checks read max_batch and nothing else - and every
    output is filled with a sentinel that must still be there afterwards."""
    blk = np.zeros(1 << 16, np.uint8)
    blk.view(np.int32)[4] = 64                         # struct gpx_config: max_batch is its fifth word
    h = blk.ctypes.data_as(ctypes.c_void_p)
    keep = blk.copy()
    counts = ctypes.create_string_buffer(b"\xa5" * 64, 64)
    cp = ctypes.cast(counts, ctypes.c_void_p)
    col = np.full(256, 0xA5A5A5A5A5A5A5A5, np.uint64)
    base = col.ctypes.data + (-col.ctypes.data) % 16
    p = ctypes.c_void_p(base)
    odd = [ctypes.c_void_p(base + k) for k in (1, 4, 8, 15)]

    def call(f, h=h, n=4, inp=p, ib=100, ibase=0, g=p, s=p, off=p, ln=p, bn=p, bc=p, cps=None, obase=0, flags=0, out=p, cb=64,
             ce=4, ver=p, rows=(p, p, p), kbn=p, kbc=p, ko=p, kl=p, c=cp):
        return f(h, n, inp, ib, ibase, g, s, off, ln, bn, bc, cps, obase, flags, out, cb, ce, ver, *rows, kbn, kbc, ko, kl, c)
    for name in ("journal_gc", "journal_gc_dev"):
        f = lib.fn[name]
        assert call(f, h=None) == EINVAL                                    # null handle
        assert call(f, c=None) == EINVAL                                    # null counts
        for kw in (dict(n=-1), dict(ib=-1), dict(cb=-1), dict(ce=-1)):      # negative sizes and caps
            assert call(f, **kw) == EINVAL, kw
        for flags in (4, 8, 7, -1, 1 << 30):                                # unknown flag bits
            assert call(f, flags=flags) == EINVAL
        for kw in (dict(g=None), dict(s=None), dict(off=None), dict(ln=None)):        # required in every call with n > 0
            for flags in (0, 1, 2, 3):
                assert call(f, flags=flags, **kw) == EINVAL, kw
        for kw in (dict(inp=None), dict(out=None), dict(ko=None), dict(kl=None)):     # required where something is written
            assert call(f, **kw) == EINVAL, kw
            assert call(f, flags=2, **kw) == EINVAL, kw
        assert call(f, bn=None) == EINVAL and call(f, bc=None) == EINVAL    # an output column without its input
        for q in odd:                                                       # in, out not 16-byte aligned
            assert call(f, out=q) == EINVAL and call(f, inp=q) == EINVAL and call(f, inp=q, flags=1) == EINVAL
        assert call(f, n=65) == ECAPACITY                                   # n > max_batch
        assert call(f, n=65, flags=1, inp=None, out=None, ko=None, kl=None) == ECAPACITY
    assert (blk == keep).all() and counts.raw == b"\xa5" * 64 and (col == 0xA5A5A5A5A5A5A5A5).all()


def test_jg_kernels_in_lockstep_emulation_under_asan(tmp_path):
    """tests/journal_gc_emulation.cpp: the kernels of gpx_journal_gc.hip.h as they are, one thread per lane - the case
    list of tests/test_journal_gc_gpu.py: verdicts under every cp_slot mode, every source phase against every output
    phase, runs of kept rows over the row-tile edge, everything and nothing kept, broken adjacency, totals around one,
    two and three output tiles, 5,000 runs in two tiles, an entry over 64 tiles, every kind of refused row, both caps, a
    cut call continued, counts only, n = 0, NULL columns, 274 tiles of rows - with garbage in the scratch and every
    buffer of its exact size (`in` rounded up to 16) under AddressSanitizer.  A stand-alone program: nothing is loaded
    into Python."""
    exe = str(tmp_path / "journal_gc_emulation")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-pthread", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "gigapaxos_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "journal_gc_emulation.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 95 and all(": ok" in ln for ln in lines), out.stdout
