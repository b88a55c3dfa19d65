"""The log index (include/gpx_logindex.h), the part that needs no GPU: the header, the exported symbols, the binding,
the JNI twins and the build lists; the argument checks, which come before any device work; and the kernels in lockstep
emulation under AddressSanitizer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import logindex_model as LM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("add", "set_gc", "lookup", "file_rows", "relocate", "files", "compact")
ARGS = dict(add=12, set_gc=7, lookup=17, file_rows=12, relocate=10, files=7, compact=2)    # with the handle
JNI = dict(add="logindexAdd", set_gc="logindexSetGc", lookup="logindexLookup", file_rows="logindexFileRows",
           relocate="logindexRelocate", files="logindexFiles", compact="logindexCompact")
EINVAL, ECAPACITY = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from gigapaxos_amd import load_hip

    return load_hip()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx_logindex.h")).read(), flags=re.S)


def test_header_library_binding_and_jni_agree(lib):
    from gigapaxos_amd import _abi, logindex

    src = header()
    calls = ["gpx_logindex_open"] + ["gpx_logindex_%s%s" % (k, f) for k in NAMES for f in ("_dev", "")]
    assert set(re.findall(r"\b(gpx_[a-z_]+)\s*\(", src)) == set(calls)
    raw = ctypes.CDLL(lib.path)
    shim = open(os.path.join(ROOT, "gigapaxos_amd", "jni", "gpx_jni.c")).read()
    for name in calls:
        assert hasattr(raw, name), name
        assert name[4:] in _abi.EXPORTED_SYMBOLS and name[4:] in _abi._DEV_SIGS and name[4:] in lib.fn
    for k in NAMES:
        sigs = []
        for f in ("_dev", ""):
            args = re.search(r"\bgpx_logindex_%s%s\s*\(([^)]*)\)" % (k, f), src).group(1).split(",")
            assert len(args) == ARGS[k] == len(_abi._DEV_SIGS["logindex_" + k + f]) + 1, k
            sigs.append([re.sub(r"\s+", " ", a).strip() for a in args])
            assert callable(getattr(logindex, k + f))
        assert sigs[0] == sigs[1], k                  # the two forms take the same arguments
        # the JNI twin of the host form: env, class, then the arguments of the call
        m = re.search(r"JFN\(jint, %s\)\(([^)]*)\)" % JNI[k], shim)
        assert m and len(m.group(1).split(",")) == ARGS[k] + 2, k
    assert re.search(r"JFN\(jint, logindexOpen\)\(([^)]*)\)", shim) and callable(logindex.open)
    subprocess.check_call(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-DGPX_HAVE_JNI", "-I",
                           os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "gigapaxos_amd", "jni", "gpx_jni.c")])
    # the journal headers keep their pinned sets of names; the two headers whose symbols need an oracle twin stay free
    for hdr in ("gpx_journal.h", "gpx_journal_gc.h", "gpx.h", "gpx_wire.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", hdr)).read(), flags=re.S)
        assert "logindex" not in text, hdr
    assert ctypes.sizeof(logindex.LogIndexCounts) == 32 == logindex.COUNTS_BYTES
    assert [f for f, _ in logindex.LogIndexCounts._fields_] == list(LM.COUNT_FIELDS)
    assert re.search(r".*".join(r"int32_t %s;" % f for f in LM.COUNT_FIELDS), src, flags=re.S)
    for name, b, m in (("ADDED", logindex.LI_ADDED, LM.ADDED), ("STALE", logindex.LI_STALE, LM.STALE),
                       ("NOGROUP", logindex.LI_NOGROUP, LM.NOGROUP), ("FULL", logindex.LI_FULL, LM.FULL),
                       ("REPEAT", logindex.LI_REPEAT, LM.REPEAT), ("RESET", logindex.LI_RESET, LM.RESET),
                       ("MAX_FILES", logindex.LI_MAX_FILES, LM.MAX_FILES)):
        assert int(re.search(r"#define GPX_LI_%s (\d+)" % name, src).group(1)) == b == m, name
    assert (LM.ADDED, LM.STALE, LM.NOGROUP, LM.FULL, LM.REPEAT, LM.RESET, LM.MAX_FILES) == (0, 1, 2, 3, 4, 1, 4096)
    assert [c for c, _ in logindex.LOOKUP_COLS] == list(LM.LOOKUP_COLS)
    assert [c for c, _ in logindex.FILE_ROWS_COLS] == list(LM.FILE_ROWS_COLS)
    # the citations, the deviations and what is out of scope stand where a reader of the header sees them
    full = open(os.path.join(ROOT, "include", "gpx_logindex.h")).read()
    for phrase in ("LogIndex.java:192-204", ":128-152", ":213-237", ":174-186", ":319-322", ":253-259", ":331-345",
                   "SQLPaxosLogger.java:367-490", "3639-3760", "3174-3207", "2725-2744", "getOrCreateIfNotExistsOrLower",
                   "Deviations", "row identity", "Out of scope", "lastActive", "IT IS NOT GROUP STATE",
                   "WHY THAT KEEPS EVERY ROW", "CHECKPOINT_INTERVAL", "garbage is refused"):
        assert phrase in full, phrase
    for f in ("Makefile", "__graft_entry__.py"):
        assert "gpx_logindex.h" in open(os.path.join(ROOT, f)).read(), f
    subprocess.check_call(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c",
                           os.path.join(ROOT, "tests", "logindex_sizeof.h")])


def test_argument_errors_come_before_any_device_work(lib):
    """No engine exists here (there is no GPU): every refusal below is decided from the arguments alone.  The handle is
    a zeroed block shaped like gpx_config - of a handle the checks read max_batch, then the word that says whether the
    index is open, which a zeroed block answers with no - and every output holds a sentinel that must still be there."""
    blk = np.zeros(1 << 16, np.uint8)
    blk.view(np.int32)[4] = 64                         # struct gpx_config: max_batch is its fifth word
    h = blk.ctypes.data_as(ctypes.c_void_p)
    keep = blk.copy()
    counts = ctypes.create_string_buffer(b"\xa5" * 32, 32)
    cp = ctypes.cast(counts, ctypes.c_void_p)
    col = np.full(256, 0xA5A5A5A5A5A5A5A5, np.uint64)
    p = ctypes.c_void_p(col.ctypes.data)
    one = np.array([3], np.int32)
    nd = ctypes.c_void_p(one.ctypes.data)
    for sfx in ("_dev", ""):
        f = {k: lib.fn["logindex_" + k + sfx] for k in NAMES}

        def add(h=h, n=4, nd=None, cols=(p,) * 6, file=1, st=p, c=cp):
            return f["add"](h, n, nd, *cols, file, st, c)

        def set_gc(h=h, n=4, g=p, gc=p, flags=0, st=p, c=cp):
            return f["set_gc"](h, n, g, gc, flags, st, c)

        def lookup(h=h, n=4, g=p, lo=p, hi=p, hm=p, cap=4, outs=(p,) * 8, st=p, c=cp):
            return f["lookup"](h, n, g, lo, hi, hm, cap, *outs, st, c)

        def file_rows(h=h, file=0, cap=4, outs=(p,) * 8, c=cp):
            return f["file_rows"](h, file, cap, *outs, c)

        def relocate(h=h, n=4, nd=None, gen=0, row=p, src=p, nf=1, off=p, ln=p, c=cp):
            return f["relocate"](h, n, nd, gen, row, src, nf, off, ln, c)

        def files(h=h, base=0, nf=4, r=p, g=p, m=p, c=cp):
            return f["files"](h, base, nf, r, g, m, c)

        for call in (add, set_gc, lookup, file_rows, relocate, files):
            assert call(h=None) == EINVAL and call(c=None) == EINVAL            # null handle, null counts
        assert f["compact"](None, cp) == EINVAL and f["compact"](h, None) == EINVAL
        for call in (add, set_gc, lookup, relocate):
            assert call(n=-1) == EINVAL
            assert call(n=65) == ECAPACITY                                      # n > max_batch
        assert add(file=-1) == EINVAL and relocate(nf=-1) == EINVAL
        for k in range(6):                                                      # a null row column
            assert add(cols=tuple(None if q == k else p for q in range(6))) == EINVAL
        assert set_gc(g=None) == EINVAL and set_gc(gc=None) == EINVAL and set_gc(flags=2) == EINVAL
        assert set_gc(flags=-1) == EINVAL and set_gc(flags=3) == EINVAL
        assert lookup(g=None) == EINVAL and lookup(lo=None) == EINVAL and lookup(hi=None) == EINVAL and lookup(cap=-1) == EINVAL
        assert file_rows(cap=-1) == EINVAL
        for k in range(8):                                                      # a null output column with cap > 0
            outs = tuple(None if q == k else p for q in range(8))
            assert lookup(outs=outs) == EINVAL and file_rows(outs=outs) == EINVAL
        assert relocate(row=None) == EINVAL and relocate(off=None) == EINVAL and relocate(ln=None) == EINVAL
        assert files(nf=-1) == EINVAL and files(nf=4097) == EINVAL
        # nothing wrong with the arguments: the index is not open
        for call in (add, set_gc, lookup, file_rows, relocate, files):
            assert call() == EINVAL
        assert add(nd=nd) == EINVAL and set_gc(gc=None, flags=1) == EINVAL and lookup(hi=None, hm=None) == EINVAL
        assert lookup(cap=0, outs=(None,) * 8) == EINVAL and f["compact"](h, cp) == EINVAL and files(nf=4096) == EINVAL
    assert lib.fn["logindex_open"](None, 16) == EINVAL
    assert (blk == keep).all() and counts.raw == b"\xa5" * 32 and (col == 0xA5A5A5A5A5A5A5A5).all() and one[0] == 3


def test_li_kernels_in_lockstep_emulation_under_asan(tmp_path):
    """tests/logindex_emulation.cpp: the kernels of gpx_logindex.hip.h as they are, one thread per lane - the case list of
    tests/test_logindex_gpu.py: adds of 255 / 256 / 257 / 513 records onto tails at 0, 255, 256 and 1,023, a full table
    and the repeat after compact, every n_dev, GC forwards, backwards, equal, thrice in a call, over four tiles and
    across the wrap, RESET, every kind of lookup range and cap cut, relocate with garbage, 1 and 4,096 bins, compact
    with none, half and all rows dead, and 274 tiles of rows - with garbage in the scratch and every buffer of its exact
    size under AddressSanitizer.  A stand-alone program: nothing is loaded into Python."""
    exe = str(tmp_path / "logindex_emulation")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-pthread", "-Wno-unknown-pragmas", "-Wno-deprecated", "-I", os.path.join(ROOT, "gigapaxos_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "logindex_emulation.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == "checks: 95" and len(lines) == 96 and all(": ok" in ln for ln in lines[:-1]), out.stdout
