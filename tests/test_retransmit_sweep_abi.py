"""The retransmission sweep (include/gpx_timers.h), the part that needs no GPU: the header, the exported symbols, the
binding, the JNI twin and the build lists; the argument checks, which come before any device work and before the handle
is used; and the kernels in lockstep emulation under AddressSanitizer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import timers_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEPS = ("gpx_retransmit_sweep", "gpx_retransmit_sweep_dev")
ENTRY_POINTS = SWEEPS + ("gpx_rtx_backoff_table",)
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from gigapaxos_amd import load_hip

    return load_hip()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx_timers.h")).read(), flags=re.S)


def test_header_library_binding_and_jni_agree(lib):
    from gigapaxos_amd import _abi, timers

    src = header()
    assert set(re.findall(r"\b(gpx_[a-z_]+)\s*\(", src)) == set(ENTRY_POINTS)
    raw = ctypes.CDLL(lib.path)
    for name in SWEEPS:
        assert hasattr(raw, name), name
        assert name[4:] in _abi.EXPORTED_SYMBOLS and name[4:] in _abi._DEV_SIGS and name[4:] in lib.fn
        assert callable(getattr(timers, name[4:]))
        # eighteen arguments in the header, seventeen after the handle in the binding
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(args) == 18 and len(_abi._DEV_SIGS[name[4:]]) == 17
    assert hasattr(raw, "gpx_rtx_backoff_table") and "rtx_backoff_table" in _abi.EXPORTED_SYMBOLS
    assert "rtx_backoff_table" in _abi._HOST_SIGS and callable(timers.backoff_table)
    # this call has no twin in the oracle and adds nothing to the two headers whose symbols need one
    for hdr in ("gpx.h", "gpx_wire.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", hdr)).read(), flags=re.S)
        assert "retransmit_sweep" not in text and "rtx" not in text
    assert ctypes.sizeof(timers.RtxCounts) == 16 == timers.COUNTS_BYTES
    assert [f for f, _ in timers.RtxCounts._fields_] == ["n_hits", "n_nogroup", "n_waiting", "n_fired"]
    assert re.search(r"int32_t n_hits;.*int32_t n_nogroup;.*int32_t n_waiting;.*int32_t n_fired;", src, flags=re.S)
    assert ctypes.sizeof(timers.RtxCfg) == 260 and [f for f, _ in timers.RtxCfg._fields_] == ["n_steps", "accept_ms", "prepare_ms"]
    assert re.search(r"int32_t n_steps;.*int32_t accept_ms\[GPX_RTX_MAX_STEPS\];.*int32_t prepare_ms\[GPX_RTX_MAX_STEPS\];",
                     src, flags=re.S)
    assert int(re.search(r"#define GPX_RTX_MAX_STEPS (\d+)", src).group(1)) == timers.RTX_MAX_STEPS == M.MAX_STEPS == 32
    assert int(re.search(r"#define GPX_RTX_PEEK (\d+)", src).group(1)) == timers.RTX_PEEK == M.PEEK == 1
    assert timers.HIT_BYTES == 31 and [c for c, _ in timers.RTX_COLS] == list(M.OUT_COLS)
    # the deviation from the reference's initTime stands where a reader of the header sees it
    full = open(os.path.join(ROOT, "include", "gpx_timers.h")).read()
    assert "DEVIATION FROM THE REFERENCE" in full and "first sweep that SEES it" in full
    # the JNI twin: env, class, handle, then the seventeen arguments of the call; it compiles against the header (-Werror)
    shim = os.path.join(ROOT, "gigapaxos_amd", "jni", "gpx_jni.c")
    m = re.search(r"JFN\(jint, retransmitSweep\)\(([^)]*)\)", open(shim).read())
    assert m and len(m.group(1).split(",")) == 20
    subprocess.check_call(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-DGPX_HAVE_JNI", "-I",
                           os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"), shim])
    # the build lists know the header
    for f in ("Makefile", "__graft_entry__.py"):
        assert "gpx_timers.h" in open(os.path.join(ROOT, f)).read(), f


def test_argument_errors_come_before_any_device_work(lib):
    """No engine exists here (there is no GPU): every refusal below is decided from the arguments alone, the handle of
    the later cases being a block of zero bytes that no check may look into."""
    from gigapaxos_amd import timers

    blk = np.zeros(1 << 16, np.uint8)
    h = blk.ctypes.data_as(ctypes.c_void_p)
    counts = ctypes.create_string_buffer(16)
    col = np.zeros(64, np.uint64)
    p = col.ctypes.data_as(ctypes.c_void_p)
    cp = ctypes.cast(counts, ctypes.c_void_p)
    good = timers.make_cfg([100, 150], [40, 60])
    cfg = ctypes.byref(good)
    cols = [p] * 10

    def bad_cfg(n_steps, neg_accept=None, neg_prepare=None):
        c = timers.make_cfg([100, 150], [40, 60])
        c.n_steps = n_steps
        if neg_accept is not None:
            c.accept_ms[neg_accept] = -1
        if neg_prepare is not None:
            c.prepare_ms[neg_prepare] = -1
        return ctypes.byref(c)
    for name in ("retransmit_sweep", "retransmit_sweep_dev"):
        f = lib.fn[name]
        assert f(None, 4, None, 0, cfg, 0, 4, *cols, cp) == EINVAL                 # null handle
        assert f(h, 4, None, 0, None, 0, 4, *cols, cp) == EINVAL                   # null cfg
        assert f(h, 4, None, 0, cfg, 0, 4, *cols, None) == EINVAL                  # null counts
        assert f(h, 4, None, 0, cfg, 0, 0, *[None] * 10, None) == EINVAL
        assert f(h, -1, None, 0, cfg, 0, 4, *cols, cp) == EINVAL                   # negative n
        assert f(h, 4, None, 0, cfg, 0, -1, *cols, cp) == EINVAL                   # negative cap
        for n_steps in (0, -1, 33, 1 << 30):                                        # n_steps outside 1 .. 32
            assert f(h, 4, None, 0, bad_cfg(n_steps), 0, 4, *cols, cp) == EINVAL
        assert f(h, 4, None, 0, bad_cfg(2, neg_accept=1), 0, 4, *cols, cp) == EINVAL      # a negative threshold
        assert f(h, 4, None, 0, bad_cfg(2, neg_prepare=0), 0, 4, *cols, cp) == EINVAL
        for flags in (2, 4, 3, -1, 1 << 30):                                        # unknown flag bits
            assert f(h, 4, None, 0, cfg, flags, 4, *cols, cp) == EINVAL
        for k in range(10):                                                         # cap > 0 with a null column
            assert f(h, 4, None, 0, cfg, 0, 4, *[None if q == k else p for q in range(10)], cp) == EINVAL
    assert not blk.any() and counts.raw == bytes(16) and not col.any()
    assert good.n_steps == 2 and list(good.accept_ms[:2]) == [100, 150]


def test_rtx_kernels_in_lockstep_emulation_under_asan(tmp_path):
    """tests/timers_emulation.cpp: the kernels of gpx_timers.hip.h as they are, one thread per lane, over a stand-in
    poke_scan_row - every hit set on tile edges, peeks, cap cuts continued on the next call, saturation, the clock
    wrapping and stepping back, a listed sweep and 258 tiles - with garbage in the scratch and every buffer of its exact
    size under AddressSanitizer.  A stand-alone program: nothing is loaded into Python."""
    exe = str(tmp_path / "timers_emulation")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-pthread", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "gigapaxos_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "timers_emulation.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 49 and all(": ok" in ln for ln in lines), out.stdout
