"""The deactivation sweep (include/gpx_sweep.h), the part that needs no GPU: the header, the exported symbols, the binding
and the JNI twin; the argument checks, which come before any device work and before the handle is used; the numpy model
(tests/sweep_model.py) against hand-written answers; the kernels in lockstep emulation under AddressSanitizer; and the
proof, on the CPU oracle alone, that the histories of tests/test_pause_sweep_gpu.py change the dump of every group they
touch."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import sweep_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("gpx_pause_sweep", "gpx_pause_sweep_dev")
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from gigapaxos_amd import load_hip

    return load_hip()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx_sweep.h")).read(), flags=re.S)


def test_header_library_binding_and_jni_agree(lib):
    from gigapaxos_amd import _abi, sweep

    src = header()
    assert set(re.findall(r"\b(gpx_[a-z_]+)\s*\(", src)) == set(ENTRY_POINTS)
    raw = ctypes.CDLL(lib.path)
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), name
        assert name[4:] in _abi.EXPORTED_SYMBOLS and name[4:] in _abi._DEV_SIGS and name[4:] in lib.fn
        assert callable(getattr(sweep, name[4:]))
        # ten arguments in the header, nine after the handle in the binding
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(args) == 10 and len(_abi._DEV_SIGS[name[4:]]) == 9
    assert ctypes.sizeof(sweep.SweepCounts) == 16 == sweep.COUNTS_BYTES
    assert [f for f, _ in sweep.SweepCounts._fields_] == ["n_hits", "n_nogroup", "n_busy", "n_paused"]
    assert re.search(r"int32_t n_hits;.*int32_t n_nogroup;.*int32_t n_busy;.*int32_t n_paused;", src, flags=re.S)
    assert int(re.search(r"#define GPX_SWEEP_PEEK (\d+)", src).group(1)) == sweep.SWEEP_PEEK == M.PEEK == 1
    assert int(re.search(r"#define GPX_SWEEP_HOLD (\d+)", src).group(1)) == sweep.SWEEP_HOLD == M.HOLD == 2
    assert sweep.HIT_BYTES == 105
    # the JNI twin: env, class, handle, then the nine arguments of the call; it compiles against the header (-Werror)
    shim = os.path.join(ROOT, "gigapaxos_amd", "jni", "gpx_jni.c")
    m = re.search(r"JFN\(jint, pauseSweep\)\(([^)]*)\)", open(shim).read())
    assert m and len(m.group(1).split(",")) == 12
    subprocess.check_call(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-DGPX_HAVE_JNI", "-I",
                           os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"), shim])
    # the build lists know the header
    for f in ("Makefile", "__graft_entry__.py"):
        assert "gpx_sweep.h" in open(os.path.join(ROOT, f)).read(), f


def test_argument_errors_come_before_any_device_work(lib):
    """No engine exists here (there is no GPU): every refusal below is decided from the arguments alone, the handle of
    the later cases being a block of zero bytes that no check may look into."""
    blk = np.zeros(1 << 16, np.uint8)
    h = blk.ctypes.data_as(ctypes.c_void_p)
    counts = ctypes.create_string_buffer(16)
    col = np.zeros(64, np.uint64)
    p = col.ctypes.data_as(ctypes.c_void_p)
    cp = ctypes.cast(counts, ctypes.c_void_p)
    for name in ("pause_sweep", "pause_sweep_dev"):
        f = lib.fn[name]
        assert f(None, 4, None, 1, 0, 4, p, p, p, cp) == EINVAL                  # null handle
        assert f(h, -1, None, 1, 0, 4, p, p, p, cp) == EINVAL                    # negative n
        assert f(h, 4, None, 1, 0, -1, p, p, p, cp) == EINVAL                    # negative cap
        assert f(h, 4, None, -1, 0, 4, p, p, p, cp) == EINVAL                    # min_age outside 0 .. 255
        assert f(h, 4, None, 256, 0, 4, p, p, p, cp) == EINVAL
        for flags in (4, 8, 7, -1, 1 << 30):                                     # unknown flag bits
            assert f(h, 4, None, 1, flags, 4, p, p, p, cp) == EINVAL
        assert f(h, 4, None, 1, 0, 4, p, p, p, None) == EINVAL                   # null counts
        assert f(h, 4, None, 1, 0, 0, None, None, None, None) == EINVAL
        for k in range(3):                                                       # cap > 0 with a null column
            cols = [None if q == k else p for q in range(3)]
            assert f(h, 4, None, 1, 0, 4, *cols, cp) == EINVAL
    assert not blk.any() and counts.raw == bytes(16) and not col.any()


def test_model_against_hand_written_answers():
    #               dead  busy  same  same  chg   same  same(255) busy+chg
    live = np.array([0, 1, 1, 1, 1, 1, 1, 1], bool)
    busy = np.array([0, 1, 0, 0, 0, 0, 0, 1], bool)
    chg = np.array([1, 0, 0, 0, 1, 0, 0, 1], bool)
    age = np.array([3, 4, 0, 1, 9, 2, 255, 7])
    r = M.sweep(live, busy, chg, age, 2, 0, 8)
    assert r["counts"] == (3, 1, 2, 3)
    assert r["hits"].tolist() == [3, 5, 6] and r["ages"].tolist() == [2, 3, 255] and r["paused"].tolist() == [3, 5, 6]
    assert r["new_age"].tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    assert r["stored"].tolist() == [4] and r["cleared"].tolist() == [0, 3, 5, 6]
    # a short capacity: the count stays, only the first is written and paused, the others keep their new age
    r = M.sweep(live, busy, chg, age, 2, 0, 1)
    assert r["counts"] == (3, 1, 2, 1) and r["hits"].tolist() == [3] and r["paused"].tolist() == [3]
    assert r["new_age"].tolist() == [0, 0, 1, 0, 0, 3, 255, 0]
    # HOLD: unchanged groups keep their age, changed ones are reset
    r = M.sweep(live, busy, chg, age, 2, M.HOLD, 8)
    assert r["hits"].tolist() == [5, 6] and r["ages"].tolist() == [2, 255]
    assert r["new_age"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    # PEEK: the same answer as the real call, nothing paused, nothing stored
    r = M.sweep(live, busy, chg, age, 2, M.PEEK, 8)
    assert r["counts"] == (3, 1, 2, 0) and r["hits"].tolist() == [3, 5, 6] and r["paused"].size == 0
    assert r["new_age"].tolist() == age.tolist() and r["stored"].size == 0 and r["cleared"].size == 0
    # PEEK | HOLD at min_age 0 reads the ages back: every caught-up group, its stored age (0 where it changed)
    r = M.sweep(live, busy, chg, age, 0, M.PEEK | M.HOLD, 8)
    assert r["hits"].tolist() == [2, 3, 4, 5, 6] and r["ages"].tolist() == [0, 1, 0, 2, 255]
    # min_age 0 without flags: the forced pause, bounded by cap
    r = M.sweep(live, busy, chg, age, 0, 0, 2)
    assert r["counts"] == (5, 1, 2, 2) and r["paused"].tolist() == [2, 3]
    assert r["new_age"].tolist() == [0, 0, 0, 0, 0, 3, 255, 0]
    # counts only
    r = M.sweep(live, busy, chg, age, 1, 0, 0)
    assert r["counts"] == (4, 1, 2, 0) and r["hits"].size == 0


def test_sweep_kernels_in_lockstep_emulation_under_asan(tmp_path):
    """tests/sweep_emulation.cpp: the kernels of gpx_sweep.hip.h as they are, one thread per lane, over a stand-in
    evaluation - every hit set, peeks, cap cuts continued under HOLD, saturation, a forced pause, a listed sweep and 258
    tiles - with garbage in the scratch and every buffer of its exact size under AddressSanitizer.  A stand-alone
    program: nothing is loaded into Python."""
    exe = str(tmp_path / "sweep_emulation")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-pthread", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "gigapaxos_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "sweep_emulation.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 36 and all(": ok" in ln for ln in lines), out.stdout


def test_every_record_of_the_gpu_histories_changes_its_groups_dump(oracle_lib):
    """The age assertions of the GPU tests cover every group: one that received no record must age by exactly one, one
    that received records must start again at 0 - which presumes that every record of the histories changes the oracle's
    dump of its group.  Shown here on the oracle alone, for whole rounds and for bare ACCEPTs."""
    from tests import sweep_common as SC

    for from_disk in (False, True):
        eo = SC.engine(oracle_lib, 1025, from_disk=from_disk)
        before = SC.dumps(eo, 1025)
        for step in range(4):
            touched = SC.traffic(eo, 1025, step)
            after = SC.dumps(eo, 1025)
            changed = np.array([a != b for a, b in zip(before, after)])
            want = np.zeros(1025, bool)
            want[touched] = True
            assert (changed == want).all(), (from_disk, step)
            assert touched.size > 100
            before = after
        eo.close()
