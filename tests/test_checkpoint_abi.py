"""Checkpoint transfer (include/gpx_checkpoint.h), the part that needs no GPU: the header, the exported symbols, the
binding and the JNI twin; the argument checks, which come before any device work and before the handle is used; and the
three kernels of gpx_checkpoint.hip.h in lockstep emulation under AddressSanitizer against the Java reading
(tests/checkpoint_model.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import checkpoint_model as M
from tests.acc_enum_common import COORD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("gpx_checkpoint_batch", "gpx_checkpoint_batch_dev")
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from gigapaxos_amd import load_hip

    return load_hip()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx_checkpoint.h")).read(), flags=re.S)


def test_header_library_binding_and_jni_agree(lib):
    import gigapaxos_amd
    from gigapaxos_amd import _abi, checkpoint

    src = header()
    assert set(re.findall(r"\b(gpx_[a-z_]+)\s*\(", src)) == set(ENTRY_POINTS)
    raw = ctypes.CDLL(lib.path)
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), name
        assert name[4:] in _abi.EXPORTED_SYMBOLS and name[4:] in _abi._DEV_SIGS and name[4:] in lib.fn
        assert callable(getattr(checkpoint, name[4:])) and getattr(gigapaxos_amd, name[4:]) is getattr(checkpoint, name[4:])
        # thirteen arguments in the header, the handle among them: twelve after the handle in the binding
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(args) == 13 and len(_abi._DEV_SIGS[name[4:]]) == 12
    assert ctypes.sizeof(checkpoint.CpCounts) == 16 == checkpoint.COUNTS_BYTES and gigapaxos_amd.CpCounts is checkpoint.CpCounts
    assert [f for f, _ in checkpoint.CpCounts._fields_] == ["n_adopted", "n_nogroup", "n_stopped", "n_runs"]
    assert re.search(r"int32_t n_adopted;.*int32_t n_nogroup;.*int32_t n_stopped;.*int32_t n_runs;", src, flags=re.S)
    assert int(re.search(r"#define GPX_CP_PEEK\s+(\d+)", src).group(1)) == checkpoint.CP_PEEK == M.CP_PEEK == 1
    assert int(re.search(r"#define GPX_CP_ADOPT\s+(\d+)", src).group(1)) == checkpoint.CP_ADOPT == M.CP_ADOPT == 1
    assert int(re.search(r"#define GPX_CP_MOVED\s+(\d+)", src).group(1)) == checkpoint.CP_MOVED == M.CP_MOVED == 2
    assert (checkpoint.IN_BYTES, checkpoint.OUT_BYTES, checkpoint.RUN_BYTES) == (8, 10, 12)
    # the JNI twin: env, class, handle, then the twelve other arguments of the call; it compiles against the header (-Werror)
    shim = os.path.join(ROOT, "gigapaxos_amd", "jni", "gpx_jni.c")
    m = re.search(r"JFN\(jint, checkpointBatch\)\(([^)]*)\)", open(shim).read())
    assert m and len(m.group(1).split(",")) == 15
    subprocess.check_call(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-DGPX_HAVE_JNI", "-I",
                           os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"), shim])
    # the build lists know the header
    for f in ("Makefile", "__graft_entry__.py"):
        assert "gpx_checkpoint.h" in open(os.path.join(ROOT, f)).read(), f


def test_argument_errors_come_before_any_device_work(lib):
    """No engine exists here (there is no GPU): every refusal below is decided from the arguments alone, the handle of
    the later cases being a block of zero bytes that no check may look into."""
    blk = np.zeros(1 << 16, np.uint8)
    h = blk.ctypes.data_as(ctypes.c_void_p)
    counts = ctypes.create_string_buffer(16)
    col = np.zeros(64, np.uint64)
    p = col.ctypes.data_as(ctypes.c_void_p)
    cp = ctypes.cast(counts, ctypes.c_void_p)
    for name in ("checkpoint_batch", "checkpoint_batch_dev"):
        f = lib.fn[name]
        good = [p] * 2 + [0] + [p] * 7 + [cp]                                    # gidx cp flags | 4 dense | 3 runs | counts
        assert f(None, 4, *good) == EINVAL                                       # null handle
        assert f(h, -1, *good) == EINVAL                                         # negative n
        for flags in (2, 4, 3, -1, 1 << 30):                                     # unknown flag bits
            assert f(h, 4, p, p, flags, *[p] * 7, cp) == EINVAL
        for k in (0, 1, 3, 4, 5, 6, 10):                                         # a null input, dense column or counts
            for peek in (0, 1):
                a = list(good)
                a[k], a[2] = None, peek
                assert f(h, 4, *a) == EINVAL, (name, k, peek)
        for k in (7, 8, 9):                                                      # a null run column without PEEK
            a = list(good)
            a[k] = None
            assert f(h, 4, *a) == EINVAL, (name, k)
        assert f(h, 0, None, None, 0, *[p] * 7, cp) == EINVAL                    # ... whatever n is
    assert not blk.any() and counts.raw == bytes(16) and not col.any()


# ---- the kernels in lockstep emulation ----------------------------------------------------------------------------------
def models_before_first_checkpoint(W, from_disk, n):
    """n (model, cp): the groups of the enumeration plan as their first checkpoint record finds them, then states no
    handler sequence reaches, then stopped groups"""
    out = []
    for seq in M.enum_sequences(W, n=n - 40):
        m = M.CpAcceptor(1, (0, COORD), -1, from_disk, W)
        for op in seq:
            if op[0] == "J":
                out.append((m, op[1]))
                break
            M.expected(m, op, W)
    hi, lo = M.WRAP_STARTS
    for start, cp in ((hi, M.INT_MAX), (hi, M.INT_MIN + 5), (lo, 5), (lo, M.INT_MAX - 1), (hi, hi - 1), (lo, lo)):
        m = M.CpAcceptor(start, (0, COORD), start - 2, from_disk, W)     # the int wrap: both oddities, target MIN_VALUE
        M.expected(m, ("D", int(M.I32(start) + 2), 0, start - 2, 0), W)  # ... with a commit parked two slots on
        out.append((m, cp))
    while len(out) < n - 8:
        case = M.STATE_CASES[len(out) % len(M.STATE_CASES)]
        out.append((M.state_model(case, W, from_disk), case[4]))
    while len(out) < n:
        m = M.CpAcceptor(3, (0, COORD), 1, from_disk, W)
        m.stopped = True
        out.append((m, 7))
    return out


def leg_words(W, from_disk, G, calls, dead=(), seed=0):
    """one leg of the case file: a table of G groups (those in `dead` do not exist), then for each call (n, peek, extra
    records that name no group) the records, the model's answers and - unless the call peeks - the table afterwards.
    A record goes to each of the first n groups in a seeded order (distinct within a call)."""
    base = models_before_first_checkpoint(W, from_disk, min(G, 600))
    pairs = []
    for g in range(G):                                            # a larger table repeats the states
        m0, cp = base[g % len(base)]
        m = M.CpAcceptor(m0._slot, m0.ballot, m0.acceptedGCSlot, from_disk, W)
        m.accepted, m.committed, m.stopped = dict(m0.accepted), dict(m0.committed), m0.stopped
        pairs.append((m, cp))
    live = [g not in dead for g in range(G)]
    models = [m for m, _ in pairs]
    words = [G, W, 1 if from_disk else 0] + M.table_words(models, live, W)
    words += [max([n + len(extra) for n, _, extra in calls] + [0]), len(calls)]
    order = np.random.default_rng(seed).permutation(G).tolist()
    for n, peek, extra in calls:
        recs = [(g, pairs[g][1]) for g in order[:n]] + [(g, 5) for g in extra]
        np.random.default_rng(seed + 1).shuffle(recs)
        words += [len(recs), peek] + [x for r in recs for x in r]
        runs, counts = [], [0, 0, 0, 0]
        for g, cp in recs:
            if not (0 <= g < G) or not live[g]:
                words += [M.S_NOGROUP, 0, 0, 0]
                counts[1] += 1
                continue
            m = models[g]
            if peek:
                st, adopt, frm, to = m.peekCheckpoint(cp)
            else:
                st, adopt, frm, to, run = m.handleCheckpoint(cp)
                if run is not None:
                    runs.append((g, int(run[0]), int(run[1])))
            fl = (M.CP_ADOPT if adopt else 0) | (M.CP_MOVED if st == 0 and to != frm else 0)
            words += [st, frm, to, fl]
            counts[0] += bool(adopt)
            counts[2] += st == M.S_STOPPED
        counts[3] = len(runs)
        words += [len(runs)] + [x for r in runs for x in r] + counts
        if not peek:
            words += M.table_words(models, live, W)
    return words


def test_checkpoint_kernels_in_lockstep_emulation_under_asan(tmp_path):
    """tests/checkpoint_emulation.cpp: the kernels of gpx_checkpoint.hip.h as they are, one thread per lane, against the
    Java reading - n = 0, 1, 255, 256, 257 and 258 tiles, every status (dead and out-of-range groups, stopped ones), the int wrap, a peek
    before every applying call that may change no byte of state, windows 4, 8 and 64 with the accepts flag on and off -
    with garbage in the scratch and every buffer of its exact size under AddressSanitizer.  A stand-alone program:
    nothing is loaded into Python."""
    exe = str(tmp_path / "checkpoint_emulation")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-pthread", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "gigapaxos_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "checkpoint_emulation.cpp")])
    M.reset_coverage()
    legs = []
    for W, fd in ((8, True), (4, False), (64, True), (4, True), (8, False), (64, False)):
        dead = {3, 64, 255, 256, 511, 599}
        calls = [(0, 1, []), (0, 0, []), (1, 1, []), (1, 0, []), (255, 1, [-1]), (255, 0, []), (256, 1, []), (257, 1, [600, -7]),
                 (600, 1, [])]
        legs.append(leg_words(W, fd, 600, calls, dead, seed=W))
        legs.append(leg_words(W, fd, 600, [(256, 0, [])], dead, seed=W + 1))
        legs.append(leg_words(W, fd, 600, [(257, 1, [2**31 - 1]), (257, 0, [2**31 - 1, -2**31])], dead, seed=W + 2))
        legs.append(leg_words(W, fd, 600, [(600, 0, [600])], dead, seed=W + 3))
    big = 258 * 256
    legs.append(leg_words(8, True, big - 2, [(big - 2, 1, [-1, big]), (big - 2, 0, [-1, big])], {0, 255, 256, 70, big - 3}, seed=9))
    zero = [k for k, v in M.CP_COVERAGE.items() if v == 0]
    assert not zero, zero
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        f.write(f"{len(legs)}\n")
        for lw in legs:
            f.write(" ".join(str(int(x)) for x in lw) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 6 * (9 + 1 + 2 + 1) + 2 and all(": ok" in ln for ln in lines), out.stdout[-3000:]
    assert "n 66048," in lines[-1] and "(peek)" in lines[-2]
