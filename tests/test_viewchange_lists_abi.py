"""The view change in list form (include/gpx_viewchange.h), the part that needs no GPU: the header, the exported symbols,
the `_abi` signatures, the binding, the JNI twins and the build lists agree; the structs are 32 bytes; and every
argument refusal is decided from the arguments alone, with a handle of zero bytes that no check may look into."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"gpx_prepare_lists": 17, "gpx_prepare_lists_dev": 17, "gpx_prepare_reply_lists": 29,
                "gpx_prepare_reply_lists_dev": 30, "gpx_prepare_reply_lists_more": 16, "gpx_prepare_reply_lists_more_dev": 16}
JNI_TWINS = {"prepareLists": "gpx_prepare_lists", "prepareReplyLists": "gpx_prepare_reply_lists",
             "prepareReplyListsMore": "gpx_prepare_reply_lists_more"}
EINVAL, ECAPACITY = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from gigapaxos_amd import load_hip

    return load_hip()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx_viewchange.h")).read(), flags=re.S)


def test_header_library_binding_and_jni_agree(lib):
    import gigapaxos_amd
    from gigapaxos_amd import _abi, viewchange

    src = header()
    assert set(re.findall(r"\b(gpx_[a-z_]+)\s*\(", src)) == set(ENTRY_POINTS)
    raw = ctypes.CDLL(lib.path)
    for name, nargs in ENTRY_POINTS.items():
        assert hasattr(raw, name), name
        assert name[4:] in _abi.EXPORTED_SYMBOLS and name[4:] in _abi._DEV_SIGS and name[4:] in lib.fn
        assert callable(getattr(viewchange, name[4:])) and getattr(gigapaxos_amd, name[4:]) is getattr(viewchange, name[4:])
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(args) == nargs and len(_abi._DEV_SIGS[name[4:]]) == nargs - 1, name     # the handle among them
        # the integers of the signature stand where the header has them
        ints = [i for i, a in enumerate(args[1:]) if "*" not in a]
        assert ints == [i for i, t in enumerate(_abi._DEV_SIGS[name[4:]]) if t is ctypes.c_int32], name
    assert callable(viewchange.reply_lists_all)
    assert ctypes.sizeof(viewchange.PlCounts) == 32 == ctypes.sizeof(viewchange.PrlCounts) == viewchange.COUNTS_BYTES
    assert gigapaxos_amd.PlCounts is viewchange.PlCounts and gigapaxos_amd.PrlCounts is viewchange.PrlCounts
    for struct, cls in (("gpx_pl_counts", viewchange.PlCounts), ("gpx_prl_counts", viewchange.PrlCounts)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
        assert re.findall(r"int32_t (\w+)", body) == [f for f, _ in cls._fields_], struct
    assert int(re.search(r"#define GPX_VCL_TILE\s+(\d+)", src).group(1)) == viewchange.VCL_TILE == 256
    kern = open(os.path.join(ROOT, "gigapaxos_amd", "csrc", "gpx_vclists.hip.h")).read()
    assert int(re.search(r"#define GPX_VCL_TILE_\s+(\d+)", kern).group(1)) == 256
    assert (viewchange.HIT_BYTES, viewchange.ENTRY_BYTES, viewchange.PV_BYTES) == (22, 14, 12)
    assert sum(np.dtype(dt).itemsize for _, dt in viewchange.HIT_COLS) == 22
    assert sum(np.dtype(dt).itemsize for _, dt in viewchange.ENTRY_COLS) == 14
    # the JNI twins: env, class, then the arguments of the call; they compile against the header (-Werror)
    shim = os.path.join(ROOT, "gigapaxos_amd", "jni", "gpx_jni.c")
    text = open(shim).read()
    for twin, name in JNI_TWINS.items():
        m = re.search(r"JFN\(jint, %s\)\(([^)]*)\)" % twin, text)
        assert m and len(m.group(1).split(",")) == ENTRY_POINTS[name] + 2, twin
        assert re.search(r"return %s\(H\(h\)" % name, text), twin
    subprocess.check_call(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-DGPX_HAVE_JNI", "-I",
                           os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"), shim])
    # the build lists know the header, the engine the three new files
    for f in ("Makefile", "__graft_entry__.py"):
        assert "gpx_viewchange.h" in open(os.path.join(ROOT, f)).read(), f
    eng = open(os.path.join(ROOT, "gigapaxos_amd", "csrc", "gpx_engine.hip")).read()
    for f in ("gpx_vclists.hip.h", "gpx_vclists_dev.inc", "gpx_vclists_host.inc"):
        assert '#include "%s"' % f in eng, f


def test_argument_errors_come_before_any_device_work(lib):
    """No engine exists here (there is no GPU): every refusal below is decided from the arguments alone."""
    blk = np.zeros(1 << 16, np.uint8)
    h = blk.ctypes.data_as(ctypes.c_void_p)
    counts = ctypes.create_string_buffer(32)
    col = np.zeros(64, np.uint64)
    p = col.ctypes.data_as(ctypes.c_void_p)
    cp = ctypes.cast(counts, ctypes.c_void_p)
    # ---- acceptor side: 4 inputs | 5 dense | cap | 4 list columns | counts
    for name in ("prepare_lists", "prepare_lists_dev"):
        f = lib.fn[name]
        good = [p] * 9 + [8] + [p] * 4 + [cp]
        assert f(None, 4, *good) == EINVAL                                       # null handle
        assert f(h, -1, *good) == EINVAL                                         # negative n
        a = list(good)
        a[9] = -1
        assert f(h, 4, *a) == EINVAL                                             # negative cap
        a = list(good)
        a[14] = None
        assert f(h, 4, *a) == EINVAL and f(h, 0, *a) == EINVAL                    # null counts, whatever n is
        for k in range(9):                                                       # a null input or dense column
            a = list(good)
            a[k] = None
            assert f(h, 4, *a) == EINVAL, (name, k)
        for k in (10, 11, 12, 13):                                               # cap > 0 with a null list column
            a = list(good)
            a[k] = None
            assert f(h, 4, *a) == EINVAL, (name, k)
    # ---- coordinator side
    hit, ent = [p] * 7, [p] * 4
    for name, nin in (("prepare_reply_lists", 11), ("prepare_reply_lists_dev", 12)):
        f = lib.fn[name]
        ins = [p] * 6 + ([3] if nin == 12 else []) + [p] * 5
        # (the host twin reads pv_off: zeros here, a valid column of no pvalues)
        good = ins + [p, p, 4, 32] + hit + ent + [cp]
        assert f(None, 4, *good) == EINVAL
        assert f(h, -1, *good) == EINVAL
        for k, v in ((nin + 2, -1), (nin + 3, -1)):                              # a negative cap
            a = list(good)
            a[k] = v
            assert f(h, 4, *a) == EINVAL, (name, k)
        if nin == 12:
            a = list(good)
            a[6] = -1                                                            # negative pv_total
            assert f(h, 4, *a) == EINVAL
            for k in (7, 8, 9):                                                  # pv_total > 0 with a null pvalue column
                a = list(good)
                a[k] = None
                assert f(h, 4, *a) == EINVAL, (name, k)
        a = list(good)
        a[-1] = None
        assert f(h, 4, *a) == EINVAL and f(h, 0, *a) == EINVAL                    # null counts
        for k in range(6):                                                       # a null required input
            a = list(good)
            a[k] = None
            assert f(h, 4, *a) == EINVAL, (name, k)
        for k in range(nin + 4, nin + 4 + 11):                                   # a cap > 0 with a null column
            a = list(good)
            a[k] = None
            assert f(h, 4, *a) == EINVAL, (name, k)
        for k in (nin, nin + 1):                                                 # v_kind / status are optional: the next
            a = list(good)                                                       # refusal decides (null counts)
            a[k], a[-1] = None, None
            assert f(h, 4, *a) == EINVAL
    bad_off = np.array([1, 1, 1, 1, 1], np.int32)                                # the host twin: pv_off[0] != 0, descending
    desc = np.array([0, 2, 1, 2, 2], np.int32)
    for off in (bad_off, desc):
        a = [p] * 5 + [off.ctypes.data_as(ctypes.c_void_p)] + [p] * 5 + [p, p, 4, 32] + hit + ent + [cp]
        assert lib.fn["prepare_reply_lists"](h, 4, *a) == EINVAL
    for name in ("prepare_reply_lists_more", "prepare_reply_lists_more_dev"):
        f = lib.fn[name]
        good = [0, 4, 32] + hit + ent + [cp]
        assert f(None, *good) == EINVAL
        for k in (0, 1, 2):                                                      # negative from_hit or cap
            a = list(good)
            a[k] = -1
            assert f(h, *a) == EINVAL, (name, k)
        for k in range(3, 15):                                                   # a null column or counts
            a = list(good)
            a[k] = None
            assert f(h, *a) == EINVAL, (name, k)
    assert not blk.any() and counts.raw == bytes(32) and not col.any()
