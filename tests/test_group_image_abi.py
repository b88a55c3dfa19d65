"""Group images (include/gpx_image.h), the part that needs no GPU: the header, the exported symbols, the binding and the
JNI twins; gpx_image_stride against a restatement; the argument checks, which come before any device work and before the
handle is used; and the format itself - tests/image_model.py against gigapaxos_amd.image.rows_to_dumps over histories the
CPU oracle is driven through until every section of a row is in use."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import image_common as IC
from tests import image_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("gpx_image_stride", "gpx_group_export_dev", "gpx_group_export", "gpx_group_import_dev", "gpx_group_import")
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from gigapaxos_amd import load_hip

    return load_hip()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx_image.h")).read(), flags=re.S)


def test_header_library_binding_and_jni_agree(lib):
    from gigapaxos_amd import _abi, image

    src = header()
    assert set(re.findall(r"\b(gpx_[a-z_]+)\s*\(", src)) == set(ENTRY_POINTS)
    raw = ctypes.CDLL(lib.path)
    nargs = {"gpx_group_export": 7, "gpx_group_export_dev": 7, "gpx_group_import": 6, "gpx_group_import_dev": 6}
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), name
        assert name[4:] in _abi.EXPORTED_SYMBOLS and name[4:] in lib.fn
        if name in nargs:
            assert name[4:] in _abi._DEV_SIGS
            args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
            assert len(args) == nargs[name] and len(_abi._DEV_SIGS[name[4:]]) == nargs[name] - 1
    assert _abi._HOST_SIGS["image_stride"] == [ctypes.c_int32, ctypes.c_int32] and lib.fn["image_stride"].restype is ctypes.c_int64
    for f in ("image_stride", "export_groups", "export_groups_dev", "import_groups", "import_groups_dev", "rows_to_dumps",
              "move_groups"):
        assert callable(getattr(image, f)), f
    assert ctypes.sizeof(image.ImageCounts) == 16 == image.COUNTS_BYTES
    assert [f for f, _ in image.ImageCounts._fields_] == ["n_live", "n_rows", "n_done", "n_rows_done"]
    assert re.search(r"int32_t n_live;.*int32_t n_rows;.*int32_t n_done;.*int32_t n_rows_done;", src, flags=re.S)
    const = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (GPX_\w+) (0x[0-9a-fA-F]+|\d+)\b", src)}
    assert const["GPX_IMAGE_FORMAT"] == image.IMAGE_FORMAT == M.FORMAT == 1
    assert (const["GPX_IMAGE_MAIN"], const["GPX_IMAGE_CONT"]) == (image.IMAGE_MAIN, image.IMAGE_CONT) == (M.MAIN, M.CONT)
    assert const["GPX_S_IMAGE"] == image.S_IMAGE == 10
    assert (const["GPX_IMG_EVICT"], const["GPX_IMG_VIEWCHANGE"]) == (image.IMG_EVICT, image.IMG_VIEWCHANGE) == (1, 2)
    for name, a, b in (("EXISTS", image.F_EXISTS, M.EXISTS), ("STOPPED", image.F_STOPPED, M.STOPPED),
                       ("HASCOORD", image.F_HASCOORD, M.HASCOORD), ("PREPARING", image.F_PREPARING, M.PREPARING),
                       ("CONTINUED", image.F_CONTINUED, M.CONTINUED)):
        assert const["GPX_IMG_F_" + name] == a == b
    assert const["GPX_IMG_F_K_SHIFT"] == image.F_K_SHIFT == 8
    assert (const["GPX_IMG_P_PRESENT"], const["GPX_IMG_P_STOP"]) == (M.P_PRESENT, M.P_STOP) == (image.P_PRESENT, image.P_STOP)
    assert (const["GPX_IMG_R_PRESENT"], const["GPX_IMG_R_STOP"], const["GPX_IMG_R_HASVALUE"]) == (M.R_PRESENT, M.R_STOP, M.R_HASVALUE)
    assert const["GPX_IMG_CO_PRESENT"] == M.CO_PRESENT == image.CO_PRESENT
    assert const["GPX_IMAGE_TILE_ENTRIES"] == image.IMAGE_TILE   # (the library's static_assert ties it to the kernels)
    assert const["GPX_IMAGE_HEADER_WORDS"] == image.HEADER_WORDS == 16 and image.IMAGE_HEADER_DTYPE.itemsize == 64
    assert [n for n in image.IMAGE_HEADER_DTYPE.names][:8] == ["format", "kind", "flags", "my_id", "kmax", "window", "gidx", "version"]
    # the JNI twins: env, class, handle, then the arguments of the call; the shim compiles against the header (-Werror)
    shim = os.path.join(ROOT, "gigapaxos_amd", "jni", "gpx_jni.c")
    text = open(shim).read()
    for jname, n in (("groupExport", 9), ("groupImport", 8)):
        m = re.search(r"JFN\(jint, %s\)\(([^)]*)\)" % jname, text)
        assert m and len(m.group(1).split(",")) == n, jname
    subprocess.check_call(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-DGPX_HAVE_JNI", "-I",
                           os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"), shim])
    for f in ("Makefile", "__graft_entry__.py"):
        assert "gpx_image.h" in open(os.path.join(ROOT, f)).read(), f


def test_stride_against_a_restatement(lib):
    from gigapaxos_amd import image

    for kmax in range(1, 17):
        for window in (4, 8, 16, 32, 64):
            s = image.image_stride(kmax, window, lib)
            assert s == M.stride(kmax, window) == 4 * image.layout(kmax, window)["stride_w"], (kmax, window)
            assert s % 64 == 0 and s >= 4 * (16 + 2 * kmax + 9 * window) and s >= 4 * M.cont_words(window)
    assert image.image_stride(3, 8, lib) == 384
    for kmax, window in ((0, 8), (17, 8), (-1, 8), (3, 0), (3, 2), (3, 12), (3, 128), (3, -8)):
        assert image.image_stride(kmax, window, lib) == -1, (kmax, window)


def test_argument_errors_come_before_any_device_work(lib):
    """No engine exists here (there is no GPU): every refusal below is decided from the arguments alone, the handle of
    the later cases being a block of zero bytes that no check may look into."""
    blk = np.zeros(1 << 16, np.uint8)
    h = blk.ctypes.data_as(ctypes.c_void_p)
    counts = ctypes.create_string_buffer(16)
    cp = ctypes.cast(counts, ctypes.c_void_p)
    buf = np.zeros(1024, np.uint64)
    assert buf.ctypes.data % 16 == 0
    p = ctypes.c_void_p(buf.ctypes.data)
    for name in ("group_export", "group_export_dev"):
        f = lib.fn[name]
        assert f(None, 4, None, 0, 4, p, cp) == EINVAL                           # null handle
        assert f(h, -1, None, 0, 4, p, cp) == EINVAL                             # negative n
        assert f(h, 4, None, 0, -1, p, cp) == EINVAL                             # negative cap
        for flags in (2, 4, 3, -1, 1 << 30):                                     # unknown flag bits
            assert f(h, 4, None, flags, 4, p, cp) == EINVAL
        assert f(h, 4, None, 0, 4, p, None) == EINVAL                            # null counts
        assert f(h, 4, None, 0, 0, None, None) == EINVAL
        assert f(h, 4, None, 0, 4, None, cp) == EINVAL                           # cap > 0 with a null buffer
    for name in ("group_import", "group_import_dev"):
        f = lib.fn[name]
        assert f(None, 4, p, None, 0, p) == EINVAL                               # null handle
        assert f(h, -1, p, None, 0, p) == EINVAL                                 # negative n_rows
        for flags in (1, 4, 3, -1, 1 << 30):                                     # unknown flag bits
            assert f(h, 4, p, None, flags, p) == EINVAL
        assert f(h, 4, p, None, 0, None) == EINVAL                               # null status
        assert f(h, 4, None, None, 0, p) == EINVAL                               # rows to import, null buffer
    for off in (4, 8, 1):                                                        # a misaligned _dev buffer
        q = ctypes.c_void_p(buf.ctypes.data + off)
        assert lib.fn["group_export_dev"](h, 4, None, 0, 4, q, cp) == EINVAL
        assert lib.fn["group_import_dev"](h, 4, q, None, 0, p) == EINVAL
    assert not blk.any() and counts.raw == bytes(16) and not buf.any()


def test_model_hand_written_row():
    """one group by hand: K = 3, W = 8, an accepted slot 9 and a commit waiting at slot 10, one proposal with one vote"""
    dump = [1, 4, 3, 100, 101, 102, 9, 0, 100, 8, 0,
            1, 9, 0, 100, 0,
            1, 10, 0, 100, 8, 1, 0,
            1, 0, 100, 10, 8, 8, 7, 1, 9, 0, 0b010, 1]
    rows = M.row_from_dump(dump, 77, 100, 3, 8)
    assert rows.shape == (1, 384)
    w = rows.view("<i4")[0]
    assert w[:16].tolist() == [1, 1, 1 | 4 | (3 << 8), 100, 3 | (8 << 16), 77, 4, 9, 0, 100, 8, 0, 100, 10, 1, 0]
    assert w[16:22].tolist() == [100, 101, 102, 8, 8, 7]
    assert w[22:30].tolist() == [0, (1 << 16) | 2, 0, 0, 0, 0, 0, 0]
    assert w[30 + 4:30 + 8].tolist() == [9, 0, 100, 1]                        # accepted slot 9 at index 1
    assert w[30 + 8:30 + 12].tolist() == [0, 0, 0, (1 | 4) << 8]               # index 2: only the commit's flag byte
    assert w[62 + 8:62 + 12].tolist() == [10, 0, 100, 8]
    assert not w[94:].any() and int(np.count_nonzero(w)) == 13 + 3 + 3 + 1 + 3 + 1 + 3     # everything else is zero
    assert M.dump_from_rows(rows, 3, 8).tolist() == dump


HISTORIES = [dict(kmax=3, k=3, window=8), dict(kmax=3, k=1, window=8), dict(kmax=3, k=2, window=4),
             dict(kmax=16, k=16, window=8), dict(kmax=3, k=3, window=64), dict(kmax=3, k=3, window=8, base_slot=2**31 - 2)]


@pytest.mark.parametrize("kw", HISTORIES, ids=lambda kw: "-".join(f"{a}{b}" for a, b in kw.items()))
def test_model_over_oracle_histories(lib, oracle_lib, kw):
    """inverse(row_from_dump(d)) == d for every group of both halves of the history; image.rows_to_dumps agrees with
    the model's inverse; rows of equal dumps are byte-equal; every section of a row is in use somewhere"""
    from gigapaxos_amd import image

    n, kmax, k, window, base = 96, kw["kmax"], kw["k"], kw["window"], kw.get("base_slot", 1)
    e = IC.engine(oracle_lib, n, kmax, window)
    IC.create(e, np.arange(n), kmax, k, base)
    cat, dead = IC.categories(n, [0, 63, 64]), IC.dead_groups(n, [0, 63, 64])
    ctx = IC.first_half(e, n, cat, k, dead)
    where = {g: (0, g) for g in range(n)}
    seen = np.zeros(M.stride(kmax, window) // 4, bool)
    seen_cont = np.zeros_like(seen)
    by_dump = {}
    for half in range(2):
        for g in range(n):
            d = e.dump(g)
            if not d[0]:
                assert g in dead
                continue
            rows = M.row_from_dump(d, g, IC.ME, kmax, window)
            assert rows.shape[1] == image.image_stride(kmax, window, lib)
            assert M.dump_from_rows(rows, kmax, window).tolist() == d.tolist(), g
            (d2,) = image.rows_to_dumps(rows, kmax, window)
            assert d2.tolist() == d.tolist(), g
            w = rows.view("<i4")
            seen |= w[0] != 0
            if rows.shape[0] == 2:
                seen_cont |= w[1] != 0
            # equal dumps, equal bytes (but for the source gidx word)
            w0 = w.copy()
            w0[:, 5] = 0
            assert by_dump.setdefault(tuple(d.tolist()), w0.tobytes()) == w0.tobytes()
        if half == 0:
            IC.second_half(where, [e], n, cat, k, ctx, dead)
    L = image.layout(kmax, window)
    for sec, hi in (("mem", L["mem"] + k), ("ns", L["ns"] + k), ("p", L["p"] + window), ("acc", L["acc"] + 4 * window),
                    ("com", L["com"] + 4 * window)):
        assert seen[L[sec]:hi].any(), sec
    assert seen_cont[L["ph"]:L["ph"] + 2 * window].any()
    if k >= 2:                                                 # (a group of one hears of itself and is elected at once)
        assert seen_cont[6] and seen_cont[L["co"]:L["coh"]].any() and seen_cont[L["coh"]:L["ph"]].any()
    if base != 1:                                              # the instances crossed Integer.MAX_VALUE
        slots = [int(e.snapshot(np.array([g], np.int32))[0]["acc_slot"][0]) for g in range(n) if g not in dead]
        assert min(slots) < 0 < max(slots)
    e.close()
