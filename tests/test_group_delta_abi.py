"""Delta images (include/gpx_delta.h), the part that needs no GPU: the header, the exported symbols, the binding and the
JNI twins; the argument checks, which come before any device work and before the handle is used; and the kernels in
lockstep emulation under AddressSanitizer and UBSan (tests/delta_emulation.cpp)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("gpx_group_export_delta_dev", "gpx_group_export_delta", "gpx_group_apply_delta_dev", "gpx_group_apply_delta")
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from gigapaxos_amd import load_hip

    return load_hip()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx_delta.h")).read(), flags=re.S)


def test_header_library_binding_and_jni_agree(lib, tmp_path):
    from gigapaxos_amd import _abi, image
    from tests import delta_model

    src = header()
    assert set(re.findall(r"\b(gpx_[a-z_]+)\s*\(", src)) == set(ENTRY_POINTS)
    raw = ctypes.CDLL(lib.path)
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), name
        assert name[4:] in _abi.EXPORTED_SYMBOLS and name[4:] in lib.fn and name[4:] in _abi._DEV_SIGS
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(args) == 9 and len(_abi._DEV_SIGS[name[4:]]) == 8
    for f in ("export_delta", "export_delta_dev", "apply_delta", "apply_delta_dev", "mirror_groups"):
        assert callable(getattr(image, f)), f
    # the struct: 32 bytes, the header's fields in the header's order; a C compiler agrees
    assert ctypes.sizeof(image.DeltaCounts) == 32 == image.DELTA_COUNTS_BYTES
    fields = ["n_live", "n_changed", "n_rows", "n_done", "n_rows_done", "n_gone", "n_gone_done", "reserved"]
    assert [f for f, _ in image.DeltaCounts._fields_] == fields
    assert re.findall(r"int32_t (\w+);", src) == fields
    prog = tmp_path / "size.c"
    prog.write_text('#include "gpx_delta.h"\n_Static_assert(sizeof(gpx_delta_counts) == 32, "32 bytes");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog)])
    const = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (GPX_\w+) (0x[0-9a-fA-F]+|\d+)\b", src)}
    assert (const["GPX_DELTA_EVICT"], const["GPX_DELTA_FULL"]) == (image.DELTA_EVICT, image.DELTA_FULL) == (1, 2)
    assert (delta_model.EVICT, delta_model.FULL) == (1, 2)
    assert "2^-64" in open(os.path.join(ROOT, "include", "gpx_delta.h")).read()      # the one probabilistic statement
    # the JNI twins: env, class, handle, then the arguments of the call; the shim compiles against the header (-Werror)
    shim = os.path.join(ROOT, "gigapaxos_amd", "jni", "gpx_jni.c")
    text = open(shim).read()
    for jname in ("exportDelta", "applyDelta"):
        m = re.search(r"JFN\(jint, %s\)\(([^)]*)\)" % jname, text)
        assert m and len(m.group(1).split(",")) == 11, jname
    subprocess.check_call(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-DGPX_HAVE_JNI", "-I",
                           os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"), shim])
    for f in ("Makefile", "__graft_entry__.py"):
        assert "gpx_delta.h" in open(os.path.join(ROOT, f)).read(), f


def test_argument_errors_come_before_any_device_work(lib):
    """No engine exists here (there is no GPU): every refusal below is decided from the arguments alone, the handle of
    the later cases being a block of zero bytes that no check may look into."""
    blk = np.zeros(1 << 16, np.uint8)
    h = blk.ctypes.data_as(ctypes.c_void_p)
    counts = ctypes.create_string_buffer(32)
    cp = ctypes.cast(counts, ctypes.c_void_p)
    buf = np.zeros(1024, np.uint64)
    assert buf.ctypes.data % 16 == 0
    p = ctypes.c_void_p(buf.ctypes.data)
    for name in ("group_export_delta", "group_export_delta_dev"):
        f = lib.fn[name]
        assert f(None, 4, None, 0, 4, p, 4, p, cp) == EINVAL                     # null handle
        assert f(h, -1, None, 0, 4, p, 4, p, cp) == EINVAL                       # negative n
        assert f(h, 4, None, 0, -1, p, 4, p, cp) == EINVAL                       # negative cap
        assert f(h, 4, None, 0, 4, p, -1, p, cp) == EINVAL                       # negative cap_gone
        for flags in (4, 8, 7, -1, 1 << 30):                                     # unknown flag bits
            assert f(h, 4, None, flags, 4, p, 4, p, cp) == EINVAL
        assert f(h, 4, None, 0, 4, p, 4, p, None) == EINVAL                      # null counts
        assert f(h, 4, None, 0, 0, None, 0, None, None) == EINVAL
        assert f(h, 4, None, 0, 4, None, 0, None, cp) == EINVAL                  # cap > 0 with a null buffer
        assert f(h, 4, None, 0, 0, None, 4, None, cp) == EINVAL                  # cap_gone > 0 with a null buffer
    for name in ("group_apply_delta", "group_apply_delta_dev"):
        f = lib.fn[name]
        assert f(None, 4, p, None, 0, p, 4, p, p) == EINVAL                      # null handle
        assert f(h, -1, p, None, 0, p, 4, p, p) == EINVAL                        # negative n_rows
        assert f(h, 4, p, None, 0, p, -1, p, p) == EINVAL                        # negative n_gone
        for flags in (1, 4, 3, -1, 1 << 30):                                     # unknown flag bits (GPX_IMG_VIEWCHANGE only)
            assert f(h, 4, p, None, flags, p, 4, p, p) == EINVAL
        assert f(h, 4, p, None, 0, None, 0, None, None) == EINVAL                # rows without a status column
        assert f(h, 4, None, None, 0, p, 0, None, None) == EINVAL                # rows to apply, null buffer
        assert f(h, 0, None, None, 0, None, 4, None, p) == EINVAL                # gone entries, null list
        assert f(h, 0, None, None, 0, None, 4, p, None) == EINVAL                # ... without a status column
    for off in (4, 8, 1):                                                        # a misaligned _dev buffer: 16 bytes for rows
        q = ctypes.c_void_p(buf.ctypes.data + off)
        assert lib.fn["group_export_delta_dev"](h, 4, None, 0, 4, q, 0, None, cp) == EINVAL
        assert lib.fn["group_apply_delta_dev"](h, 4, q, None, 0, p, 0, None, None) == EINVAL
    for off in (1, 2, 3):                                                        # ... 4 for the gone list
        q = ctypes.c_void_p(buf.ctypes.data + off)
        assert lib.fn["group_export_delta_dev"](h, 4, None, 0, 0, None, 4, q, cp) == EINVAL
        assert lib.fn["group_apply_delta_dev"](h, 0, None, None, 0, None, 4, q, p) == EINVAL
    assert not blk.any() and counts.raw == bytes(32) and not buf.any()


def test_delta_kernels_in_lockstep_emulation_under_asan(tmp_path):
    """tests/delta_emulation.cpp: the kernels of gpx_delta.hip.h and the functions of gpx_image.hip.h they call, as they
    are, one thread per lane, over a table with the engine's columns - every changed set on three tiles, one changed
    word per group for every word of both rows, stale words that change nothing, caps inside a tile, on a tile's edge
    and between a group's two rows, cap_gone cuts, EVICT, FULL, a listed scan, apply with replaced and refused rows and
    a gone list, at two shapes, and 258 tiles - with garbage in the scratch and every buffer of its exact size.  A
    stand-alone program: nothing is loaded into Python."""
    exe = str(tmp_path / "delta_emulation")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-pthread", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "gigapaxos_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "delta_emulation.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.strip().splitlines()
    assert lines and all(": ok" in ln for ln in lines), out.stdout[-3000:]
    for what in ("words: one word each", "between a group's two rows", "on the edge of tile 0", "cap_gone inside tile 0",
                 "evict: cut inside tile 1", "FULL", "listed: delta", "apply: replace and refuse", "258 tiles"):
        assert any(what in ln for ln in lines), what
