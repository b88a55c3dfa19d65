"""The journal batches (include/gpx_journal.h), the part that needs no GPU: the header, the exported symbols, the binding,
the JNI twin and the build lists; the argument checks, which come before any device work; gpx_journal_walk against the
model; the model against the project's own FileLogger; and the kernels in lockstep emulation under AddressSanitizer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import journal_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKS = ("gpx_journal_pack", "gpx_journal_pack_dev")
ENTRY_POINTS = PACKS + ("gpx_journal_walk",)
EINVAL, ECAPACITY = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from gigapaxos_amd import load_hip

    return load_hip()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx_journal.h")).read(), flags=re.S)


def test_header_library_binding_and_jni_agree(lib):
    from gigapaxos_amd import _abi, journal

    src = header()
    assert set(re.findall(r"\b(gpx_[a-z_]+)\s*\(", src)) == set(ENTRY_POINTS)
    raw = ctypes.CDLL(lib.path)
    for name in PACKS:
        assert hasattr(raw, name), name
        assert name[4:] in _abi.EXPORTED_SYMBOLS and name[4:] in _abi._DEV_SIGS and name[4:] in lib.fn
        assert callable(getattr(journal, name[4:]))
        # twenty-seven arguments in the header, twenty-six after the handle in the binding
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        assert len(args) == 27 and len(_abi._DEV_SIGS[name[4:]]) == 26
    assert hasattr(raw, "gpx_journal_walk") and "journal_walk" in _abi._HOST_SIGS and callable(journal.journal_walk)
    assert len(re.search(r"\bgpx_journal_walk\s*\(([^)]*)\)", src).group(1).split(",")) == 8 == len(_abi._HOST_SIGS["journal_walk"])
    # this call has no twin in the oracle and adds nothing to the two headers whose symbols need one
    for hdr in ("gpx.h", "gpx_wire.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", hdr)).read(), flags=re.S)
        assert "journal" not in text
    assert ctypes.sizeof(journal.JournalCounts) == 32 == journal.COUNTS_BYTES
    assert [f for f, _ in journal.JournalCounts._fields_] == ["n_entries", "n_done", "n_bad", "reserved", "n_bytes", "bytes_done"]
    assert re.search(r"int32_t n_entries;.*int32_t n_done;.*int32_t n_bad;.*int32_t reserved;.*int64_t n_bytes;.*"
                     r"int64_t bytes_done;", src, flags=re.S)
    assert int(re.search(r"#define GPX_JR_COUNT_ONLY (\d+)", src).group(1)) == journal.JR_COUNT_ONLY == M.COUNT_ONLY == 1
    assert [c for c, _ in journal.ROW_COLS] == list(M.ROW_COLS) and journal.ROW_BYTES == 32
    # what an entry is, and what is out of scope, stand where a reader of the header sees them
    full = open(os.path.join(ROOT, "include", "gpx_journal.h")).read()
    for phrase in ("AS RECEIVED", "AcceptPacket.java:95-135", "Out of scope", "getJournaledMessage", "FileLogger::logBatch"):
        assert phrase in full, phrase
    # the JNI twin: env, class, handle, then the twenty-six arguments of the call; it compiles against the header
    shim = os.path.join(ROOT, "gigapaxos_amd", "jni", "gpx_jni.c")
    m = re.search(r"JFN\(jint, journalPack\)\(([^)]*)\)", open(shim).read())
    assert m and len(m.group(1).split(",")) == 29
    subprocess.check_call(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-DGPX_HAVE_JNI", "-I",
                           os.path.join(ROOT, "tests", "jni_stub"), "-I", os.path.join(ROOT, "include"), shim])
    # the build lists know the header
    for f in ("Makefile", "__graft_entry__.py"):
        assert "gpx_journal.h" in open(os.path.join(ROOT, f)).read(), f
    # the C struct is 32 bytes for a C compiler too
    subprocess.check_call(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c",
                           os.path.join(ROOT, "tests", "journal_sizeof.h")])


def test_argument_errors_come_before_any_device_work(lib):
    """No engine exists here (there is no GPU): every refusal below is decided from the arguments alone.  The handle of
    the later cases is a GpxConfig-shaped block - of a handle the checks read max_batch and nothing else - and every
    output is filled with a sentinel that must still be there afterwards."""
    blk = np.zeros(1 << 16, np.uint8)
    blk.view(np.int32)[4] = 64                         # struct gpx_config: max_batch is its fifth word
    h = blk.ctypes.data_as(ctypes.c_void_p)
    keep = blk.copy()
    counts = ctypes.create_string_buffer(b"\xa5" * 32, 32)
    cp = ctypes.cast(counts, ctypes.c_void_p)
    col = np.full(256, 0xA5A5A5A5A5A5A5A5, np.uint64)   # 16-byte aligned at [2:] or [0:], whichever numpy gave
    base = col.ctypes.data + (-col.ctypes.data) % 16
    p = ctypes.c_void_p(base)
    odd = [ctypes.c_void_p(base + k) for k in (1, 4, 8, 15)]

    def call(f, h=h, n=4, frames=p, fb=100, nf=4, off=p, ln=None, rf=None, g=p, s=p, bn=p, bc=p, fl=p, st=p, base_off=0,
             flags=0, out=p, cb=64, ce=4, rows=(p, p, p, p, p), eo=p, el=p, c=cp):
        return f(h, n, frames, fb, nf, off, ln, rf, g, s, bn, bc, fl, st, base_off, flags, out, cb, ce, *rows, eo, el, c)
    for name in ("journal_pack", "journal_pack_dev"):
        f = lib.fn[name]
        assert call(f, h=None) == EINVAL                                    # null handle
        assert call(f, c=None) == EINVAL                                    # null counts
        for kw in (dict(n=-1), dict(nf=-1), dict(fb=-1), dict(cb=-1), dict(ce=-1)):   # negative sizes and caps
            assert call(f, **kw) == EINVAL, kw
        for flags in (2, 4, 3, -1, 1 << 30):                                # unknown flag bits
            assert call(f, flags=flags) == EINVAL
        for kw in (dict(off=None), dict(fl=None), dict(st=None), dict(frames=None)):  # required in every call with n > 0
            assert call(f, **kw) == EINVAL, kw
            assert call(f, flags=1, **kw) == EINVAL, kw
        for kw in (dict(g=None), dict(s=None), dict(bn=None), dict(bc=None), dict(out=None), dict(eo=None), dict(el=None)):
            assert call(f, **kw) == EINVAL, kw                              # required where something is packed
        for q in odd:                                                       # out not 16-byte aligned
            assert call(f, out=q) == EINVAL
        assert call(f, n=65) == ECAPACITY                                   # n > max_batch
        assert call(f, n=65, flags=1, out=None, eo=None, el=None) == ECAPACITY
    assert (blk == keep).all() and counts.raw == b"\xa5" * 32 and (col == 0xA5A5A5A5A5A5A5A5).all()
    # the walk's own checks
    w = lib.fn["journal_walk"]
    n, good = ctypes.c_int32(7), ctypes.c_int64(7)
    args = (p, p, ctypes.byref(n), ctypes.byref(good))
    assert w(p, -1, 0, 4, *args) == EINVAL and w(None, 8, 0, 4, *args) == EINVAL and w(p, 8, 0, -1, *args) == EINVAL
    assert w(p, 8, 0, 4, None, p, ctypes.byref(n), ctypes.byref(good)) == EINVAL
    assert w(p, 8, 0, 4, p, p, None, ctypes.byref(good)) == EINVAL and w(p, 8, 0, 4, p, p, ctypes.byref(n), None) == EINVAL
    assert (n.value, good.value) == (7, 7) and (col == 0xA5A5A5A5A5A5A5A5).all()


def test_walk_against_the_model(lib):
    from gigapaxos_amd import journal as J

    rng = np.random.default_rng(2)
    frames = [bytes(rng.integers(0, 256, int(k)).astype(np.uint8)) for k in rng.integers(0, 400, 300)]
    data = M.logbatch(frames) + b"\x00\x00\x01"          # a torn prefix behind the last entry
    offs, lens, good = M.walk(data, 99)
    e_off, e_len, n, gb = J.journal_walk(data, 99, lib=lib)
    assert (e_off.tolist(), e_len.tolist(), n, gb) == (offs, lens, 300, len(data) - 3) and lens == [len(f) for f in frames]


def test_the_model_is_what_filelogger_writes(tmp_path):
    """tests/journal_logger_bytes.cpp: gpx::FileLogger itself (gpx_host.cpp, linked with the CPU oracle for the engine
    symbols it also needs) logs frames of 0, 1, 3, 4, 5 and 70,000 bytes; the file equals the model's bytes."""
    from tests.oracle_binding import build_oracle

    build_oracle()
    exe, log = str(tmp_path / "journal_logger_bytes"), str(tmp_path / "journal.log")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"), "-include",
                           os.path.join(ROOT, "tests", "host_oracle_prefix.h"), "-o", exe,
                           os.path.join(ROOT, "tests", "journal_logger_bytes.cpp"),
                           os.path.join(ROOT, "gigapaxos_amd", "host", "gpx_host.cpp"), "-L", os.path.join(ROOT, "oracle"),
                           "-lgpx_oracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    out = subprocess.run([exe, log], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "logged 6 frames" in out.stdout, out.stdout + out.stderr
    lens = [0, 1, 3, 4, 5, 70000]
    frames = [bytes((f * 31 + q * 7 + 1) % 251 for q in range(k)) for f, k in enumerate(lens)]
    block = np.frombuffer(b"".join(frames), np.uint8)
    off = np.cumsum([0] + lens)
    z = np.zeros(6, np.int32)
    p = M.pack(block, off, z, z, z, z, np.full(6, M.R_TOLOG, np.uint8), np.zeros(6, np.uint8))
    data = open(log, "rb").read()
    assert data == p.bytes == M.logbatch(frames) and len(data) == 70013 + 24
    assert M.walk(data)[1] == lens and [M.read_entry(data, int(o), k) for o, k in zip(p.rows["off"], lens)] == frames


def test_jr_kernels_in_lockstep_emulation_under_asan(tmp_path):
    """tests/journal_emulation.cpp: the kernels of gpx_journal.hip.h as they are, one thread per lane - every phase of an
    entry boundary in both frame forms, totals around one, two and three output tiles, more than 4,096 entries in a tile,
    an entry over 64 tiles, the selection with every kind of unusable frame, both caps, a cut call continued, counts
    only, n = 0, 258 tiles of records - with garbage in the scratch and every buffer of its exact size under
    AddressSanitizer.  A stand-alone program: nothing is loaded into Python."""
    exe = str(tmp_path / "journal_emulation")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-pthread", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "gigapaxos_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "journal_emulation.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 84 and all(": ok" in ln for ln in lines), out.stdout


def test_byte_run_core_in_lockstep_emulation_under_asan(tmp_path):
    """tests/bytes_emulation.cpp: the pieces of gpx_bytes.hip.h as they are, one thread per lane, each against a plain
    loop - the wave-wide search at 0, 1, 63, 64, 65, 4,096 and 4,097 positions, the LDS search, the unaligned load at the
    end of a block at each alignment, the copy skeleton under the smallest family (tile edges +- 5, 4,097 descriptors in
    a tile, a run over three tiles, every tail, more tiles than the grid, nothing), the caps helpers cut by entries and
    by bytes in tile 0 and in tile 257 - every buffer of its exact size under AddressSanitizer and UBSan.  A stand-alone
    program: nothing is loaded into Python."""
    exe = str(tmp_path / "bytes_emulation")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-pthread", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "gigapaxos_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "bytes_emulation.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().splitlines() == ["wave_search: ok", "lds_search: ok", "load4_unaligned: ok", "copy_runs: ok",
                                               "caps: ok"], out.stdout
