"""The hit-compacting scans (include/gpx_scan.h), the part that needs no GPU: the header, the exported symbols and the
binding; the argument checks, which come before any device work and before the handle is used; the numpy model against
hand-written answers; and the proof, on the CPU oracle alone, that every scenario of tests/test_scan_hits_gpu.py has
exactly the hits it was built for."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import scan_hits_common as SC
from tests import scan_hits_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCANS = ("gpx_election_scan_hits", "gpx_poke_scan_hits", "gpx_gap_scan_hits")
ENTRY_POINTS = SCANS + tuple(s + "_dev" for s in SCANS) + ("gpx_election_begin_hits_dev",)
EINVAL, ECAPACITY = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from gigapaxos_amd import load_hip

    return load_hip()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx_scan.h")).read(), flags=re.S)


def test_header_library_and_binding_agree(lib):
    from gigapaxos_amd import _abi, scan

    src = header()
    declared = set(re.findall(r"\b(gpx_[a-z_]+)\s*\(", src))
    assert declared == set(ENTRY_POINTS)
    names = declared | {"gpx_scan_counts", "GPX_SCAN_TILE", "GPX_GAP_HIT_SYNC", "GPX_GAP_HIT_MISSING", "GPX_GAP_HIT_AHEAD"}
    for hdr in ("gpx.h", "gpx_wire.h", "gpx_packed.h", "gpx_packed_out.h"):
        other = open(os.path.join(ROOT, "include", hdr)).read()
        assert not any(re.search(r"\b%s\b" % name, other) for name in names), hdr
    raw = ctypes.CDLL(lib.path)
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), name
        assert name[4:] in _abi.EXPORTED_SYMBOLS and name[4:] in _abi._DEV_SIGS and name[4:] in lib.fn
        assert callable(getattr(scan, name[4:]))
    assert ctypes.sizeof(scan.ScanCounts) == 16 == scan.COUNTS_BYTES
    assert re.search(r"int32_t n_hits;.*int32_t n_nogroup;.*int32_t reserved\[2\];", src, flags=re.S)
    assert int(re.search(r"#define GPX_SCAN_TILE (\d+)", src).group(1)) == scan.SCAN_TILE == SC.T
    for name, val in (("SYNC", scan.GAP_HIT_SYNC), ("MISSING", scan.GAP_HIT_MISSING), ("AHEAD", scan.GAP_HIT_AHEAD)):
        assert int(re.search(r"#define GPX_GAP_HIT_%s (\d+)" % name, src).group(1)) == val
    assert scan.HIT_BYTES == M.HIT_BYTES == {"election": 13, "poke": 26, "gap": 21}


def test_argument_errors_come_before_any_device_work(lib):
    """No engine exists here (there is no GPU): every refusal below is decided from the arguments alone, the handle of
    the later cases being a block of zero bytes that no check may look into."""
    fn = lib.fn
    blk = np.zeros(1 << 16, np.uint8)
    h = blk.ctypes.data_as(ctypes.c_void_p)
    counts = ctypes.create_string_buffer(16)
    col = np.zeros(8, np.uint64)
    p = col.ctypes.data_as(ctypes.c_void_p)
    cp = ctypes.cast(counts, ctypes.c_void_p)
    nodes = np.arange(17, dtype=np.int32)
    nl = nodes.ctypes.data_as(ctypes.c_void_p)
    for dev in ("", "_dev"):
        el, pk, gp = fn["election_scan_hits" + dev], fn["poke_scan_hits" + dev], fn["gap_scan_hits" + dev]
        # null handle
        assert el(None, 4, None, None, 0, None, 0, 0, 4, p, p, p, p, cp) == EINVAL
        assert pk(None, 4, None, 4, p, p, p, p, p, p, p, p, cp) == EINVAL
        assert gp(None, 4, None, 1, 0, 64, 0, 4, p, p, p, p, p, cp) == EINVAL
        # negative n, negative cap, null counts
        for n, cap, c in ((-1, 4, cp), (4, -1, cp), (4, 4, None)):
            assert el(h, n, None, None, 0, None, 0, 0, cap, p, p, p, p, c) == EINVAL
            assert pk(h, n, None, cap, p, p, p, p, p, p, p, p, c) == EINVAL
            assert gp(h, n, None, 1, 0, 64, 0, cap, p, p, p, p, p, c) == EINVAL
        # node lists: at most 16 entries, no negative length, no null list with a length
        assert el(h, 4, None, nl, 17, None, 0, 0, 4, p, p, p, p, cp) == ECAPACITY
        assert el(h, 4, None, None, 0, nl, 17, 0, 4, p, p, p, p, cp) == ECAPACITY
        assert el(h, 4, None, nl, -1, None, 0, 0, 4, p, p, p, p, cp) == EINVAL
        assert el(h, 4, None, None, 3, None, 0, 0, 4, p, p, p, p, cp) == EINVAL
        # cap > 0 with a null column, whichever it is
        for k in range(4):
            cols = [None if q == k else p for q in range(4)]
            assert el(h, 4, None, None, 0, None, 0, 0, 4, *cols, cp) == EINVAL
        for k in range(8):
            cols = [None if q == k else p for q in range(8)]
            assert pk(h, 4, None, 4, *cols, cp) == EINVAL
        for k in range(5):
            cols = [None if q == k else p for q in range(5)]
            assert gp(h, 4, None, 1, 0, 64, 0, 4, *cols, cp) == EINVAL
    bg = fn["election_begin_hits_dev"]
    assert bg(None, 4, cp, p, p, p) == EINVAL and bg(h, -1, cp, p, p, p) == EINVAL
    assert bg(h, 4, None, p, p, p) == EINVAL and bg(h, 4, cp, None, p, p) == EINVAL
    assert bg(h, 4, cp, p, None, p) == EINVAL and bg(h, 4, cp, p, p, None) == EINVAL
    assert bg(h, 0, None, None, None, None) == 0
    assert not blk.any() and counts.raw == bytes(16) and not col.any()


def test_model_against_hand_written_answers():
    g = np.arange(10, dtype=np.int32)
    # election: (run, p_bnum, p_first, status); entry 3 names no group, entry 7 runs
    run = np.array([0, 2, 0, 0, 1, 0, 0, 4, 0, 3], np.uint8)
    pb = np.array([0, 5, 0, 0, 1, 0, 0, 9, 0, 2], np.int32)
    pf = np.array([0, 7, 0, 0, 3, 0, 0, 4, 0, 8], np.int32)
    st = np.array([0, 0, 0, 1, 0, 0, 1, 0, 0, 0], np.uint8)
    cols, nh, ng = M.compact("election", (run, pb, pf, st), g + 100, 10)
    assert (nh, ng) == (4, 2)
    assert [c.tolist() for c in cols] == [[101, 104, 107, 109], [2, 1, 4, 3], [5, 1, 9, 2], [7, 3, 4, 8]]
    assert [c.dtype for c in cols] == [np.int32, np.uint8, np.int32, np.int32]
    cols, nh, ng = M.compact("election", (run, pb, pf, st), g + 100, 3)
    assert (nh, ng) == (4, 2) and cols[0].tolist() == [101, 104, 107]
    cols, nh, ng = M.compact("election", (run, pb, pf, st), g, 0)
    assert (nh, ng) == (4, 2) and all(c.shape == (0,) for c in cols)
    # a listed scan: the order of hits is the array order, duplicates stay
    lst = np.array([7, 1, 7, 3, 1, 0, 9, 9, 2, 4], np.int32)
    cols, nh, _ = M.compact("election", (run[lst], pb[lst], pf[lst], st[lst]), lst, 10)
    assert nh == 7 and cols[0].tolist() == [7, 1, 7, 1, 9, 9, 4] and cols[1].tolist() == [4, 2, 4, 2, 3, 3, 1]
    # poke: (poke, slot, bnum, bcoord, median_cp, flags, heard, status)
    pk = np.array([0, 1, 2, 0, 0, 1, 0, 0, 2, 0], np.uint8)
    dense = (pk, g * 2, g + 1, np.full(10, 100, np.int32), g - 3, (g == 5).astype(np.uint8), (g * 3).astype(np.uint32),
             np.array([0, 0, 0, 0, 1, 0, 0, 0, 1, 0], np.uint8))
    cols, nh, ng = M.compact("poke", dense, g, 10)
    assert (nh, ng) == (3, 2)            # entry 8 pokes in the columns but names no group: not a hit
    assert [c.tolist() for c in cols] == [[1, 2, 5], [1, 2, 1], [2, 4, 10], [2, 3, 6], [100] * 3, [-2, -1, 2], [0, 0, 1],
                                          [3, 6, 15]]
    # gap: (first, max_committed, missing, should_sync, status); entry 2 is stopped, entry 9 wraps
    first = np.array([0, 0, 0, 5, 5, 1, 0, 0, 0, 2**31 - 2], np.int32)
    maxc = np.array([-1, 2, 2, 4, 9, 1, 3, -1, 0, -2**31], np.int32)
    miss = np.array([0, 3, 0, 0, 7, 0, 5, 0, 0, 3], np.uint64)
    sync = np.array([1, 1, 1, 0, 1, 0, 0, 1, 0, 1], np.uint8)
    st = np.array([0, 0, 2, 0, 0, 0, 0, 1, 0, 0], np.uint8)
    d = (first, maxc, miss, sync, st)
    want = {0: [0, 1, 3, 4, 5, 6, 8, 9], M.GAP_HIT_SYNC: [0, 1, 4, 9], M.GAP_HIT_SYNC | M.GAP_HIT_MISSING: [1, 4, 9],
            M.GAP_HIT_AHEAD: [1, 4, 5, 6, 8, 9], M.GAP_HIT_MISSING | M.GAP_HIT_AHEAD: [1, 4, 6, 9], 7: [1, 4, 9]}
    for require, hits in want.items():
        cols, nh, ng = M.compact("gap", d, g, 10, require)
        assert cols[0].tolist() == hits and nh == len(hits) and ng == 1, require
        assert cols[3].dtype == np.uint64 and cols[3].tolist() == miss[hits].tolist()


# ---- oracle only: the scenarios of the GPU tests have the hits they were built for --------------------------------------
@pytest.mark.parametrize("name", SC.SET_NAMES)
def test_election_scenarios_hit_where_they_were_built_to(oracle_lib, name):
    hits = SC.hit_set(name)
    eo = SC.election_engine(oracle_lib, hits, mine=4)
    dense = SC.election_dense(eo, None, SC.G)
    assert np.nonzero(M.hit_mask("election", dense))[0].tolist() == hits.tolist()
    if hits.size:
        assert set(dense[0][hits].tolist()) == {1, 2}                       # RUN_MINE and RUN_NEXT
    forced = SC.election_dense(eo, None, SC.G + SC.SPARE, force=True)
    assert M.hit_mask("election", forced).sum() == SC.G and (forced[3] == M.S_NOGROUP).sum() == SC.SPARE
    if hits.size < SC.G:
        assert 4 in forced[0].tolist()                                       # RUN_FORCED
    lst = SC.listed()
    d = SC.election_dense(eo, lst, lst.shape[0])
    assert (d[3] == M.S_NOGROUP).sum() == 6
    eo.close()


@pytest.mark.parametrize("name", SC.SET_NAMES)
def test_poke_scenarios_hit_where_they_were_built_to(oracle_lib, name):
    hits = SC.hit_set(name)
    eo = SC.poke_engine(oracle_lib, hits)
    dense = SC.poke_dense(eo, None, SC.G)
    assert np.nonzero(M.hit_mask("poke", dense))[0].tolist() == hits.tolist()
    if hits.size:
        assert set(dense[0][hits].tolist()) == {1, 2} and dense[5].sum() == 1     # ACCEPT and PREPARE; one stop request
        assert len(set(dense[4][hits].tolist())) > 1                              # median_cp is not one value
    eo.close()


@pytest.mark.parametrize("kmax,k,window", [(3, 3, 8), (5, 5, 64), (16, 9, 8)])
def test_poke_scenarios_of_every_instantiation(oracle_lib, kmax, k, window):
    hits = SC.hit_set("sparse")
    eo = SC.poke_engine(oracle_lib, hits, kmax=kmax, k=k, window=window)
    dense = SC.poke_dense(eo, None, SC.G)
    assert np.nonzero(M.hit_mask("poke", dense))[0].tolist() == hits.tolist()
    assert len(set(dense[4][hits].tolist())) > 1
    eo.close()


@pytest.mark.parametrize("name", SC.SET_NAMES)
def test_gap_scenarios_hit_where_they_were_built_to(oracle_lib, name):
    hits = SC.hit_set(name)
    eo, live = SC.gap_engine(oracle_lib, hits)
    for setting in SC.GAP_SETTINGS:
        dense = SC.gap_dense(eo, None, SC.G, setting)
        assert (dense[4] == M.S_STOPPED).sum() == hits.size - live.size
        for require in (SC.GAP_HIT_SYNC | SC.GAP_HIT_MISSING, SC.GAP_HIT_AHEAD):
            if require & SC.GAP_HIT_SYNC and setting[0] in (5, 400):
                continue                  # a gap of 2 is below these thresholds: who syncs depends on the slot and the mode
            assert np.nonzero(M.hit_mask("gap", dense, require))[0].tolist() == live.tolist(), (setting, require)
        assert M.hit_mask("gap", dense, 0).sum() == SC.G - (hits.size - live.size)
        if live.size:
            assert dense[2][live].tolist() == [3] * live.size                  # slots 0 and 1 of the window are missing
    if hits.size > 2:                                                        # a window across Integer.MAX_VALUE
        w = hits[2]
        assert dense[0][w] == 2**31 - 2 and dense[1][w] == -2**31
    eo.close()


def test_one_engine_serves_several_hit_sets(oracle_lib):
    eo = SC.election_multi_engine(oracle_lib)
    for name in SC.SET_NAMES:
        down, long_dead, force = SC.multi_params(name)
        dense = SC.election_dense(eo, None, SC.G, force, down, long_dead)
        assert np.nonzero(M.hit_mask("election", dense))[0].tolist() == SC.hit_set(name).tolist(), name
    eo.close()


def test_compaction_kernels_in_lockstep_emulation_under_asan(tmp_path):
    """tests/scan_emulation.cpp: the kernels of gpx_scan.hip.h as they are, one thread per lane, over a stand-in
    evaluation - every hit set, short capacities, a listed scan, more tiles than one round of the offsets kernel sums,
    the counted begin - with garbage in the scratch and every buffer of its exact size under AddressSanitizer."""
    import subprocess

    exe = str(tmp_path / "scan_emulation")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-pthread", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "gigapaxos_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "scan_emulation.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 20 and all(": ok" in ln for ln in lines), out.stdout


def test_compaction_core_in_lockstep_emulation_under_asan(tmp_path):
    """tests/compact_emulation.cpp: the pieces of gpx_compact.hip.h as they are, one thread per lane, each against a
    plain loop - the per-pass tile count for 2 and 4 predicates with ragged last passes, the offsets loop for 1 to 3
    prefixed and 0 to 3 summed words at 0, 1, 255, 256, 257 and 600 tiles, the cap-cut helper with the cap at every
    position of a tile of mixed weights - every buffer of its exact size under AddressSanitizer."""
    import subprocess

    exe = str(tmp_path / "compact_emulation")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-pthread", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "gigapaxos_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "compact_emulation.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().splitlines() == ["tile_count: ok", "tile_offsets: ok", "cap_cut: ok"], out.stdout
