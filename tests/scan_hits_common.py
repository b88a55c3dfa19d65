"""Scenarios of the hit-compacting scans (include/gpx_scan.h): engines whose hits sit where a test wants them, by
construction.  Every builder runs unchanged over the HIP library and over the CPU oracle; the expected answer of a scan is
always tests/scan_hits_model.py applied to the ORACLE's dense scan of the same history."""
import numpy as np

from gigapaxos_amd import Engine, hri_create, make_hri, S_OK, C_HASVALUE, C_STOP
from gigapaxos_amd import wire as W
from gigapaxos_amd.scan import SCAN_TILE, GAP_HIT_SYNC, GAP_HIT_MISSING, GAP_HIT_AHEAD
from tests import scan_hits_model as M

T = SCAN_TILE
G = 3 * T + 17                     # the last tile is partial
SPARE = 8                          # groups G .. G + SPARE - 1 of every engine: never created, or created and retired
INT_MAX = 2**31 - 1
ME, MEMBERS = 101, (100, 101, 102)
SET_NAMES = ("none", "all", "edges", "hole", "sparse")
# (threshold, mode, limit) of tests/host_rows_common.gap_run
GAP_SETTINGS = ((1, W.SYNC_DEFAULT, 64), (5, W.SYNC_DEFAULT, 4), (400, W.SYNC_TO_PAUSE, 64), (1000, W.SYNC_FORCE, 64))
GAP_REQUIRES = (0, GAP_HIT_SYNC, GAP_HIT_SYNC | GAP_HIT_MISSING, GAP_HIT_AHEAD)


def hit_set(name, n_groups=G):
    if name == "none":
        return np.zeros(0, np.int64)
    if name == "all":
        return np.arange(n_groups)
    if name == "edges":
        return np.array([0, 63, 64, 255, 256, T - 1, T, 2 * T - 1, 2 * T, 3 * T, 3 * T + 16])
    if name == "hole":                               # tiles 0 and 2 full, tile 1 empty: offsets carry across it
        return np.concatenate([np.arange(0, T), np.arange(2 * T, 3 * T)])
    assert name == "sparse"
    s = np.nonzero(np.random.default_rng(97).random(n_groups) < 1 / 97)[0]
    assert s.size > 3
    return s


def _engine(lib, my_id, n_groups, kmax, window):
    return Engine(lib, my_id, n_groups + SPARE, kmax=kmax, window=window, max_batch=max(n_groups + SPARE, 1 << 12))


def _members(n, kmax, k=3):
    mem = np.zeros((n, kmax), np.int32)
    mem[:, :k] = np.arange(100, 100 + k)
    return mem


def _spares(e, n_groups, kmax, k=3):
    """group n_groups + 2 is created and retired again; the other spare groups never exist"""
    g = np.array([n_groups + 2], np.int32)
    assert (e.create_groups(g, _members(1, kmax, k), k, hri_create(1, k, 100)) == S_OK).all()
    e.retire_groups(g)


# ---- election: my_id 101 of {100, 101, 102}; node 100 is down ------------------------------------------------------------
ELECTION_DOWN = (100,)


def election_engine(lib, hits, n_groups=G, mine=0):
    """Groups in `hits` have acceptor ballot coordinator 100 (down, and 101 is next in line: RUN_NEXT), the others 102.
    `mine` > 0: every mine-th group of the set has coordinator 101 itself and no coordinator object (RUN_MINE)."""
    e = _engine(lib, ME, n_groups, 3, 8)
    rows = hri_create(n_groups, 3, 102)
    rows["acc_bcoord"][hits] = 100
    rows["coord_bcoord"][hits] = 100
    rows["acc_bnum"] = np.arange(n_groups) % 5
    rows["acc_slot"] = 1 + np.arange(n_groups) % 7
    if mine and len(hits):
        own = np.asarray(hits)[::mine]
        rows["acc_bcoord"][own] = ME
        rows["has_coord"][own] = 0
    assert (e.create_groups(np.arange(n_groups), _members(n_groups, 3), 3, rows) == S_OK).all()
    _spares(e, n_groups, 3)
    return e


def election_dense(eo, gidx, n, force=False, down=ELECTION_DOWN, long_dead=()):
    g = np.arange(n, dtype=np.int32) if gidx is None else gidx
    return W.election_scan(W.WireEngine(eo), g, down, long_dead, force)


MULTI_SETS = ("sparse", "edges", "hole")


def election_multi_engine(lib, n_groups=G):
    """ONE engine for several hit sets: the ballot coordinator of a group is a node outside the group, 200 + a bit per
    set of MULTI_SETS the group belongs to (102, which stays up, for groups in none).  A scan with the ids of one set down
    and long dead hits exactly that set (RUN_LONGDEAD); with nobody down nothing; with force everything."""
    e = _engine(lib, ME, n_groups, 3, 8)
    mask = np.zeros(n_groups, np.int32)
    for b, name in enumerate(MULTI_SETS):
        mask[hit_set(name, n_groups)] |= 1 << b
    rows = hri_create(n_groups, 3, 102)
    rows["acc_bcoord"] = np.where(mask > 0, 200 + mask, 102)
    rows["coord_bcoord"] = rows["acc_bcoord"]
    rows["acc_bnum"] = np.arange(n_groups) % 3
    rows["acc_slot"] = 1 + np.arange(n_groups) % 5
    assert (e.create_groups(np.arange(n_groups), _members(n_groups, 3), 3, rows) == S_OK).all()
    _spares(e, n_groups, 3)
    return e


def multi_params(name):
    """(down_nodes, long_dead_nodes, force) that make `name` the hit set of an election_multi_engine"""
    if name == "all":
        return (), (), True
    if name == "none":
        return (), (), False
    bit = 1 << MULTI_SETS.index(name)
    ids = tuple(200 + m for m in range(1, 1 << len(MULTI_SETS)) if m & bit)
    return ids, ids, False


# ---- poke: my_id 100 coordinates every group ----------------------------------------------------------------------------
def poke_engine(lib, hits, n_groups=G, kmax=3, k=3, window=8):
    """A proposal outstanding on the groups of the set (POKE_ACCEPT; one of them a stop request), election_begin at
    ballot 1 on every third of them instead (POKE_PREPARE).  node_slots differ per group: median_cp is not trivial."""
    e = _engine(lib, 100, n_groups, kmax, window)
    rows = hri_create(n_groups, k, 100)
    rows["node_slots"][:, :k] = (np.arange(n_groups)[:, None] * 7 + np.arange(k)[None, :] * 3) % 5
    assert (e.create_groups(np.arange(n_groups), _members(n_groups, kmax, k), k, rows) == S_OK).all()
    _spares(e, n_groups, kmax, k)
    hits = np.asarray(hits, np.int32)
    prep, acc = hits[2::3], np.setdiff1d(hits, hits[2::3]).astype(np.int32)
    if acc.size:
        stop = np.zeros(acc.size, np.uint8)
        stop[acc.size // 2] = 1
        assert (e.propose(acc, stop)[4] == S_OK).all()
    if prep.size:
        assert (e.election_begin(prep, np.ones(prep.size, np.int32)) == 0).all()   # GPX_EB_PREPARING
    return e


def poke_dense(eo, gidx, n):
    return eo.poke_scan(np.arange(n, dtype=np.int32) if gidx is None else gidx)


# ---- gap: a valued commit at slot 2 while slot 0 is open ------------------------------------------------------------------
def gap_engine(lib, hits, n_groups=G, window=8):
    """Every group starts at slot 0.  Groups of the set get a decision for slot 2 (slots 0 and 1 missing); every 7th of
    them (from the second) is stopped instead by a stop decision at slot 0, and every 7th (from the third) sits two
    slots before Integer.MAX_VALUE, so that its window and its commit cross the wrap."""
    e = _engine(lib, 100, n_groups, 3, window)
    hits = np.asarray(hits, np.int64)
    stopped, wrap = hits[1::7], hits[2::7]
    rows = hri_create(n_groups, 3, 100)
    rows["acc_slot"] = 0
    rows["next_proposal_slot"] = 0
    rows["acc_slot"][wrap] = INT_MAX - 1
    rows["acc_gc_slot"][wrap] = INT_MAX - 2
    rows["next_proposal_slot"][wrap] = INT_MAX - 1
    assert (e.create_groups(np.arange(n_groups), _members(n_groups, 3), 3, rows) == S_OK).all()
    _spares(e, n_groups, 3)
    g = np.setdiff1d(hits, stopped).astype(np.int32)
    if g.size:
        slot = (rows["acc_slot"][g].astype(np.int64) + 2 + 2**31) % 2**32 - 2**31
        z = np.zeros(g.size, np.int32)
        st, _ = e.commit(g, z, np.full(g.size, 100, np.int32), slot.astype(np.int32), z, np.full(g.size, C_HASVALUE, np.uint8))
        assert (st == S_OK).all()
    if stopped.size:
        g = stopped.astype(np.int32)
        z = np.zeros(g.size, np.int32)
        st, _ = e.commit(g, z, np.full(g.size, 100, np.int32), z, z, np.full(g.size, C_HASVALUE | C_STOP, np.uint8))
        assert (st == S_OK).all()
    return e, np.setdiff1d(hits, stopped)


def gap_dense(eo, gidx, n, setting):
    g = np.arange(n, dtype=np.int32) if gidx is None else gidx
    return W.gap_scan(W.WireEngine(eo), g, *setting)


def listed(n_groups=G, seed=5):
    """A scanned list whose length is no multiple of 64: every third group in shuffled order, duplicates, -1, the first
    index beyond the table, groups never created and the retired one."""
    rng = np.random.default_rng(seed)
    g = rng.permutation(np.arange(0, n_groups, 3))
    extra = np.array([-1, n_groups + SPARE, n_groups, n_groups + 1, n_groups + 2, 0, 0, T, T, -1])
    out = np.concatenate([g[:500], extra, g[500:], g[:37]]).astype(np.int32)
    assert out.shape[0] % 64 != 0
    return out


def same(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), f"{what}: column {k}"


__all__ = ["M", "make_hri"]
