"""Scenarios of the deactivation sweep (include/gpx_sweep.h).  A History applies one sequence of operations to a HIP
engine and to the CPU oracle and can replay it into a scratch oracle engine; the expected answer of a sweep is
tests/sweep_model.py over the ORACLE: live and busy from orc_group_retire(PAUSE) on the scratch copy, rows from
orc_group_snapshot, changed from orc_group_dump against its value when the group's signature was last stored."""
import numpy as np

from gigapaxos_amd import Engine, hri_create, S_OK, S_NOGROUP, S_BUSY, C_HASVALUE
from tests import sweep_model as M

ME = 100
F_FROM_DISK = 1


def engine(lib, n_groups, kmax=3, k=3, window=8, from_disk=True, my_id=ME, create=True):
    e = Engine(lib, my_id, n_groups, kmax=kmax, window=window, max_batch=max(n_groups, 1 << 12),
               flags=F_FROM_DISK if from_disk else 0)
    if create:
        create_all(e, n_groups, kmax, k)
    return e


def members_of(n, kmax, k):
    mem = np.zeros((n, kmax), np.int32)
    mem[:, :k] = np.arange(ME, ME + k)
    return mem


def create_all(e, n_groups, kmax=3, k=3, groups=None):
    g = np.arange(n_groups, dtype=np.int32) if groups is None else np.asarray(groups, np.int32)
    rows = hri_create(g.size, k, ME)
    rows["node_slots"][:, :k] = (g[:, None] * 7 + np.arange(k)[None, :] * 3) % 5   # all k of them are in the row
    rows["acc_bnum"] = 0
    assert (e.create_groups(g, members_of(g.size, kmax, k), k, rows) == S_OK).all()


def whole_rounds(e, g, k=3):
    """propose, a majority of accept replies, the decision committed: the group is caught up again, one slot on"""
    g = np.asarray(g, np.int32)
    if not g.size:
        return
    sl, bn, bc, med, st = e.propose(g)
    assert (st == S_OK).all()
    decided = 0
    for acc in range(ME, ME + k // 2 + 1):
        decided += e.accept_reply(g, bn, bc, sl, np.full(g.size, acc, np.int32), np.zeros(g.size, np.int32)).gidx.shape[0]
    assert decided == g.size
    status, _ = e.commit(g, bn, bc, sl, med, np.full(g.size, C_HASVALUE, np.uint8))
    assert (status == S_OK).all()


def bare_accepts(e, g, step):
    """an ACCEPT for the group's current slot at a ballot number no earlier step used: accepted, not committed"""
    g = np.asarray(g, np.int32)
    if not g.size:
        return
    rows, _ = e.snapshot(g)
    out, _ = e.accept(g, np.full(g.size, step + 1, np.int32), np.full(g.size, ME, np.int32), rows["acc_slot"],
                      np.zeros(g.size, np.int32))
    assert (out[4] == S_OK).all()


def touch(e, groups, step, k=3):
    """Traffic for exactly `groups`: whole rounds for the even ones, bare ACCEPTs for the odd ones.  Every record
    changes its group's dump (tests/test_pause_sweep_abi.py shows it on the oracle)."""
    groups = np.asarray(groups, np.int32)
    whole_rounds(e, groups[groups % 2 == 0], k)
    bare_accepts(e, groups[groups % 2 == 1], step)


def touch_live(e, groups, step, k=3):
    """touch() for those of `groups` that are alive (a history that has paused some of them)"""
    groups = np.asarray(groups, np.int32)
    touch(e, groups[e.snapshot(groups)[1] == S_OK], step, k)


def traffic(e, n_groups, step):
    """a third of the table, another third each step -> the touched groups"""
    g = np.nonzero((np.arange(n_groups) * 7 + step) % 3 == 0)[0].astype(np.int32)
    touch(e, g, step)
    return g


def dumps(e, n_groups):
    return [tuple(e.dump(g).tolist()) for g in range(n_groups)]


class History:
    """One sequence of operations on a HIP engine (may be None) and the oracle, replayable into a scratch oracle."""

    def __init__(self, hip_lib, oracle_lib, n_groups, **kw):
        self.oracle_lib, self.n, self.kw = oracle_lib, n_groups, kw
        self.eh = engine(hip_lib, n_groups, create=False, **kw) if hip_lib is not None else None
        self.eo = engine(oracle_lib, n_groups, create=False, **kw)
        self.ops = []
        # what the sweep's idle words must hold, kept by the model: the dump a stored signature stands for, the age
        self.ref = [None] * n_groups
        self.age = np.zeros(n_groups, np.uint8)

    def do(self, op):
        """op(engine) on both engines, and remembered"""
        for e in (self.eh, self.eo):
            if e is not None:
                op(e)
        self.ops.append(op)

    def scratch(self):
        e = engine(self.oracle_lib, self.n, create=False, **self.kw)
        for op in self.ops:
            op(e)
        return e

    def close(self):
        for e in (self.eh, self.eo):
            if e is not None:
                e.close()

    # ---- the expected answer --------------------------------------------------------------------------------------
    def expect(self, gidx, n, min_age, flags, cap):
        """-> (model result, groups of the entries, rows of the written hits)"""
        groups = np.arange(n, dtype=np.int64) if gidx is None else np.asarray(gidx, np.int64)
        inr = (groups >= 0) & (groups < self.n)
        sc = self.scratch()
        _, st = sc.retire_groups(groups[inr].astype(np.int32))
        sc.close()
        status = np.full(groups.size, S_NOGROUP, np.uint8)
        status[inr] = st
        live, busy = status != S_NOGROUP, status == S_BUSY
        assert set(np.unique(status).tolist()) <= {S_OK, S_NOGROUP, S_BUSY}
        changed = np.ones(groups.size, bool)
        age = np.zeros(groups.size, np.int64)
        self._now = {}
        for i in np.nonzero(inr)[0]:
            g = int(groups[i])
            self._now[g] = tuple(self.eo.dump(g).tolist())
            changed[i] = self.ref[g] is None or self.ref[g] != self._now[g]
            age[i] = self.age[g]
        r = M.sweep(live, busy, changed, age, min_age, flags, cap)
        rows, _ = self.eo.snapshot(groups[r["hits"]].astype(np.int32))
        return r, groups, rows

    def settle(self, r, groups):
        """after a call that was not a peek: the idle words as the model leaves them, and the oracle retires exactly
        the paused groups"""
        inr = (groups >= 0) & (groups < self.n)
        for i in np.nonzero(inr)[0]:
            self.age[int(groups[i])] = r["new_age"][i]
        for i in r["stored"]:
            self.ref[int(groups[i])] = self._now[int(groups[i])]
        for i in r["cleared"]:
            if inr[i]:
                self.ref[int(groups[i])] = None
        paused = groups[r["paused"]].astype(np.int32)
        if paused.size:
            _, st = self.eo.retire_groups(paused)
            assert (st == S_OK).all()
            self.ops.append(lambda e, p=paused: e.retire_groups(p))
