"""Histories for the group image tests (include/gpx_image.h).  `first_half` takes the groups of a table into every state
a row has a section for - idle, whole rounds, a bare ACCEPT, proposals with a minority of votes, a commit ahead of an
undecided slot, stopped, running for coordinator with and without carried-over and pre-active proposals - and kills a
few; `second_half` is how the protocol goes on from there: the votes that decide, the commits that release the waiting
ones, the PREPARE replies that elect, new proposals.  Both work on a HIP engine and on the CPU oracle alike; the second
takes the place (engine, row) every group now lives at and answers in logical group numbers."""
import numpy as np

from gigapaxos_amd import Engine, hri_create, S_OK, C_HASVALUE, C_STOP, RETIRE_KILL
from tests import sweep_common as SC

ME = SC.ME
IDLE, ROUNDS, BARE, MINORITY, AHEAD, STOPPED, ELECT_FULL, ELECT_BARE = range(8)


def engine(lib, n_groups, kmax=3, window=8, max_batch=None):
    return Engine(lib, ME, n_groups, kmax=kmax, window=window, max_batch=max_batch or max(n_groups, 1 << 12), flags=1)


def create(e, groups, kmax, k, base_slot=1):
    g = np.asarray(groups, np.int32)
    rows = hri_create(g.size, k, ME)
    rows["acc_slot"] = base_slot
    rows["next_proposal_slot"] = base_slot
    rows["acc_gc_slot"] = base_slot - 1
    rows["version"] = g % 5
    rows["node_slots"][:, :k] = base_slot - 1 - (g[:, None] + np.arange(k)[None, :]) % 3
    assert (e.create_groups(g, SC.members_of(g.size, kmax, k), k, rows) == S_OK).all()


def categories(n, edges=()):
    """the state every group is taken to; the groups at `edges` run for coordinator (two rows each)"""
    cat = np.arange(n) % 8
    cat[np.asarray(edges, np.int64)] = ELECT_FULL
    return cat


def dead_groups(n, edges=()):
    return np.setdiff1d(np.arange(5, n, 11), np.asarray(edges, np.int64)).astype(np.int32)


def _sel(cat, c):
    return np.nonzero(cat == c)[0].astype(np.int32)


def _votes(e, g, bn, bc, sl, acceptors):
    out = []
    for a in acceptors:
        out.append(e.accept_reply(g, bn, bc, sl, np.full(g.size, a, np.int32), np.zeros(g.size, np.int32)))
    return out


def first_half(e, n, cat, k, dead=()):
    """every group into its state; returns what the second half needs to know (the same on every engine)"""
    ctx = {}
    maj = k // 2 + 1
    g = _sel(cat, ROUNDS)
    if g.size:
        # the first slot is accepted here before it is decided: executing it removes the accepted entry and leaves its
        # words behind, stale, under a cleared present bit
        out, _ = e.accept(g, np.zeros(g.size, np.int32), np.full(g.size, ME, np.int32), e.snapshot(g)[0]["acc_slot"],
                          np.zeros(g.size, np.int32))
        assert (out[4] == S_OK).all()
    for r in range(3):
        SC.whole_rounds(e, g[g % 3 >= r], k)
    SC.bare_accepts(e, _sel(cat, BARE), 0)
    g = _sel(cat, MINORITY)
    if g.size:
        s0, bn, bc, _, st = e.propose(g)
        s1 = e.propose(g)[0]
        assert (st == S_OK).all()
        for d in _votes(e, g, bn, bc, s0, range(ME, ME + maj - 1)):
            assert d.gidx.size == 0
        ctx["minority"] = (s0.copy(), s1.copy(), bn.copy(), bc.copy())
    g = _sel(cat, AHEAD)
    if g.size:
        slot = e.snapshot(g)[0]["acc_slot"]
        st, runs = e.commit(g, np.zeros(g.size, np.int32), np.full(g.size, ME, np.int32), slot + 1, slot - 1,
                            np.full(g.size, C_HASVALUE, np.uint8))
        assert (st == S_OK).all() and runs.gidx.size == 0
        ctx["ahead"] = slot.copy()
        early = (g // 8) % 2 == 1                               # every other one is released at once: a stale committed entry
        if early.any():
            st, runs = e.commit(g[early], np.zeros(early.sum(), np.int32), np.full(early.sum(), ME, np.int32), slot[early],
                                slot[early] - 1, np.full(early.sum(), C_HASVALUE, np.uint8))
            assert (st == S_OK).all() and (runs.count == 2).all()
    g = _sel(cat, STOPPED)
    if g.size:
        sl, bn, bc, med, st = e.propose(g, np.ones(g.size, np.uint8))
        assert (st == S_OK).all()
        _votes(e, g, bn, bc, sl, range(ME, ME + maj))
        st, _ = e.commit(g, bn, bc, sl, med, np.full(g.size, C_HASVALUE | C_STOP, np.uint8))
        assert (st == S_OK).all()
    for c in (ELECT_FULL, ELECT_BARE):
        g = _sel(cat, c)
        if g.size:
            assert (e.election_begin(g, np.ones(g.size, np.int32)) == 0).all()       # GPX_EB_PREPARING
    g = _sel(cat, ELECT_FULL)
    if g.size:
        for r in range(2):                                                            # pre-active proposals, with handles
            st = e.propose(g, handle=(g.astype(np.int64) << 33) + 5 + r)[4]
            assert (st == 8).all()                                                    # GPX_S_PREACTIVE
        if k >= 2:                                                                    # one reply: no majority yet
            slot = e.snapshot(g)[0]["acc_slot"]
            e.prepare_reply(g, np.full(g.size, ME + 1, np.int32), np.ones(g.size, np.int32), np.full(g.size, ME, np.int32),
                            slot, [[(int(s), 0, ME, (int(x) << 34) + 9, int(x) & 1)] for s, x in zip(slot, g)])
    dead = np.asarray(dead, np.int32)
    if dead.size:
        e.retire_groups(dead, RETIRE_KILL)
    return ctx


def second_half(where, engines, n, cat, k, ctx, dead=(), split=None):
    """The protocol goes on.  where[g] = (engine index, row) of logical group g; engines: the engines in that order.
    Every call is made once per part of `split` (default: the engine a group lives on; all groups of a part live on one
    engine) with the groups of that part, the group index rewritten; returns every call's outputs as plain lists, group
    columns back in logical numbers: two runs over different placements of the same groups, split alike, must return
    the same."""
    maj = k // 2 + 1
    alive = np.ones(n, bool)
    alive[np.asarray(dead, np.int64)] = False
    split = np.array([where[g][0] for g in range(n)]) if split is None else np.asarray(split)
    log = []

    def each(groups, fn):
        """fn(engine, rows, positions into `groups`) per part, parts ascending"""
        groups = np.asarray(groups, np.int32)
        for part in np.unique(split):
            pos = np.nonzero(alive[groups] & (split[groups] == part))[0]
            if pos.size:
                e = engines[where[int(groups[pos[0]])][0]]
                rows = np.array([where[int(g)][1] for g in groups[pos]], np.int32)
                back = {int(r): int(g) for r, g in zip(rows, groups[pos])}
                log.append(fn(e, rows, pos, back))

    def votes(groups, bn, bc, sl, acceptor):
        def fn(e, rows, pos, back):
            d = e.accept_reply(rows, bn[pos], bc[pos], sl[pos], np.full(pos.size, acceptor, np.int32), np.zeros(pos.size, np.int32))
            return ("votes", [back[int(x)] for x in d.gidx], d.slot.tolist(), d.bnum.tolist(), d.bcoord.tolist(),
                    d.median_cp.tolist(), d.kind.tolist(), d.status.tolist())
        each(groups, fn)

    if "minority" in ctx:                                        # the votes that decide: slot s0, then s1
        g = _sel(cat, MINORITY)
        s0, s1, bn, bc = ctx["minority"]
        votes(g, bn, bc, s0, ME + maj - 1)
        for a in range(ME, ME + maj):
            votes(g, bn, bc, s1, a)
    if "ahead" in ctx:                                           # the commit that releases the waiting one
        g = _sel(cat, AHEAD)
        slot = ctx["ahead"]

        def fn(e, rows, pos, back):
            st, runs = e.commit(rows, np.zeros(pos.size, np.int32), np.full(pos.size, ME, np.int32), slot[pos], slot[pos] - 1,
                                np.full(pos.size, C_HASVALUE, np.uint8))
            return ("commit", st.tolist(), [back[int(x)] for x in runs.gidx], runs.first.tolist(), runs.count.tolist())
        each(g, fn)
    for c in (ELECT_FULL, ELECT_BARE):                           # the PREPARE replies that elect
        g = _sel(cat, c)
        for a in range(ME, ME + maj + 1):
            def fn(e, rows, pos, back, a=a):
                slot = e.snapshot(rows)[0]["acc_slot"]
                (vk, em, st), lists = e.prepare_reply(rows, np.full(pos.size, a, np.int32), np.ones(pos.size, np.int32),
                                                      np.full(pos.size, ME, np.int32), slot, None)
                return ("prepare_reply", vk.tolist(), em.tolist(), st.tolist(), lists)
            each(g, fn)
    everybody = np.arange(n, dtype=np.int32)                     # new proposals, everywhere

    def fn(e, rows, pos, back):
        return ("propose",) + tuple(x.tolist() for x in e.propose(rows))
    each(everybody, fn)
    return log


def all_dumps(where, engines, n, dead=()):
    """the dump of every logical group where it lives now (a dead group has no place: its old row may be taken)"""
    dead = set(np.asarray(dead).tolist())
    return [(0,) if g in dead else tuple(engines[where[g][0]].dump(where[g][1]).tolist()) for g in range(n)]
