"""The per-bucket accept-reply kernels behind the tiled front end (k_bucket_ar16_tiles_k4 / _k5, gigapaxos_amd/csrc/
gpx_ar16.hip.h) on the smallest tables that still take that front end with several buckets: 2,048 groups in
four buckets of 512 lanes, and 2,000 groups, whose last bucket is partial.  A regular round - every group with one to four
votes on its one outstanding slot at the batch's ballot, one decision per group - is staged by the K <= 4 kernel as two
words per vote and replayed in registers; anything else sends the whole workgroup back to the four-word layout.  Each case
below is one of the ways a bucket is, or stops being, regular; the results must be the oracle's either way: proposals,
decisions, per-vote status, HotRestoreInfo rows and counters.  Follows PISM.handleBatchedAcceptReply
(PaxosInstanceStateMachine.java:1370-1419) -> PCS.handleAcceptReplyMyBallot / HigherBallot
(PaxosCoordinatorState.java:597-683)."""
import numpy as np
import pytest

from gigapaxos_amd import hri_create, streams, S_OK, C_HASVALUE, C_STOP
from tests.parity_common import make_pair, wrap32
from tests.test_fullsize_gpu import _same

pytestmark = pytest.mark.gpu
INT32_MAX = (1 << 31) - 1


class Pair:
    """The HIP engine and the oracle over the same table, forced onto the tiled front end (no small-call kernel) with
    buckets of 512 groups.  base: per-group first slot (default 1 everywhere); coord: per-group coordinator.
    node_slots: how far behind `base - 1` every member's nodeSlotNumbers entry starts (one offset per member column;
    default 0 everywhere); window: the engine's window; tile: (votes, threads) per scatter workgroup, forced through
    GPX_TILE_T / GPX_TILE_NT (default: chosen per call); shift: GPX_BUCKET_SHIFT (1 << shift lanes per bucket)."""

    def __init__(self, monkeypatch, hip_lib, oracle_lib, G=2048, k=3, members=None, kmax=None, ks=None, coord=None, base=None,
                 holes=(), me=100, node_slots=None, window=8, tile=None, shift=9):
        monkeypatch.setenv("GPX_SAR_MAX_N", "0")
        monkeypatch.setenv("GPX_BUCKET_SHIFT", str(shift))
        if tile is not None:
            monkeypatch.setenv("GPX_TILE_T", str(tile[0]))
            monkeypatch.setenv("GPX_TILE_NT", str(tile[1]))
        self.G, self.k, self.me = G, k, me
        self.W, self.tile, self.shift = window, tile, shift
        self.kmax = kmax = k if kmax is None else kmax
        self.members = list(range(100, 100 + k)) if members is None else list(members)
        self.eh, self.eo = make_pair(hip_lib, oracle_lib, me, G, kmax, window, max_batch=4 * G * kmax + 4096)
        self.g = np.array([x for x in range(G) if x not in set(holes)], np.int32)
        n = self.g.shape[0]
        self.ks = np.full(n, k, np.uint8) if ks is None else np.asarray(ks, np.uint8)[self.g]
        mem = np.zeros((n, kmax), np.int32)
        for j in range(kmax):
            mem[:, j] = np.where(j < self.ks, self.members[j] if j < len(self.members) else 0, 0)
        self.base = np.ones(G, np.int64) if base is None else np.asarray(base, np.int64)
        coord = np.full(G, me, np.int32) if coord is None else np.asarray(coord, np.int32)
        rows = hri_create(n, k, me)
        rows["acc_bcoord"] = rows["coord_bcoord"] = coord[self.g]  # (as hri_create(1, k, coord) per group)
        b = self.base[self.g]
        rows["acc_slot"] = wrap32(rows["acc_slot"].astype(np.int64) - 1 + b)
        rows["acc_gc_slot"] = wrap32(rows["acc_gc_slot"].astype(np.int64) - 1 + b)
        rows["next_proposal_slot"] = wrap32(rows["next_proposal_slot"].astype(np.int64) - 1 + b)
        rows["node_slots"][:, :kmax] = wrap32(np.repeat((b - 1)[:, None], kmax, 1)) * (np.arange(kmax)[None, :] < self.ks[:, None])
        if node_slots is not None:
            behind = np.asarray(node_slots, np.int64)[None, :kmax]
            rows["node_slots"][:, :kmax] = wrap32((b - 1)[:, None] - behind) * (np.arange(kmax)[None, :] < self.ks[:, None])
        for e in (self.eh, self.eo):
            assert (e.create_groups(self.g, mem, self.ks, rows) == S_OK).all()
        if "profile_enable" in self.eh.lib.fn:  # (an oracle in the HIP engine's place has no kernels to name)
            self.eh.profile(2)
        self.round = 0

    def propose(self, g=None):
        g = self.g if g is None else np.asarray(g, np.int32)
        for x, y in zip(self.eh.propose(g), self.eo.propose(g)):
            assert (x == y).all()

    def votes(self, shuffled=True, groups=None):
        """This round's votes of every (or the given) group: slot = the group's base + round."""
        g = self.g if groups is None else np.asarray(groups, np.int32)
        cols = [c.copy() for c in streams.vote_round(self.G, self.members[:self.k], self.round, self.me, config_id=3,
                                                     shuffled=shuffled, groups=g)]
        if self.ks.min() < self.k:  # smaller groups: only their own members answer
            kk = np.zeros(self.G, np.int32)
            kk[self.g] = self.ks
            idx = np.searchsorted(np.array(self.members[:self.k]), cols[4])
            keep = idx < kk[cols[0]]
            cols = [np.ascontiguousarray(c[keep]) for c in cols]
        off = (self.base - 1)[cols[0]]
        cols[3] = wrap32(cols[3].astype(np.int64) + off)
        cols[5] = wrap32(cols[5].astype(np.int64) + off)
        return cols

    def reply(self, cols, what):
        dh, do = self.eh.accept_reply(*cols), self.eo.accept_reply(*cols)
        _same(dh, do, f"round {self.round} ({what})")
        self.round += 1
        return do

    def finish(self, kernel="k_bucket_ar16_tiles_k4"):
        allg = np.arange(self.G, dtype=np.int32)
        sh, so = self.eh.snapshot(allg), self.eo.snapshot(allg)
        assert sh[0].tobytes() == so[0].tobytes() and (sh[1] == so[1]).all()
        assert self.eh.counters() == self.eo.counters()
        prof = self.eh.profile_read()
        assert kernel in prof and "k_scatter_tiles" in prof, prof
        self.eh.close()
        self.eo.close()


def _insert(cols, at, vote):
    return [np.ascontiguousarray(np.insert(c, at, v)) for c, v in zip(cols, vote)]


@pytest.mark.parametrize("G", [2048, 2000])
def test_regular_rounds_and_the_ring(monkeypatch, hip_lib, oracle_lib, G):
    """Ten consecutive shuffled rounds with a window of 8: the slot crosses the ring (slot & 7 wraps at round 7), every
    call's outputs are in place.  2,000 groups: the last bucket is partial (its lanes beyond the table decide nothing)."""
    p = Pair(monkeypatch, hip_lib, oracle_lib, G=G)
    for r in range(10):
        p.propose()
        do = p.reply(p.votes(), "regular")
        assert do.gidx.shape[0] == G
        assert p.eh.path_counters() == (r + 1, 0)
    p.finish()


def test_learning_the_ratio(monkeypatch, hip_lib, oracle_lib):
    """One acceptor's votes missing: every bucket's count differs from its span (compacted, the ratio is learnt), then in
    place with two votes per decision, compacted once when all three answer again, then in place."""
    p = Pair(monkeypatch, hip_lib, oracle_lib)
    placed = 0
    for what, wp in zip(["all", "lost", "lost", "all", "all"], [True, False, True, False, True]):
        p.propose()
        cols = p.votes()
        if what == "lost":
            keep = cols[4] != p.members[-1]
            cols = [np.ascontiguousarray(c[keep]) for c in cols]
        p.reply(cols, what)
        pc, cc = p.eh.path_counters()
        assert pc + cc == p.round and (pc == placed + 1) == wp, (what, pc, cc)
        placed = pc
    p.finish()


@pytest.mark.parametrize("copies", [2, 6])
def test_more_votes_than_rows(monkeypatch, hip_lib, oracle_lib, copies):
    """A vote of group 700 repeated: five votes (nine with six more copies) in a group of three, more than the four rows
    - its bucket falls back, the others stay regular."""
    p = Pair(monkeypatch, hip_lib, oracle_lib)
    for r in range(2):
        p.propose()
        cols = p.votes()
        i = int(np.nonzero(cols[0] == 700)[0][0])
        v = [c[i] for c in cols]
        for j in range(copies):
            cols = _insert(cols, (i * 7 + 911 * j) % cols[0].shape[0], v)
        p.reply(cols, f"{3 + copies} votes in group 700")
    p.finish()


@pytest.mark.parametrize("what", ["higher", "lower"])
def test_another_ballot_in_one_group(monkeypatch, hip_lib, oracle_lib, what):
    """A vote of a HIGHER ballot in front of group 1300's own votes preempts its coordinator (the whole workgroup takes the
    general path, the preemption is an output); a vote of a LOWER ballot is stepped over and the group decides."""
    p = Pair(monkeypatch, hip_lib, oracle_lib)
    for r in range(3):
        p.propose()
        cols = p.votes()
        if r == 1:
            i = int(np.nonzero(cols[0] == 1300)[0][0])
            v = [c[i] for c in cols]
            if what == "higher":
                v[1], v[2] = 1, 101
            else:
                v[2] = 99
            cols = _insert(cols, max(i - 5, 0), v)
        do = p.reply(cols, what)
        if r == 1:
            assert do.gidx.shape[0] == p.G, "a preemption or a decision for group 1300"
    p.finish()


@pytest.mark.parametrize("members", [[-1, 100, 70000], [100, 70000, INT32_MAX]])
def test_escaped_acceptor_ids(monkeypatch, hip_lib, oracle_lib, members):
    """Node ids that do not fit the record's 16 bits: those votes carry the escape bit and are fetched from the caller's
    columns by their true arrival index (tile * tile size + offset)."""
    p = Pair(monkeypatch, hip_lib, oracle_lib, members=members)
    for r in range(3):
        p.propose()
        do = p.reply(p.votes(), "escaped ids")
        assert do.gidx.shape[0] == p.G
    p.finish()


@pytest.mark.parametrize("far", ["half", "one"])
def test_groups_out_of_lock_step(monkeypatch, hip_lib, oracle_lib, far):
    """Slots more than 128 apart: every other group 1,000 slots ahead gives wide tiles (slot and checkpoint travel beside the
    records); a single group far ahead gives one escaped slot, fetched from the columns."""
    G = 2048
    base = np.ones(G, np.int64)
    if far == "half":
        base[1::2] = 1001
    else:
        base[777] = 5001
    p = Pair(monkeypatch, hip_lib, oracle_lib, base=base)
    for r in range(3):
        p.propose()
        do = p.reply(p.votes(), far)
        assert do.gidx.shape[0] == G
    p.finish()


def test_groups_that_do_not_coordinate(monkeypatch, hip_lib, oracle_lib):
    """Inside otherwise regular buckets: a group whose coordinator is another node (it ignores every vote), a stopped group
    and a row of the table that holds no group."""
    G = 2048
    coord = np.full(G, 100, np.int32)
    coord[300] = 101
    p = Pair(monkeypatch, hip_lib, oracle_lib, coord=coord, holes=(900,))
    one = np.array([1500], np.int32)
    z1 = np.zeros(1, np.int32)
    kind = np.array([C_HASVALUE | C_STOP], np.uint8)
    sh, so = (e.commit(one, z1, np.full(1, 100, np.int32), np.ones(1, np.int32), z1, kind) for e in (p.eh, p.eo))
    assert (sh[0] == so[0]).all()
    for r in range(3):
        p.propose()
        cols = p.votes(groups=np.arange(G, dtype=np.int32))  # votes for the hole and the stopped group as well
        do = p.reply(cols, "idle, stopped and missing groups")
        assert do.gidx.shape[0] < G
    p.finish()


def test_five_replicas(monkeypatch, hip_lib, oracle_lib):
    """2,048 groups x 5: k_bucket_ar16_tiles_k5 (eight rows per group, on the four-word layout: its two-word form does not
    fit the kernel's registers); one round with a duplicated vote."""
    p = Pair(monkeypatch, hip_lib, oracle_lib, k=5)
    for r in range(4):
        p.propose()
        cols = p.votes()
        if r == 2:
            cols = _insert(cols, 17, [c[4000] for c in cols])
        do = p.reply(cols, "k = 5")
        assert do.gidx.shape[0] == p.G
    p.finish(kernel="k_bucket_ar16_tiles_k5")


def test_groups_of_one_and_two_members(monkeypatch, hip_lib, oracle_lib):
    """An engine of kmax 4 with groups of one, two and three members: one vote decides a group of one."""
    G = 2048
    ks = 1 + (np.arange(G) % 3)
    p = Pair(monkeypatch, hip_lib, oracle_lib, k=3, kmax=4, ks=ks)
    for r in range(3):
        p.propose()
        do = p.reply(p.votes(), "k = 1, 2, 3")
        assert do.gidx.shape[0] == G
    p.finish()


def test_sorted_by_group(monkeypatch, hip_lib, oracle_lib):
    """The regular round with its votes sorted by group: one long run per bucket and tile."""
    p = Pair(monkeypatch, hip_lib, oracle_lib)
    for r in range(3):
        p.propose()
        do = p.reply(p.votes(shuffled=False), "sorted")
        assert do.gidx.shape[0] == p.G
    p.finish()
