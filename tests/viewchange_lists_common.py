"""Histories for the view change in list form (tests/test_viewchange_lists_gpu.py on the HIP engine,
tests/test_viewchange_lists_model.py on the oracle alone): two engines get one history through the dense host calls, then
one batch whose records are placed BY CONSTRUCTION - which record completes a majority, which is preempted, which is
refused - so that a test chooses where in the batch (and in which GPX_VCL_TILE of it) the hits and their entries fall.

Coordinator side.  Three members (7, 101, 5000), the candidate 101 with ballot (2, 101), every group's acceptor at S0.
A record is a KIND; each uses a fresh group:

  '.'   a first reply (member 7, no pvalues): RECORDED, no hit
  'i'   a reply of a non-member: IGNORED, no hit
  '0'   completes the majority with nothing carried and nothing proposed: ELECTED, 0 entries
  '1'   ... with slot S0 carried: ELECTED, 1 entry (carry)
  'W'   ... with S0 and S0 + W - 1 carried: ELECTED, W entries (carry, no-ops, carry)
  'P'   ... with two pre-active proposals and nothing carried: ELECTED, 2 entries (pre-active)
  'S'   ... with a stop carried at S0 and a request at S0 + 2: ELECTED, 4 entries (carry, no-op, carry, new stop)
  'X'   a higher ballot reaches a candidate with two pre-active proposals: PREEMPTED, 2 entries
  'C'   a reply whose own pvalues S0 and S0 + W share a ring index: IGNORED + GPX_S_WINDOW, a hit without entries
  'N'   completes the majority with a carried range of W + 1 slots: RECORDED + GPX_S_WINDOW, a hit without entries
  'G'   a group beyond the table: GPX_S_NOGROUP, a hit without entries

Acceptor side.  Group g has accepted g % (W + 1) pvalues at S0, S0 + 1, ... in ballot (0, 7), with S0 one below
Integer.MAX_VALUE (WRAP_S0): the slots of the longer lists lie on both sides of it, and the order they were numbered in
is not their signed order - or at PLAIN_S0, where the ring order of a list is not its slot order."""
import numpy as np

from gigapaxos_amd import Engine, S_OK
from tests.election_common import plain_rows, EB_PREPARING, S_PREACTIVE, PV_STOP

MEM, ME, BNUM, NON_MEMBER = [7, 101, 5000], 101, 2, 77
S0 = 5
G, MAX_BATCH = 3000, 4096
ELECT_KINDS = "01WPS"
HIT_KINDS = ELECT_KINDS + "XCNG"
WRAP_S0 = 2 ** 31 - 2                       # Integer.MAX_VALUE - 1
PLAIN_S0 = 6                                # accepted slots 6 .. 13: ring indices wrap inside the list at W = 4 and 8


def i32(x):
    return int((int(x) + 2 ** 31) % 2 ** 32 - 2 ** 31)


def coordinator_engine(lib, W, groups=G, max_batch=MAX_BATCH):
    e = Engine(lib, ME, groups, kmax=3, window=W, max_batch=max_batch)
    marr = np.tile(np.array(MEM, np.int32), (groups, 1))
    assert (e.create_groups(np.arange(groups), marr, 3, plain_rows(groups, S0, 0, MEM[0], gc=S0 - 2)) == S_OK).all()
    assert (e.election_begin(np.arange(groups, dtype=np.int32), np.full(groups, BNUM, np.int32)) == EB_PREPARING).all()
    return e


def first_reply_of(kind, W, x):
    """(first_slot, pvalues) of member 7's reply that precedes a record of this kind; None: there is none"""
    h = 70_000 + 10 * x
    return {"0": (S0, []), "1": (S0, [(S0, 0, 7, h, 0)]), "W": (S0, [(S0, 0, 7, h, 0), (S0 + W - 1, 1, 5000, h + 1, 0)]),
            "P": (S0, []), "S": (S0, [(S0, 0, 7, h, PV_STOP), (S0 + 2, 1, 7, h + 2, 0)]),
            "N": (S0 - 1, [(S0 + W - 1, 0, 7, h, 0)])}.get(kind)


def coordinator_batch(engines, W, kinds, first_group=0):
    """Prepares both engines for a batch of these kinds (pre-active proposals and first replies through the dense host
    calls) -> the batch: (gidx, acceptor, r_bnum, r_bcoord, first_slot, per-record pvalues)."""
    n = len(kinds)
    g = np.arange(first_group, first_group + n, dtype=np.int32)
    assert first_group + n <= int(engines[0].cfg.max_groups)
    pre = np.array([x for x, k in enumerate(kinds) if k in "PX"], np.int64)
    firsts = [(x, first_reply_of(k, W, x)) for x, k in enumerate(kinds) if first_reply_of(k, W, x) is not None]
    for e in engines:
        for i in range(2):
            if pre.shape[0]:
                sl, _, _, _, ps = e.propose(g[pre], np.zeros(pre.shape[0], np.uint8), handle=9001 + i + 10 * pre)
                assert (ps == S_PREACTIVE).all() and (sl == S0 + i).all()
        if firsts:
            idx = np.array([x for x, _ in firsts], np.int64)
            (vk, _, st), _ = e.prepare_reply(g[idx], np.full(idx.shape[0], 7, np.int32), np.full(idx.shape[0], BNUM, np.int32),
                                             np.full(idx.shape[0], ME, np.int32), [f[0] for _, f in firsts],
                                             [f[1] for _, f in firsts])
            assert (vk == 1).all() and (st == S_OK).all()     # RECORDED
    gidx, acc, rb, rc, fs, pvs = g.copy(), [], [], [], [], []
    for x, k in enumerate(kinds):
        a, b, f, pv = 5000, (BNUM, ME), S0, []
        if k == ".":
            a = 7
        elif k == "i":
            a = NON_MEMBER
        elif k == "X":
            a, b = 7, (BNUM + 1, 7)
        elif k == "C":
            a, pv = 7, [(S0, 0, 7, 60_000 + x, 0), (S0 + W, 0, 7, 61_000 + x, 0)]
        elif k == "N":
            f = S0 - 1
        elif k == "G":
            gidx[x] = int(engines[0].cfg.max_groups) + 5 + x
        acc.append(a), rb.append(b[0]), rc.append(b[1]), fs.append(f), pvs.append(pv)
    return gidx, np.array(acc, np.int32), np.array(rb, np.int32), np.array(rc, np.int32), np.array(fs, np.int32), pvs


def expected_entries(kind, W):
    return {"0": 0, "1": 1, "W": W, "P": 2, "S": 4, "X": 2, "C": 0, "N": 0, "G": 0}[kind]


def pattern(n, placed="", seed=0):
    """n kinds: a seeded mix with hits of every kind - or `placed` = {index: kind} over a background of non-hits."""
    if isinstance(placed, dict):
        out = ["." if x % 5 else "i" for x in range(n)]
        for x, k in placed.items():
            if -n <= x < n:
                out[x] = k
        return "".join(out)
    rng = np.random.default_rng(seed)
    return "".join(rng.choice(list("..i" + HIT_KINDS), n).tolist())


# ---- acceptor side --------------------------------------------------------------------------------------------------------
def acceptor_engine(lib, W, groups=G, max_batch=MAX_BATCH, s0=WRAP_S0):
    e = Engine(lib, ME, groups, kmax=3, window=W, max_batch=max_batch)
    marr = np.tile(np.array(MEM, np.int32), (groups, 1))
    s0 = i32(s0)
    assert (e.create_groups(np.arange(groups), marr, 3, plain_rows(groups, s0, 0, MEM[0], gc=i32(s0 - 2))) == S_OK).all()
    g = np.arange(groups, dtype=np.int32)
    for j in range(min(W, 8)):          # at most eight accepted pvalues per group, also at W = 64
        sel = g[g % (min(W, 8) + 1) > j]
        m = sel.shape[0]
        # a ring position that is not the arrival order either: slot S0 + (3 j mod 8)
        off = (3 * j) % min(W, 8)
        r = e.accept(sel, np.zeros(m, np.int32), np.full(m, MEM[0], np.int32), np.full(m, i32(s0 + off), np.int32),
                     np.full(m, i32(s0 - 1), np.int32))
        assert (r[0][4] == S_OK).all()
    return e


def acceptor_batch(n, groups=G, s0=WRAP_S0, seed=0, first_group=0):
    """n PREPAREs: mostly one per group at a greater ballot; every 9th group twice in the call, the second time at a
    smaller ballot (NACK after adopt); every 11th record at a ballot below the acceptor's (NACK); every 13th prunes the
    first accepted slot (first_slot S0 + 1); every 37th names no group."""
    g = (first_group + np.arange(n, dtype=np.int64)) % groups
    bn, bc, fs = np.full(n, 3, np.int32), np.full(n, ME, np.int32), np.full(n, i32(s0), np.int32)
    x = np.arange(n)
    bn[x % 11 == 10], bc[x % 11 == 10] = 0, 5            # (0, 5) < (0, 7)
    fs[x % 13 == 12] = i32(s0 + 1)
    dup = x[(x % 9 == 8) & (x >= 4)]
    g[dup], bn[dup] = g[dup - 4], 2                      # the same group four records on, at a smaller ballot
    g[x % 37 == 36] = groups + 7
    return g.astype(np.int32), bn, bc, fs
