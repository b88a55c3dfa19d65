"""Traffic for the delta image tests (include/gpx_delta.h).  One table of 700 groups: rows 0 .. 559 belong to the
mixed-op fuzz (tests/parity_common.py, the driver of the geometry cells), rows 560 .. 699 to scripted steps the fuzz does
not make - elections that begin, end and begin again (a second row appears, goes, comes back), one accept reply below
majority (p_ring's responded mask alone), groups that die and rows that are created again with another state.  Every
step is applied to two engines and their answers are compared; tests/test_group_delta_model.py runs it oracle against
oracle and asserts what keeps the GPU test from being vacuous."""
import numpy as np

from gigapaxos_amd import Engine, S_OK, RETIRE_KILL
from tests import image_common as IC
from tests.parity_common import create_mixed_groups, fuzz

ME = IC.ME
N, FUZZ_G, ROUNDS = 700, 560, 6                  # tiles of 256 + 256 + 188
SCRIPTED = np.arange(FUZZ_G, N, dtype=np.int32)
GMAP = np.arange(FUZZ_G, dtype=np.int32)
NODES = [100, 101, 102, 103, 104, 105, 106, 107]
# seeds, steps and batch: chosen so that every round changes between 5 % and 60 % of the live groups on both shapes
# (asserted in tests/test_group_delta_model.py), and fixed
SHAPES = {"k3-w8": dict(kmax=3, k=3, window=8, seed=311, steps=3, batch=60),
          "k8-w4": dict(kmax=8, k=5, window=4, seed=312, steps=3, batch=60)}


def engine(lib, shape):
    return Engine(lib, ME, N, kmax=shape["kmax"], window=shape["window"], max_batch=1 << 12, flags=1)


def populate(ea, eb, shape, rng):
    create_mixed_groups(ea, eb, FUZZ_G, shape["kmax"], NODES, rng)
    for e in (ea, eb):
        IC.create(e, SCRIPTED, shape["kmax"], shape["k"])


def _plain(x):
    if isinstance(x, np.ndarray):
        return x.tolist()
    if hasattr(x, "as_tuple_array"):
        return x.as_tuple_array().tolist()
    if isinstance(x, (tuple, list)):
        return [_plain(y) for y in x]
    return x


def both(ea, eb, fn):
    """fn(engine) on both engines: the answers must be the same; returns engine a's"""
    ra, rb = fn(ea), fn(eb)
    assert _plain(ra) == _plain(rb)
    return ra


def mirror_round(ea, eb, shape, rng, r, ctx):
    """round r of the history, on both engines alike"""
    kmax, k = shape["kmax"], shape["k"]
    maj = k // 2 + 1
    fuzz(ea, eb, FUZZ_G, NODES, rng, steps=shape["steps"], batch=shape["batch"], gmap=GMAP)
    s = SCRIPTED
    none = np.zeros(0, np.int32)
    # one vote, below majority, for the proposals of the round before; new proposals for the next round
    if "votes" in ctx:
        g, sl, bn, bc = ctx.pop("votes")
        both(ea, eb, lambda e: e.accept_reply(g, bn, bc, sl, np.full(g.size, ME, np.int32), np.zeros(g.size, np.int32)))
    g = s[s % 7 == r % 7]
    out = both(ea, eb, lambda e: e.propose(g))
    ctx["votes"] = (g, out[0].copy(), out[1].copy(), out[2].copy())
    # elections: the class of the round before is elected, this round's class begins, the class of two rounds ago - by
    # now active - runs again at a higher ballot
    finish = s[s % 6 == (r - 1) % 6] if r >= 1 else none
    for a in range(ME, ME + maj + 1):
        if finish.size:
            both(ea, eb, lambda e: e.prepare_reply(finish, np.full(finish.size, a, np.int32), np.full(finish.size, r, np.int32),
                                                   np.full(finish.size, ME, np.int32), e.snapshot(finish)[0]["acc_slot"], None))
    begin = s[s % 6 == r % 6]
    both(ea, eb, lambda e: e.election_begin(begin, np.full(begin.size, r + 1, np.int32)))
    again = s[s % 6 == (r - 2) % 6] if r >= 2 else none
    if again.size:
        both(ea, eb, lambda e: e.election_begin(again, np.full(again.size, 10 + r, np.int32)))
    # groups die; the rows that died the round before are created again, in another state
    born = ctx.pop("dead", none)
    if born.size:
        for e in (ea, eb):
            IC.create(e, born, kmax, k, base_slot=20 + r)
    dead = np.concatenate([GMAP[GMAP % 40 == r], s[(s % 6 == (r + 4) % 6) & (s % 5 == 0)]]).astype(np.int32)
    both(ea, eb, lambda e: e.retire_groups(dead, RETIRE_KILL)[1])
    ctx["dead"] = GMAP[GMAP % 40 == r]
