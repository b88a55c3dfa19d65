"""Bucket-geometry edges: the engine against the oracle at the table sizes where gpx_engine_create's geometry changes.

  130,560 / 130,561   buckets of 256 -> 512 groups (shift 8 -> 9)
  2^21                4,096 buckets of 512 groups: the tiled front end's counter block is full (tl_cnt_words)
  2^21 + 1            shift 10
  2^22                4,096 buckets of 1,024 groups
  2^22 + 1            shift 11: buckets of 2,048 groups on 1,024 threads - the ACCEPT / COMMIT partition path on
                      k_scatter_ac / k_bucket_accept / k_bucket_commit / k_emit_runs, two accept-reply passes
  2^23 + 1            shift 12 (BASELINE config #5's 10 M groups have the same geometry)

The default run takes 130,561, 2^21, 2^21 + 1 and 2^22 + 1; GPX_FULL_MATRIX=1 adds the others.  At each size, from
groups created in bulk: shuffled accept-reply calls of ~500 k votes (4,096-vote tiles), of 3.1 M votes (12,288-vote
tiles) and of ~500 k votes again on the same engine (what a large call left in the tile area must not matter), then the
mixed-op fuzz (ACCEPT, COMMIT, PREPARE, proposals and accept replies; shuffled, then grouped by group) and the
coordinator side of the view change (election_begin, prepare replies with carried pvalues, poke_scan) on a hot set of
a few thousand groups on the table's edges (tests/geometry_common.py: hot_set).  Every call's outputs and statuses,
then the snapshot rows of the hot set and of a seeded sample, then the counters; every call asserts the kernels that
geometry_common's restatement of the dispatch predicts."""
import os

import numpy as np
import pytest

from gigapaxos_amd import hri_create, S_OK
from tests.geometry_common import geometry, ar_route, ar_kernels, hot_set
from tests.parity_common import make_pair, fuzz
from tests.test_fullsize_gpu import _same

pytestmark = pytest.mark.gpu

SIZES = [130_561, pytest.param(1 << 21, marks=pytest.mark.gpu_fast), (1 << 21) + 1, (1 << 22) + 1]
if os.environ.get("GPX_FULL_MATRIX") == "1":
    SIZES += [130_560, 1 << 22, (1 << 23) + 1]
MEMBERS = [100, 101, 102]
N_BIG = 3_100_000


@pytest.fixture(autouse=True)
def _default_paths(monkeypatch):
    for v in ("GPX_AR_TILES", "GPX_TRY_RUNS", "GPX_SAR_MAX_N", "GPX_BUCKET_SHIFT", "GPX_TILE_T", "GPX_TILE_NT"):
        monkeypatch.delenv(v, raising=False)


def _profiled(e, fn):
    e.profile(2)
    out = fn()
    ran = e.profile_read()
    e.profile(0)
    return out, ran


def _votes(groups, slot, n_target, rng):
    """Shuffled votes of every member for `slot` of each group in `groups`, repeated (duplicates) up to ~n_target."""
    reps = max(1, -(-n_target // (3 * groups.shape[0])))
    gi = np.repeat(groups, 3 * reps).astype(np.int32)
    acc = np.tile(np.array(MEMBERS, np.int32), groups.shape[0] * reps)
    n = gi.shape[0]
    cols = [gi, np.zeros(n, np.int32), np.full(n, 100, np.int32), np.full(n, slot, np.int32), acc,
            np.full(n, slot - 1, np.int32)]
    order = rng.permutation(n)
    return [np.ascontiguousarray(c[order]) for c in cols]


def _ar_call(eh, eo, geo, cols, what):
    route = ar_route(geo, cols[0].shape[0])
    dh, ran = _profiled(eh, lambda: eh.accept_reply(*cols))
    do = eo.accept_reply(*cols)
    _same(dh, do, what)
    want = ar_kernels(route)
    assert want <= set(ran), (what, route, sorted(ran))
    assert ("k_scatter_tiles" in ran) == (route[0] == "tiles"), (what, route, sorted(ran))
    return route


def _election(eh, eo, sel, rng):
    """The coordinator side of the view change on `sel`: a higher ballot, prepare replies that carry pvalues."""
    bn = np.ones(sel.shape[0], np.int32)
    assert eh.election_begin(sel, bn).tolist() == eo.election_begin(sel, bn).tolist()
    gi = np.repeat(sel, 2).astype(np.int32)
    n = gi.shape[0]
    acc = np.tile(np.array(MEMBERS[1:], np.int32), sel.shape[0])
    first = eo.snapshot(gi)[0]["acc_slot"].astype(np.int32) + rng.integers(-1, 2, n).astype(np.int32)
    pvs = []
    for i in range(n):
        ss = int(first[i]) + np.sort(rng.choice(6, int(rng.integers(0, 4)), replace=False))
        pvs.append([(int(s), int(rng.integers(0, 2)), int(rng.choice(MEMBERS)), 10 ** 10 + int(s), 0) for s in ss])
    rb = np.ones(n, np.int32) - (rng.random(n) < 0.05).astype(np.int32)
    rc = np.full(n, 100, np.int32)
    (ah, lh), ran = _profiled(eh, lambda: eh.prepare_reply(gi, acc, rb, rc, first, pvs))
    ao, lo = eo.prepare_reply(gi, acc, rb, rc, first, pvs)
    for x, y, nm in zip(ah, ao, ("v_kind", "e_median", "status")):
        assert x.tolist() == y.tolist(), f"prepare reply {nm}"
    assert lh == lo, "prepare reply carried pvalues"
    assert "k_bucket_prepare_reply" in ran, sorted(ran)
    for x, y in zip(eh.poke_scan(sel), eo.poke_scan(sel)):
        assert x.tolist() == y.tolist(), "poke_scan"


@pytest.mark.parametrize("G", SIZES)
def test_geometry_edges_vs_oracle(hip_lib, oracle_lib, G):
    k = 3
    geo = geometry(G, k)
    rng = np.random.default_rng(G)
    eh, eo = make_pair(hip_lib, oracle_lib, 100, G, k, 8, max_batch=max(G, N_BIG) + N_BIG // 10)
    mem = np.tile(np.array(MEMBERS, np.int32), (G, 1))
    for e in (eh, eo):
        assert (e.create_groups(np.arange(G), mem, k, hri_create(G, k, 100)) == S_OK).all()
    g = np.arange(G, dtype=np.int32)
    for _ in range(3):  # slots 1, 2, 3 outstanding everywhere
        for x, y in zip(eh.propose(g), eo.propose(g)):
            assert (x == y).all()
    hot, place = hot_set(G, geo, rng)
    last = place["last bucket"]

    # accept replies: ~500 k votes (4,096-vote tiles where the tiled front end takes the call), 3.1 M votes, then ~500 k
    # votes again on the same engine; each call has votes for the groups of the last bucket
    def some(m):
        pick = rng.choice(G, size=min(G, m), replace=False).astype(np.int32)
        return np.unique(np.concatenate([pick, hot, last]))
    routes = [_ar_call(eh, eo, geo, _votes(some(166_000), 1, 500_000, rng), "~500 k votes"),
              _ar_call(eh, eo, geo, _votes(some(1_033_000), 2, N_BIG, rng), "3.1 M votes"),
              _ar_call(eh, eo, geo, _votes(some(166_000), 3, 500_000, rng), "~500 k votes after 3.1 M")]
    if geo["ar_passes"] == 1 and G >= 1 << 20:  # what the tiled front end is for: both tile sizes
        assert routes[0][:2] == ("tiles", 4096) and routes[1][:2] == ("tiles", 12288), routes

    # the mixed-op fuzz on the hot set, shuffled then grouped by group; batches past the one-workgroup vote path
    nodes = MEMBERS + [103]
    H = hot.shape[0]
    seen, ran = {}, set()
    for ordered in (False, True):
        s, r = _profiled(eh, lambda: fuzz(eh, eo, H, nodes, rng, steps=24, batch=4000, slot_base=3, span=24,
                                          ordered=ordered, gmap=hot, min_batch=1100))
        ran |= set(r)
        for op, st in s.items():
            seen.setdefault(op, set()).update(st)
    assert all(seen[op] for op in ("propose", "accept", "accept_reply", "commit", "prepare")), seen
    assert "k_ar_tiny" not in ran
    assert ar_kernels(ar_route(geo, 1100)) <= ran, sorted(ran)
    want = {"k_bucket_prepare", "k_bucket_propose"}
    want |= {"k_bucket_accept16", "k_bucket_commit16"} if geo["ac16"] else {"k_scatter_ac", "k_bucket_accept",
                                                                            "k_bucket_commit", "k_emit_runs"}
    assert want <= ran, (sorted(want - ran), sorted(ran))

    _election(eh, eo, hot[::3].copy(), rng)

    assert eh.snapshot(hot)[0].tobytes() == eo.snapshot(hot)[0].tobytes()
    sample = np.unique(rng.integers(0, G, 4096)).astype(np.int32)
    assert eh.snapshot(sample)[0].tobytes() == eo.snapshot(sample)[0].tobytes()
    assert eh.counters() == eo.counters()
    eh.close()
    eo.close()
