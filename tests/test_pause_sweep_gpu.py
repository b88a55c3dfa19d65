"""The deactivation sweep (include/gpx_sweep.h) on the GPU.  Every case applies one history to a HIP engine and to the CPU
oracle (tests/sweep_common.py); the expected answer of a call is tests/sweep_model.py over the ORACLE: live and busy from
orc_group_retire(PAUSE) on a scratch copy of the oracle, rows from orc_group_snapshot, changed from orc_group_dump against
its value when the signature was last stored.  After each real sweep the oracle retires exactly the paused groups, so
the two stay in lockstep.  Both forms write into sentinel-filled buffers with padding behind cap.

Ages are asserted for EVERY group of every table: a group that received no record since the last sweep must have its age
plus one, exactly; one that received records must be back at 0 (every record of these histories changes its group's dump:
tests/test_pause_sweep_abi.py shows that on the oracle alone).  They are read back with PEEK | HOLD at min_age 0."""
import os

import numpy as np
import pytest

from gigapaxos_amd import S_OK, S_NOGROUP, C_HASVALUE, HRI_DTYPE
from gigapaxos_amd import sweep
from tests import sweep_common as SC
from tests import sweep_model as M

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
PAD = 9                                   # entries behind cap that no call may touch
T = 1024                                  # groups per workgroup of the first launch
G3 = 3 * T + 1                            # three tiles and one entry
DTYPES = [dt for _, dt in sweep.SWEEP_COLS]
EDGES = np.array([0, 63, 64, 255, 256, 1023, 1024, 2047, 2048, 3071, 3072])


def filled(count, dtype):
    return np.frombuffer(bytes([SENTINEL]) * (count * np.dtype(dtype).itemsize), dtype).copy()


def untouched(a):
    return (np.asarray(a).view(np.uint8) == SENTINEL).all()


def call_host(eh, gidx, n, min_age, flags, cap, null_cols=False):
    out = None if null_cols else [filled(cap + PAD, dt) for dt in DTYPES]
    cols, counts = sweep.pause_sweep(eh, gidx, min_age, flags, cap=cap, n=n, out=out)
    if out is not None:
        for c, a in zip(cols, out):
            assert c.shape[0] == max(0, min(counts.n_hits, cap)) and c.ctypes.data == a.ctypes.data
    return out, counts


def call_dev(eh, gidx, n, min_age, flags, cap, null_cols=False):
    """the _dev form: device buffers everywhere, the counts read from device memory after one engine sync"""
    import torch

    bufs = [] if null_cols else [torch.full(((cap + PAD) * dt.itemsize,), SENTINEL, dtype=torch.uint8, device="cuda")
                                 for dt in DTYPES]
    cnt = torch.full((16 + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    g = None if gidx is None else torch.from_numpy(np.ascontiguousarray(gidx, np.int32)).cuda()
    torch.cuda.synchronize()
    sweep.pause_sweep_dev(eh, n, 0 if g is None else g.data_ptr(), min_age, flags, cap,
                          [b.data_ptr() for b in bufs] if bufs else [0, 0, 0], cnt.data_ptr())
    eh.sync()
    raw = cnt.cpu().numpy()
    assert untouched(raw[16:])
    counts = sweep.SweepCounts.from_buffer_copy(raw[:16].tobytes())
    out = None if null_cols else [b.cpu().numpy().view(dt) for b, dt in zip(bufs, DTYPES)]
    return out, counts


def check(H, min_age, flags, cap, form, gidx=None, n=None, null_cols=False, what=""):
    """One call against the model over the oracle: columns, counts, the sentinel from the last written entry on; a
    call that is not a peek then settles the history.  Returns the model's answer and the entries' groups."""
    n = (H.n if gidx is None else len(gidx)) if n is None else n
    r, groups, rows = H.expect(gidx, n, min_age, flags, cap)
    out, counts = (call_host if form == "host" else call_dev)(H.eh, gidx, n, min_age, flags, cap, null_cols)
    tag = f"{what} {form} min_age={min_age} flags={flags} cap={cap}"
    got = (counts.n_hits, counts.n_nogroup, counts.n_busy, counts.n_paused)
    print(f"{tag}: counts {got}, model {r['counts']}")
    assert got == r["counts"], tag
    k = r["hits"].size
    if out is not None:
        assert out[0][:k].tolist() == groups[r["hits"]].tolist(), tag
        assert out[1][:k].tolist() == r["ages"].tolist(), tag
        assert out[2][:k].tobytes() == rows.tobytes(), tag
        assert all(untouched(a[k:]) for a in out), f"{tag}: written at or beyond entry {k}"
    if not flags & M.PEEK:
        H.settle(r, groups)
    return r, groups


def peek_both(H, min_age, flags, cap, **kw):
    """both forms, twice the host one: a peek changes nothing, so all three see the same"""
    for form in ("host", "dev", "host"):
        r, groups = check(H, min_age, flags | M.PEEK, cap, form, **kw)
    return r, groups


def ages_agree(H, what=""):
    """every caught-up group's stored age, read back with PEEK | HOLD at min_age 0, against the model's"""
    return check(H, 0, M.PEEK | M.HOLD, H.n, "host", what=what + " ages")


def liveness_agrees(H):
    """paused groups answer GPX_S_NOGROUP, the others are alive: through gpx_group_snapshot, against the oracle"""
    g = np.arange(H.n, dtype=np.int32)
    (rh, sh), (ro, so) = H.eh.snapshot(g), H.eo.snapshot(g)
    assert sh.tolist() == so.tolist() and rh.tobytes() == ro.tobytes()
    return sh


def history(hip_lib, oracle_lib, n, **kw):
    H = SC.History(hip_lib, oracle_lib, n, **kw)
    kmax, k = kw.get("kmax", 3), kw.get("k", 3)
    H.do(lambda e: SC.create_all(e, n, kmax, k))
    return H


def hit_set(name, n=G3):
    if name == "edges":
        return EDGES
    if name == "hole":                      # tile 0 nothing but hits, tile 1 empty, tile 2 nothing but hits
        return np.concatenate([np.arange(0, T), np.arange(2 * T, 3 * T)])
    if name == "all":
        return np.arange(n)
    assert name == "none"
    return np.zeros(0, np.int64)


# 1 ---- where the hits sit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges", "hole", "all", "none"])
def test_hits_by_construction(hip_lib, oracle_lib, name):
    H = history(hip_lib, oracle_lib, G3)
    hits = hit_set(name)
    r, _ = check(H, 1, 0, G3, "host", what="first")
    assert r["counts"] == (0, 0, 0, 0)                                # nobody has an age yet
    others = np.setdiff1d(np.arange(G3), hits)
    H.do(lambda e: SC.touch(e, others, 0))
    r, _ = peek_both(H, 1, 0, G3, what=name)
    assert r["hits"].tolist() == hits.tolist() and r["counts"] == (hits.size, 0, 0, 0)
    r, _ = check(H, 1, 0, G3, "dev", what=name)
    assert r["paused"].tolist() == hits.tolist()
    st = liveness_agrees(H)
    assert (st[hits] == S_NOGROUP).all() and (st[others] == S_OK).all()
    r, _ = ages_agree(H, name)
    assert r["hits"].tolist() == others.tolist() and not r["ages"].any()
    H.close()


# 2 ---- short capacities; HOLD continues after a cut ------------------------------------------------------------------------
def test_capacities_and_hold(hip_lib, oracle_lib):
    H = history(hip_lib, oracle_lib, G3)
    idle = np.union1d(np.arange(0, G3, 7), EDGES)
    tile0 = int((idle < T).sum())
    check(H, 1, 0, G3, "dev", what="first")
    H.do(lambda e: SC.touch(e, np.setdiff1d(np.arange(G3), idle), 0))
    # the period's tick, counting only: the idle groups now have age 1, nothing is paused
    r, _ = check(H, 1, 0, 0, "host", null_cols=True, what="tick, counts only")
    assert r["counts"] == (idle.size, 0, 0, 0)
    check(H, 1, M.HOLD, 0, "dev", null_cols=True, what="counts only")
    left = idle.size
    for cap, form in ((1, "host"), (tile0 - 1, "dev"), (None, "host"), (5, "dev")):
        cap = left - 1 if cap is None else cap                         # n_hits - 1: one hit is left behind
        peek_both(H, 1, M.HOLD, cap, what="cut")
        r, groups = check(H, 1, M.HOLD, cap, form, what="cut")
        assert r["counts"] == (left, idle.size - left, 0, min(cap, left))
        assert r["paused"].tolist() == idle[idle.size - left:][:cap].tolist()      # the NEXT cap hits, in order
        left -= min(cap, left)
        st = liveness_agrees(H)
        assert (st[idle[:idle.size - left]] == S_NOGROUP).all() and (st[idle[idle.size - left:]] == S_OK).all()
        ages_agree(H, "cut")
    assert left == 0                                                   # the last call's cap was above n_hits
    # the next period: everybody left is idle; cap = n_hits exactly
    r, _ = peek_both(H, 1, 0, G3, what="second period")
    n_hits = r["counts"][0]
    assert n_hits == G3 - idle.size
    r, _ = check(H, 1, 0, n_hits, "dev", what="cap = n_hits")
    assert r["counts"] == (n_hits, idle.size, 0, n_hits)
    assert (liveness_agrees(H) == S_NOGROUP).all()
    H.close()


# 3 ---- ageing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_age", [0, 1, 2, 3])
def test_ageing_over_six_sweeps(hip_lib, oracle_lib, min_age):
    n = T + 1
    H = history(hip_lib, oracle_lib, n)
    paused = 0
    for step in range(6):
        if step:
            # a third of the table per step, in turn; the groups 1, 5, 9, ... never: they reach every min_age here
            H.do(lambda e, s=step: SC.touch_live(e, np.nonzero(((np.arange(n) * 7 + s) % 3 == 0) & (np.arange(n) % 4 != 1))[0], s))
        first, _ = peek_both(H, min_age, 0, 40, what=f"sweep {step}")
        if step == 3:                                                  # not a period: nobody ages
            r, _ = check(H, min_age, M.HOLD, 40, "host", what=f"hold {step}")
        else:
            r, _ = check(H, min_age, 0, 40, "dev" if step & 1 else "host", what=f"sweep {step}")
            assert r["hits"].tolist() == first["hits"].tolist() and r["ages"].tolist() == first["ages"].tolist()
        paused += r["counts"][3]
        ages_agree(H, f"sweep {step}")
        liveness_agrees(H)
    assert paused > 40
    H.close()


def test_age_saturates_at_255(hip_lib, oracle_lib):
    n = T + 1
    H = history(hip_lib, oracle_lib, n)
    busy = np.arange(5, n, 50, dtype=np.int32)
    H.do(lambda e: e.propose(busy))
    check(H, 1, 0, 0, "host", null_cols=True, what="first")
    # 253 periods without traffic, counting only: the model takes live, busy and the dumps from the first of them
    live = np.ones(n, bool)
    is_busy = np.zeros(n, bool)
    is_busy[busy] = True
    for _ in range(253):
        out, counts = call_dev(H.eh, None, n, 255, 0, 0, null_cols=True)
        r = M.sweep(live, is_busy, np.zeros(n, bool), H.age, 255, 0, 0)
        assert (counts.n_hits, counts.n_nogroup, counts.n_busy, counts.n_paused) == r["counts"] == (0, 0, busy.size, 0)
        H.age = r["new_age"]
    assert int(H.age.max()) == 253
    for want in (254, 255, 255):
        r, _ = check(H, 255, 0, 0, "host", null_cols=True, what="towards 255")
        assert int(H.age.max()) == want and r["counts"][0] == (n - busy.size if want == 255 else 0)
        ages_agree(H, "saturation")
    r, _ = check(H, 255, M.HOLD, n, "dev", what="at 255")
    assert r["paused"].size == n - busy.size and set(r["ages"].tolist()) == {255}
    H.close()


# 4 ---- busy groups of each kind -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("from_disk", [True, False])
def test_busy_groups_of_each_kind(hip_lib, oracle_lib, from_disk):
    n = T + 1
    H = history(hip_lib, oracle_lib, n, from_disk=from_disk)
    a, b, c, d = (np.arange(q, n, 40, dtype=np.int32) for q in (3, 64, 65, 255))
    check(H, 1, 0, n, "host", what="first")
    H.do(lambda e: e.propose(a))                                           # an outstanding proposal
    H.do(lambda e: e.commit(b, np.zeros(b.size, np.int32), np.full(b.size, SC.ME, np.int32), np.full(b.size, 3, np.int32),
                            np.zeros(b.size, np.int32), np.full(b.size, C_HASVALUE, np.uint8)))   # a commit ahead of slot 1
    H.do(lambda e: SC.bare_accepts(e, c, 0))                               # accepted, not committed
    H.do(lambda e: e.election_begin(d, np.ones(d.size, np.int32)))         # running for coordinator, nobody heard yet
    r, groups = peek_both(H, 1, 0, 30, what="busy kinds")
    assert r["counts"][2] == a.size + b.size + (0 if from_disk else c.size)
    touched = np.concatenate([a, b, c, d])
    assert r["counts"][0] == n - touched.size                              # with accepts from disk c is caught up, at age 0
    check(H, 1, 0, 30, "dev", what="busy kinds")
    ages_agree(H, "busy kinds")
    # a PREPARE reply that is no majority yet: the coordinator's wait mask and carried-over pvalues are activity
    H.do(lambda e: e.prepare_reply(d, np.full(d.size, SC.ME + 1, np.int32), np.ones(d.size, np.int32),
                                   np.full(d.size, SC.ME, np.int32), np.ones(d.size, np.int32),
                                   [[(1, 0, SC.ME, 7 + int(g), 0)] for g in d]))
    r, groups = check(H, 1, 0, 30, "host", what="after a prepare reply")
    assert not np.isin(d, groups[r["hits"]]).any()
    ages_agree(H, "after a prepare reply")
    check(H, 1, 0, n, "dev", what="everybody idle")
    liveness_agrees(H)
    H.close()


# 5 ---- windows, group sizes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmax,k,window", [(3, 3, 4), (3, 3, 64), (16, 16, 8), (3, 1, 8)])
def test_windows_and_group_sizes(hip_lib, oracle_lib, kmax, k, window):
    n = T + 1
    H = history(hip_lib, oracle_lib, n, kmax=kmax, k=k, window=window)
    check(H, 1, 0, n, "dev", what="first")
    for step in range(2):
        H.do(lambda e, s=step: SC.touch_live(e, np.nonzero((np.arange(n) + s) % 3 == 0)[0], s, k))
        peek_both(H, 1, 0, 100, what=f"K={k} W={window}")
        r, groups = check(H, 1, 0, 100, "host" if step else "dev", what=f"K={k} W={window}")
        assert r["paused"].size == 100
        ages_agree(H)
    liveness_agrees(H)
    H.close()


# 6 ---- bound names ---------------------------------------------------------------------------------------------------------
def test_paused_names_answer_nogroup(hip_lib, oracle_lib):
    from gigapaxos_amd import wire as W

    n = 300
    H = history(hip_lib, oracle_lib, n)
    names = [b"svc-%d" % g for g in range(n)]
    wh = W.WireEngine(H.eh)
    assert (wh.bind(names, np.arange(n)) == S_OK).all()
    check(H, 1, 0, n, "host", what="first")
    r, groups = check(H, 1, 0, 100, "dev", what="names")
    assert r["paused"].tolist() == list(range(100)) and r["counts"][0] == n
    frames = [W.batched_accept_reply(names[g], 0, 101, 0, 100, 0, [1]) for g in range(n)]
    st = wh.decode(frames).f_status
    assert (st[:100] == W.W_NOGROUP).all() and (st[100:] == W.W_OK).all()
    H.close()


# 7 ---- round trip: pause, run on, restore from the returned rows, run on ---------------------------------------------------------
def test_round_trip_through_the_returned_rows(hip_lib, oracle_lib):
    from tests.parity_common import make_pair, create_mixed_groups, fuzz

    G, kmax, nodes = 700, 5, [100, 101, 102, 103, 104]
    rng = np.random.default_rng(11)
    eh, eo = make_pair(hip_lib, oracle_lib, 100, G, kmax, 8)
    members, ks = create_mixed_groups(eh, eo, G, kmax, nodes, rng)
    fuzz(eh, eo, G, nodes, rng, 30, 400)
    # a forced pause of everything that can be paused: orc_group_retire(PAUSE) is the model AND the oracle's lockstep step
    g = np.arange(G, dtype=np.int32)
    rows_o, st_o = eo.retire_groups(g)
    ok = np.nonzero(st_o == S_OK)[0]
    out, counts = call_dev(eh, None, G, 0, 0, G)
    assert (counts.n_hits, counts.n_nogroup, counts.n_busy, counts.n_paused) == (ok.size, 0, G - ok.size, ok.size)
    assert 0 < ok.size < G
    assert out[0][:ok.size].tolist() == ok.tolist() and out[2][:ok.size].tobytes() == rows_o[ok].tobytes()
    assert all(untouched(a[ok.size:]) for a in out)
    fuzz(eh, eo, G, nodes, rng, 20, 400)
    for e in (eh, eo):
        assert (e.create_groups(ok, members[ok], ks[ok], out[2][:ok.size]) == S_OK).all()
    fuzz(eh, eo, G, nodes, rng, 30, 400)                                    # ends with every group's dump compared
    eh.close()
    eo.close()


# 8 ---- a listed sweep ---------------------------------------------------------------------------------------------------------
def test_listed_sweep_with_dead_rows_and_entries_out_of_range(hip_lib, oracle_lib):
    H = history(hip_lib, oracle_lib, G3)
    dead = np.arange(10, G3, 97, dtype=np.int32)
    H.do(lambda e: e.retire_groups(dead, 1))
    rng = np.random.default_rng(5)
    lst = rng.permutation(np.arange(0, G3, 3))
    lst = np.concatenate([lst[:500], [-1, G3, G3 + 5, -2**31, 2**31 - 1], lst[500:]]).astype(np.int32)
    assert lst.size % 64 and np.unique(lst).size == lst.size and np.isin(dead, lst).any()
    check(H, 1, 0, lst.size, "dev", gidx=lst, what="listed, first")
    H.do(lambda e: SC.touch(e, np.setdiff1d(lst[20::2], np.concatenate([dead, [-1, G3, G3 + 5, -2**31, 2**31 - 1]])), 0))
    r, groups = peek_both(H, 1, 0, lst.size, gidx=lst, what="listed")
    assert r["counts"][1] == 5 + np.isin(dead, lst).sum() and r["counts"][0] > 300
    r, groups = check(H, 1, 0, 200, "dev", gidx=lst, what="listed, cut")
    assert groups[r["hits"]].tolist() == [g for g in lst.tolist() if g in set(groups[r["hits"]].tolist())]
    check(H, 1, M.HOLD, lst.size, "host", gidx=lst, what="listed, the rest")
    ages_agree(H, "listed")
    liveness_agrees(H)
    H.close()


# 9 ---- many tiles -------------------------------------------------------------------------------------------------------------
def many_tiles(hip_lib, oracle_lib, n):
    """one hit in 1,000: expected by construction (every group but the hits gets traffic between the two sweeps), rows
    from the oracle's snapshot; which kernels ran, from the engine's profile"""
    eh, eo = SC.engine(hip_lib, n), SC.engine(oracle_lib, n)
    hits = np.arange(0, n, 1000, dtype=np.int32)
    others = np.setdiff1d(np.arange(n, dtype=np.int32), hits)
    out, counts = call_host(eh, None, n, 1, 0, n)
    assert (counts.n_hits, counts.n_nogroup, counts.n_busy, counts.n_paused) == (0, 0, 0, 0)
    for e in (eh, eo):
        SC.touch(e, others, 0)
    rows, _ = eo.snapshot(hits)
    eh.profile(2)
    out, counts = call_dev(eh, None, n, 1, 0, hits.size + 7)
    prof = eh.profile_read()
    eh.profile(0)
    assert (counts.n_hits, counts.n_nogroup, counts.n_busy, counts.n_paused) == (hits.size, 0, 0, hits.size)
    assert out[0][:hits.size].tolist() == hits.tolist() and set(out[1][:hits.size].tolist()) == {1}
    assert out[2][:hits.size].tobytes() == rows.tobytes() and all(untouched(a[hits.size:]) for a in out)
    assert {k: v[0] for k, v in prof.items()} == {"k_sweep_tile": 1, "k_sweep_offsets": 1, "k_sweep_move": 1}, sorted(prof)
    _, st = eo.retire_groups(hits)
    assert (st == S_OK).all()
    sample = np.concatenate([hits[:50], others[:50], others[-50:], hits[-50:]])
    (rh, sh), (ro, so) = eh.snapshot(sample), eo.snapshot(sample)
    assert sh.tolist() == so.tolist() and rh.tobytes() == ro.tobytes()
    eh.close()
    eo.close()


def test_130561_groups_one_hit_in_a_thousand(hip_lib, oracle_lib):
    many_tiles(hip_lib, oracle_lib, 130561)


@pytest.mark.skipif(os.environ.get("GPX_FULL_MATRIX") != "1", reason="the untrimmed matrix: GPX_FULL_MATRIX=1")
def test_a_million_groups_one_hit_in_a_thousand(hip_lib, oracle_lib):
    many_tiles(hip_lib, oracle_lib, (1 << 20) + 1)


def test_capacity_limit_and_a_sweep_after_a_refusal(hip_lib):
    import ctypes as C

    eh = SC.engine(hip_lib, 100)
    counts = sweep.SweepCounts()
    n_max = max(int(eh.cfg.max_groups), int(eh.cfg.max_batch))
    assert eh.lib.fn["pause_sweep"](eh.h, n_max + 1, None, 1, 0, 0, None, None, None, C.byref(counts)) == -2
    (g, a, rows), counts = sweep.pause_sweep(eh, None, min_age=0)
    assert g.tolist() == list(range(100)) and counts.n_paused == 100 and rows.dtype == HRI_DTYPE
    eh.close()
