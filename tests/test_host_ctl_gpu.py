"""The twenty control-plane host-pointer calls on the GPU, each against the CPU oracle: one history applied to a HIP engine
and to the oracle, every output of every call compared byte for byte.  The hit-compacting scans and the sweep have no
oracle form: their expected answers are tests/scan_hits_model.py and tests/sweep_model.py over the oracle's dense scans,
as in tests/test_scan_hits_gpu.py and tests/test_pause_sweep_gpu.py.

Shapes: n = 0, 1 and 1,001 (no multiple of 4: every 16-byte path has a tail); capacities below, at and above the hit
count; the lifecycle calls over 262,145 groups (one chunk of 2^18 and one record); one engine through a small, a large
and a small call again, so that the arena of temporary device columns grows and is rewound."""
import numpy as np
import pytest

from gigapaxos_amd import hri_create, S_OK, S_NOGROUP, S_BUSY, RETIRE_KILL, RETIRE_PAUSE
from gigapaxos_amd import scan, sweep
from gigapaxos_amd import wire as W
from tests import scan_hits_model as HM
from tests import sweep_model as SM
from tests.parity_common import make_pair

pytestmark = pytest.mark.gpu

ME = 100
SIZES = (0, 1, 1001)


def i32(n, v=0):
    return np.full(n, v, np.int32)


def pair_of(hip_lib, oracle_lib, n_groups, max_batch=4096):
    """(HIP engine, oracle engine), as the other parity tests build them"""
    return make_pair(hip_lib, oracle_lib, ME, n_groups, 3, 8, max_batch=max_batch)


def create(e, n):
    g = np.arange(n, dtype=np.int32)
    mem = np.zeros((n, 3), np.int32)
    mem[:] = (ME, ME + 1, ME + 2)
    rows = hri_create(n, 3, ME)
    rows["node_slots"][:, :3] = (g[:, None] * 7 + np.arange(3)[None, :] * 3) % 5
    return e.create_groups(g, mem, 3, rows)


def same_traces(a, b):
    assert [x[0] for x in a] == [x[0] for x in b]
    for (label, xs), (_, ys) in zip(a, b):
        assert len(xs) == len(ys), label
        for k, (x, y) in enumerate(zip(xs, ys)):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (label, k)


def twins_trace(e, n):
    """Seventeen of the twenty calls over n records on one engine of n + 8 groups (the lifecycle ones included)."""
    G = n + 8
    we = W.WireEngine(e)
    g = np.arange(n, dtype=np.int32)
    out = []

    def rec(label, *arrays):
        out.append((label, [np.ascontiguousarray(a).copy() for a in arrays]))

    rec("group_create", create(e, n))
    names = [b"svc-%d" % i for i in range(n)]
    rec("names_bind", we.bind(names, g))
    rec("names_lookup", we.lookup(names[::-1]))
    rec("names_coordinator", W.names_coordinator(we, g[::-1].copy(), 1))
    # a list with entries out of range and a duplicate behind it
    lst = np.concatenate([g[::-1], [-1, G + 3, 0]]).astype(np.int32) if n else g
    rec("election_scan", *W.election_scan(we, lst, (ME,), (), False))
    rec("election_scan, forced, whole table", *W.election_scan(we, None, (), (ME + 2,), True))
    rec("gap_scan", *W.gap_scan(we, lst, 1))
    rec("poke_scan", *e.poke_scan(lst))
    sl, bn, bc, md, st = e.propose(g)
    rec("poke_scan, proposals outstanding, whole table", *e.poke_scan(None))
    d = e.accept_reply(np.concatenate([g, g]), i32(2 * n), i32(2 * n, ME), np.concatenate([sl, sl]),
                       np.concatenate([i32(n, ME), i32(n, ME + 1)]), i32(2 * n))
    assert d.gidx.shape[0] == n
    frames, fg, nb = we.pack_commits(d)
    rec("wire_pack_commits", np.frombuffer(b"".join(frames), np.uint8), fg, [nb], [len(f) for f in frames])
    votes = [W.batched_accept_reply(names[i], 0, ME + 1 + (i & 1), 0, ME, 2, [4, 5]) for i in range(n)]
    burst = votes + frames + ([W.batched_commit(b"unknown", 0, 0, ME, 0, [1], [ME + 1]), votes[0][:-3]] if n else [])
    for caps in ({}, dict(cap_votes=n // 3, cap_commits=n // 3, cap_accepts=0, cap_requests=0)):
        dec = we.decode(burst, **caps)
        rec("wire_decode %s" % sorted(caps), dec.f_status, dec.f_gidx, dec.f_type, *dec.votes.values(), *dec.commits.values(),
            *dec.accepts.values(), *dec.requests.values(), list(dec.counts.values()))
    (rb, rc, rm, rf, ast), _ = e.accept(g, i32(n), i32(n, ME), sl, i32(n))
    # 300 more replies of group 0: over the 256 of one pass, packed by a second pass
    idx = np.concatenate([g, i32(300)]) if n > 1 else g
    for sender, req in ((None, None), (i32(idx.size, ME), np.arange(idx.size, dtype=np.int64) * 7)):
        fr, pg, pd, ub, pb = we.pack_accept_replies(idx, sl[idx], rb[idx], rc[idx], rm[idx], ast[idx], sender, req)
        rec("wire_pack_accept_replies", np.frombuffer(b"".join(fr), np.uint8), pg, pd, ub, [pb], [len(f) for f in fr])
    dense, pv = e.prepare(g, i32(n, 1), i32(n, ME + 1), i32(n))
    rec("prepare_batch", *dense, np.array(pv, np.int64).reshape(-1, 4))
    est = (g * 37 % 900).astype(np.int32)
    for weight, stop in ((None, None), (1 + g % 3, (g % 17 == 5).astype(np.uint8))):
        leader, rst, b = W.request_batch(we, g, est, weight, stop, max_bytes=4096, max_size=16)
        rec("request_batch", leader, rst, *b.values())
    rec("election_begin", e.election_begin(g, i32(n, 2)))
    pvals = [[(3, 1, ME + 1, 50 + i, 0)] if i % 2 else [] for i in range(n)]
    for acceptor, pv_in in ((ME + 1, None), (ME + 2, pvals)):                   # the second reply is the majority
        (vk, em, pst), lists = e.prepare_reply(g, i32(n, acceptor), i32(n, 2), i32(n, ME), i32(n), pv_in)
        rec("prepare_reply_batch", vk, em, pst, [len(x) for x in lists], np.array([t for x in lists for t in x], np.int64))
    rec("names_unbind", we.unbind(g[::3].copy()))
    rec("group_snapshot", *e.snapshot(lst))
    rec("group_retire, kill", *e.retire_groups(g[::2].copy(), RETIRE_KILL))
    rec("group_retire, pause", *e.retire_groups(lst[:-1].copy() if n else lst, RETIRE_PAUSE))   # (no group twice)
    rec("group_snapshot afterwards", *e.snapshot(g))
    e.close()
    return out


@pytest.mark.parametrize("n", SIZES)
def test_every_dense_twin_against_the_oracle(hip_lib, oracle_lib, n):
    same_traces(*[twins_trace(e, n) for e in pair_of(hip_lib, oracle_lib, n + 8)])


# ---- the hit-compacting twins: the model over the oracle's dense scan ------------------------------------------------------
def scan_pair(hip_lib, oracle_lib, n):
    """Groups 0 .. n-1 on both; every third has a proposal outstanding (poke), every fifth a commit ahead (gap), the
    coordinator of every seventh is the node that is down (election)."""
    pair = pair_of(hip_lib, oracle_lib, n + 8)
    for e in pair:
        g = np.arange(n, dtype=np.int32)
        mem = np.zeros((n, 3), np.int32)
        mem[:] = (ME, ME + 1, ME + 2)
        rows = hri_create(n, 3, ME)
        rows["acc_bcoord"][::7] = ME + 2
        rows["coord_bcoord"][::7] = ME + 2
        rows["has_coord"][::7] = 0
        assert (e.create_groups(g, mem, 3, rows) == S_OK).all()
        own = np.setdiff1d(g, g[::7]).astype(np.int32)
        if own[::3].size:
            assert (e.propose(own[::3].copy())[4] == S_OK).all()
        ahead = g[::5].copy()
        if ahead.size:
            e.commit(ahead, i32(ahead.size), rows["acc_bcoord"][ahead], i32(ahead.size, 3), i32(ahead.size),
                     np.full(ahead.size, 1, np.uint8))
    return pair


@pytest.mark.parametrize("n", SIZES)
def test_hit_twins_at_capacities_around_the_hit_count(hip_lib, oracle_lib, n):
    eh, eo = scan_pair(hip_lib, oracle_lib, n)
    wo = W.WireEngine(eo)
    lst = np.concatenate([np.arange(n)[::-1], [-1, n + 9, 0]]).astype(np.int32) if n else None
    for gidx in (None, lst):
        groups = np.arange(n, dtype=np.int32) if gidx is None else gidx
        m = groups.shape[0]
        dense = {"election": W.election_scan(wo, groups, (ME + 2,), (), False), "poke": eo.poke_scan(groups),
                 "gap": W.gap_scan(wo, groups, 1)}
        calls = {"election": lambda cap: scan.election_scan_hits(eh, gidx, (ME + 2,), (), False, cap=cap, n=m),
                 "poke": lambda cap: scan.poke_scan_hits(eh, gidx, cap=cap, n=m),
                 "gap": lambda cap: scan.gap_scan_hits(eh, gidx, 1, require=scan.GAP_HIT_AHEAD, cap=cap, n=m)}
        for kind in ("election", "poke", "gap"):
            require = scan.GAP_HIT_AHEAD if kind == "gap" else 0
            hits = int(HM.hit_mask(kind, dense[kind], require).sum())
            assert n < 7 or hits > 2, kind
            for cap in sorted({0, max(hits - 1, 0), hits, hits + 3}):
                want, n_hits, n_nog = HM.compact(kind, dense[kind], groups, cap, require)
                got, counts = calls[kind](cap)
                assert (counts.n_hits, counts.n_nogroup) == (n_hits, n_nog) == (hits, n_nog), (kind, cap)
                if cap:
                    assert [a.tobytes() for a in got] == [np.ascontiguousarray(a).tobytes() for a in want], (kind, cap)
    eh.close()
    eo.close()


@pytest.mark.parametrize("n", SIZES)
def test_sweep_twin_at_capacities_around_the_hit_count(hip_lib, oracle_lib, n):
    """Groups never swept before: every caught-up one is a hit of age 0 at min_age 0.  Every third group has a proposal
    outstanding (busy); the list adds entries out of range.  PEEK calls change nothing; the last call pauses."""
    eh, eo = pair_of(hip_lib, oracle_lib, n + 8)
    g = np.arange(n, dtype=np.int32)
    for e in (eh, eo):
        assert (create(e, n) == S_OK).all()
        if g[::3].size:
            assert (e.propose(g[::3].copy())[4] == S_OK).all()
    lst = np.concatenate([g[::-1], [-1, n + 9]]).astype(np.int32) if n else None
    for gidx in (None, lst):
        groups = g if gidx is None else gidx
        m = groups.shape[0]
        rows, st = eo.snapshot(groups)
        live = st == S_OK
        busy = live & (np.isin(groups, g[::3]))
        hits = int((live & ~busy).sum())
        for cap in sorted({0, max(hits - 1, 0), hits, hits + 3}):
            want = SM.sweep(live, busy, np.ones(m, bool), np.zeros(m), 0, SM.PEEK, cap)
            (og, oa, orows), counts = sweep.pause_sweep(eh, gidx, 0, sweep.SWEEP_PEEK, cap=cap, n=m)
            assert (counts.n_hits, counts.n_nogroup, counts.n_busy, counts.n_paused) == tuple(want["counts"]), cap
            if cap:
                assert og.tolist() == groups[want["hits"]].tolist() and oa.tolist() == list(want["ages"])
                assert orows.tobytes() == rows[want["hits"]].tobytes()
    # the real thing: the first two hits leave the table
    cap = 2
    want = SM.sweep(np.ones(n, bool), np.isin(g, g[::3]), np.ones(n, bool), np.zeros(n), 0, 0, cap)
    (og, oa, orows), counts = sweep.pause_sweep(eh, None, 0, 0, cap=cap, n=n)
    assert og.tolist() == g[want["paused"]].tolist() and counts.n_paused == len(want["paused"])
    if og.size:
        orc_rows, orc_st = eo.retire_groups(og.copy(), RETIRE_PAUSE)
        assert (orc_st == S_OK).all() and orc_rows.tobytes() == orows.tobytes()
    assert [a.tobytes() for a in eh.snapshot(g)] == [a.tobytes() for a in eo.snapshot(g)]
    assert S_BUSY != S_NOGROUP
    eh.close()
    eo.close()


# ---- one chunk plus one record ------------------------------------------------------------------------------------------
def test_lifecycle_calls_over_one_chunk_and_one_record(hip_lib, oracle_lib):
    n = (1 << 18) + 1
    traces = []
    for e in pair_of(hip_lib, oracle_lib, n):
        g = np.arange(n, dtype=np.int32)
        t = [("group_create", [create(e, n)])]
        assert (t[0][1][0] == S_OK).all()
        t.append(("group_snapshot", list(e.snapshot(g[::-1].copy()))))
        t.append(("group_retire", list(e.retire_groups(g, RETIRE_PAUSE))))
        t.append(("group_snapshot afterwards", list(e.snapshot(g))))
        assert (t[3][1][1] == S_NOGROUP).all()
        traces.append(t)
        e.close()
    same_traces(*traces)


# ---- the arena: small, large, small ---------------------------------------------------------------------------------------
def test_one_engine_through_a_small_a_large_and_a_small_call(hip_lib, oracle_lib):
    G = 20001
    traces = []
    for e in pair_of(hip_lib, oracle_lib, G, max_batch=1 << 15):
        we = W.WireEngine(e)
        assert (create(e, G) == S_OK).all()
        t = []
        for n in (5, G, 5, 1001, G, 1):
            g = (np.arange(n, dtype=np.int32) * 7) % G                      # distinct: 7 does not divide G
            t.append(("poke_scan %d" % n, [np.ascontiguousarray(a) for a in e.poke_scan(g)]))
            t.append(("gap_scan %d" % n, [np.ascontiguousarray(a) for a in W.gap_scan(we, g, 1)]))
            dense, pv = e.prepare(g, i32(n, 1), i32(n, ME + 1), i32(n))
            t.append(("prepare_batch %d" % n, [np.ascontiguousarray(a) for a in dense]))
        traces.append(t)
        e.close()
    same_traces(*traces)
