#!/usr/bin/env python
"""The hit-compacting scans (include/gpx_scan.h) against the dense scans they stand beside (not the judged bench line).

One engine per scan, 1 M groups x 3 replicas, window 8.  Each scan is measured at four hit densities - none, 1 in 1,000,
1 in 3 (a failover: about one group in K) and all - and every cell runs, in ONE process with the repetitions of its legs
interleaved (median and spread reported, as scripts/bench_packed_votes.py does):
  dense          the dense host call (gpx_election_scan / gpx_poke_scan / gpx_gap_scan), pageable outputs: the yardstick
  hits_pageable  the hits host call into pageable memory
  hits_pinned    the hits host call into gpx_host_alloc memory
  dev            the _dev form between device events on the engine's stream, and its per-kernel split (gpx_profile_read)
The bytes that cross the link follow from the layouts and are asserted: dense 10 / 23 / 22 B per scanned group (the gap
scan's 22 are 18 out and the 4 of the gidx it must be given), hits 13 / 26 / 21 B per hit plus 16 B of counts.  Last, the resident failover burst of scripts/bench_election.py with
gpx_election_scan_hits_dev -> gpx_election_begin_hits_dev in front: the scan inside the event bracket."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DENSITIES = ("none", "1_in_1000", "1_in_3", "all")
# bytes the dense call moves per scanned group, from its columns: run 1 + p_bnum 4 + p_first 4 + status 1; poke 1 + four
# int32 + flags 1 + heard 4 + status 1; first 4 + max_committed 4 + missing 8 + sync 1 + status 1 out and the gidx the dense
# gap scan must be given, 4 in
DENSE_BYTES = {"election": 10, "poke": 23, "gap": 18}
DENSE_BYTES_IN = {"election": 0, "poke": 0, "gap": 4}


def classes(G):
    """class 0: one group in 1,000; class 1: the other multiples of 3; class 2: the rest.  Density d = classes < d."""
    g = np.arange(G)
    return np.where(g % 1000 == 0, 0, np.where(g % 3 == 0, 1, 2)).astype(np.int32)


def expected_hits(G, d):
    return int((classes(G) < d).sum())


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2] * 1e3, 4), "min_ms": round(xs[0] * 1e3, 4), "max_ms": round(xs[-1] * 1e3, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    ap.add_argument("--no-burst", action="store_true", help="skip the failover burst")
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()
    from gigapaxos_amd import Engine, hri_create, load_hip, make_hri, S_OK, C_HASVALUE
    from gigapaxos_amd import scan
    from gigapaxos_amd import wire as W
    from gigapaxos_amd.scan import ELECTION_COLS, POKE_COLS, GAP_COLS, HIT_BYTES

    G, K, R = a.groups, 3, a.reps
    lib = load_hip()
    cls = classes(G)
    allg = np.arange(G, dtype=np.int32)
    mem = np.tile(np.array([100, 101, 102], np.int32), (G, 1))
    dev = torch.device("cuda:0")
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(ts)
    out = {"config": {"groups": G, "k": K, "window": 8, "reps_per_leg": R, "tile": scan.SCAN_TILE}, "scans": {}}

    def engine(my_id, rows):
        e = Engine(lib, my_id, G, kmax=K, window=8, max_batch=G + 1024)
        assert (e.create_groups(allg, mem, K, rows) == S_OK).all()
        e.set_stream(ts.cuda_stream)
        return e

    def measure(kind, e, cols, dense_call, hits_call, dev_call, d, want):
        """One cell: the four legs interleaved, R repetitions each"""
        assert sum(np.dtype(dt).itemsize for _, dt in cols) == HIT_BYTES[kind]
        pageable = [np.zeros(G, dt) for _, dt in cols]
        pinned = [e.host_alloc(G, dt) for _, dt in cols]
        tdt = {1: torch.uint8, 4: torch.int32, 8: torch.int64}
        d_out = [torch.zeros(G, dtype=tdt[np.dtype(dt).itemsize], device=dev) for _, dt in cols]
        d_cnt = torch.zeros(4, dtype=torch.int32, device=dev)
        ptrs = [t.data_ptr() for t in d_out]
        torch.cuda.synchronize()
        times = {leg: [] for leg in ("dense", "hits_pageable", "hits_pinned", "dev")}
        legs = list(times)
        for rep in range(R + 1):                                   # the first repetition warms every leg
            for j in range(len(legs)):
                leg = legs[(rep + j) % len(legs)]                  # the order rotates
                if leg == "dense":
                    t0 = time.perf_counter()
                    dn = dense_call()
                    dt_ = time.perf_counter() - t0
                    assert sum(c.dtype.itemsize for c in dn) == DENSE_BYTES[kind] and all(c.shape[0] == G for c in dn)
                elif leg == "dev":
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ev0.record(ts)
                    dev_call(ptrs, d_cnt.data_ptr())
                    ev1.record(ts)
                    torch.cuda.synchronize()
                    dt_ = ev0.elapsed_time(ev1) * 1e-3
                    assert d_cnt.cpu().tolist() == [want, 0, 0, 0]
                else:
                    o = pageable if leg == "hits_pageable" else pinned
                    t0 = time.perf_counter()
                    hc, counts = hits_call(o)
                    dt_ = time.perf_counter() - t0
                    assert counts.n_hits == want and counts.n_nogroup == 0 and hc[0].shape[0] == want
                if rep:
                    times[leg].append(dt_)
        e.profile(2)
        for _ in range(R):
            dev_call(ptrs, d_cnt.data_ptr())
        e.sync()
        prof = e.profile_read()
        e.profile(0)
        cell = {"hits": want, "bytes_over_the_link": {"dense": G * (DENSE_BYTES[kind] + DENSE_BYTES_IN[kind]),
                                                      "hits": want * HIT_BYTES[kind] + 16}}
        for leg in legs:
            cell[leg] = stats(times[leg])
        cell["dev_kernels_ms"] = {k: round(v[1] / v[0], 5) for k, v in sorted(prof.items()) if k.startswith("k_scan_")}
        for leg in ("hits_pageable", "hits_pinned"):
            cell[leg + "_over_dense"] = round(cell[leg]["median_ms"] / cell["dense"]["median_ms"], 3)
        del hc
        e.host_free(*pinned)
        return cell

    def crossover(cells, leg):
        slower = [d for d in DENSITIES if cells[d][leg + "_over_dense"] > 1.0]
        return slower[0] if slower else "never (faster than dense at every density measured)"

    # ---- election: the ballot coordinator of a group is 201 + its class; me = 101 holds no coordinator ------------------
    rows = hri_create(G, K, 100)
    rows["acc_bcoord"] = 201 + cls
    rows["coord_bcoord"] = rows["acc_bcoord"]
    e = engine(101, rows)
    we = W.WireEngine(e)
    cells = {}
    for d, name in enumerate(DENSITIES):
        ids = tuple(range(201, 201 + d))
        cells[name] = measure(
            "election", e, ELECTION_COLS, lambda: W.election_scan(we, None, ids, ids),
            lambda o: scan.election_scan_hits(e, None, ids, ids, out=o),
            lambda p, c: scan.election_scan_hits_dev(e, G, 0, ids, ids, False, G, p, c), d, expected_hits(G, d))
    out["scans"]["election"] = {"cells": cells, "slower_than_dense_from": {leg: crossover(cells, leg) for leg in
                                                                           ("hits_pageable", "hits_pinned")}}
    e.close()

    # ---- gap: every group at slot 2 with a decision 5 / 3 / 1 slots ahead by class; the threshold picks the density --------
    rows = hri_create(G, K, 100)
    rows["acc_slot"] = 2
    rows["acc_gc_slot"] = 1
    rows["next_proposal_slot"] = 2
    e = engine(100, rows)
    we = W.WireEngine(e)
    z = np.zeros(G, np.int32)
    ahead = np.array([5, 3, 1], np.int32)[cls]
    st, _ = e.commit(allg, z, np.full(G, 100, np.int32), 2 + ahead, z, np.full(G, C_HASVALUE, np.uint8))
    assert (st == S_OK).all()
    req = scan.GAP_HIT_SYNC | scan.GAP_HIT_MISSING
    cells = {}
    for d, (name, thr) in enumerate(zip(DENSITIES, (1000, 5, 3, 1))):
        cells[name] = measure(
            "gap", e, GAP_COLS, lambda: W.gap_scan(we, allg, thr),
            lambda o: scan.gap_scan_hits(e, None, thr, require=req, out=o),
            lambda p, c: scan.gap_scan_hits_dev(e, G, 0, thr, 0, 64, req, G, p, c), d, expected_hits(G, d))
    out["scans"]["gap"] = {"cells": cells, "slower_than_dense_from": {leg: crossover(cells, leg) for leg in
                                                                      ("hits_pageable", "hits_pinned")}}
    e.close()

    # ---- poke: proposals are made class by class, the densities in ascending order ------------------------------------------
    e = engine(100, hri_create(G, K, 100))
    cells = {}
    for d, name in enumerate(DENSITIES):
        if d:
            g = allg[cls == d - 1]
            assert (e.propose(g)[4] == S_OK).all()
        cells[name] = measure(
            "poke", e, POKE_COLS, lambda: e.poke_scan(None), lambda o: scan.poke_scan_hits(e, None, out=o),
            lambda p, c: scan.poke_scan_hits_dev(e, G, 0, G, p, c), d, expected_hits(G, d))
    out["scans"]["poke"] = {"cells": cells, "slower_than_dense_from": {leg: crossover(cells, leg) for leg in
                                                                       ("hits_pageable", "hits_pinned")}}
    e.close()

    if not a.no_burst:
        try:
            out["failover_burst_resident"] = failover_burst(torch, lib, G, ts)
        except Exception as x:  # noqa: BLE001  (a side measurement: the table above stands without it)
            out["failover_burst_resident"] = {"not_measured": repr(x)}
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def failover_burst(torch, lib, G, ts):
    """scripts/bench_election.py's resident burst - every group fails over at once - with the scan in front and inside the
    event bracket: scan_hits_dev -> begin_hits_dev (the count stays on the device) -> propose_h_dev -> prepare_reply_dev.
    Between bursts the dead node's ballot is raised by a PREPARE (untimed), so that the next scan finds every group again."""
    from gigapaxos_amd import Engine, make_hri, S_OK, scan

    K, Wn = 3, 8
    dev = torch.device("cuda:0")
    e = Engine(lib, 1, G, kmax=K, window=Wn, max_batch=2 * G + 1024)
    rows = make_hri(G)
    rows["acc_slot"] = 5
    rows["acc_gc_slot"] = 4
    rows["next_proposal_slot"] = -1
    allg = np.arange(G, dtype=np.int32)
    assert (e.create_groups(allg, np.tile(np.array([0, 1, 2], np.int32), (G, 1)), K, rows) == S_OK).all()
    e.set_stream(ts.cuda_stream)
    rng = np.random.default_rng(0)
    pre = allg[rng.random(G) < 0.3]
    n = 2 * G
    perm = rng.permutation(n)
    gi = np.concatenate([allg, allg])[perm].astype(np.int32)
    acc = np.concatenate([np.full(G, 1, np.int32), np.full(G, 2, np.int32)])[perm]
    has = rng.random(n) < 0.5
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum(has)
    m = int(off[n])
    T = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    VP = lambda t_: C.c_void_p(t_.data_ptr())  # noqa: E731
    d_pre, d_h = T(pre), T(np.arange(1, pre.size + 1, dtype=np.int64))
    d_gi, d_acc, d_rc, d_first, d_off = T(gi), T(acc), T(np.full(n, 1, np.int32)), T(np.full(n, 5, np.int32)), T(off)
    d_ps = T((5 + rng.integers(0, 2, m)).astype(np.int32))
    d_pbn, d_pbc, d_pfl = T(np.zeros(m, np.int32)), T(np.zeros(m, np.int32)), T(np.zeros(m, np.uint8))
    d_ph = T((10 ** 9 + np.arange(m)).astype(np.int64))
    o_g, o_b, o_f = (torch.zeros(G, dtype=torch.int32, device=dev) for _ in range(3))
    o_r, o_es = (torch.zeros(G, dtype=torch.uint8, device=dev) for _ in range(2))
    cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    o_p = [torch.zeros(pre.size, dtype=torch.int32, device=dev) for _ in range(4)]
    o_pst = torch.zeros(pre.size, dtype=torch.uint8, device=dev)
    o_vk, o_st = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2))
    o_ec, o_em = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))
    o_es_ = torch.zeros(n * Wn, dtype=torch.int32, device=dev)
    o_ek, o_ef = (torch.zeros(n * Wn, dtype=torch.uint8, device=dev) for _ in range(2))
    o_eh = torch.zeros(n * Wn, dtype=torch.int64, device=dev)
    res = {}
    for it in range(3):                                            # the last burst is reported
        if it:
            e.prepare(allg, np.full(G, 2 * it, np.int32), np.zeros(G, np.int32), np.full(G, 5, np.int32))
        d_rb = torch.full((n,), 2 * it + 1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record(ts)
        scan.election_scan_hits_dev(e, G, 0, (0,), (), False, G,
                                    [o_g.data_ptr(), o_r.data_ptr(), o_b.data_ptr(), o_f.data_ptr()], cnt.data_ptr())
        ev[1].record(ts)
        scan.election_begin_hits_dev(e, G, cnt.data_ptr(), o_g.data_ptr(), o_b.data_ptr(), o_es.data_ptr())
        ev[2].record(ts)
        lib.check(lib.fn["propose_batch_h_dev"](e.h, pre.size, VP(d_pre), None, VP(d_h), VP(o_p[0]), VP(o_p[1]),
                                                VP(o_p[2]), VP(o_p[3]), VP(o_pst)), "propose_batch_h_dev")
        ev[3].record(ts)
        lib.check(lib.fn["prepare_reply_batch_dev"](e.h, n, VP(d_gi), VP(d_acc), VP(d_rb), VP(d_rc), VP(d_first),
                                                    VP(d_off), m, VP(d_ps), VP(d_pbn), VP(d_pbc), VP(d_ph), VP(d_pfl),
                                                    VP(o_vk), VP(o_ec), VP(o_em), VP(o_es_), VP(o_ek), VP(o_eh),
                                                    VP(o_ef), VP(o_st)), "prepare_reply_batch_dev")
        ev[4].record(ts)
        torch.cuda.synchronize()
        assert cnt.cpu().tolist() == [G, 0, 0, 0] and int((o_b == 2 * it + 1).sum()) == G
        assert int((o_es == 0).sum()) == G and int((o_pst == 8).sum()) == pre.size and int((o_vk == 2).sum()) == G
        names = ("election_scan_hits", "election_begin_hits", "propose_preactive", "prepare_reply")
        res = {k: round(ev[i].elapsed_time(ev[i + 1]), 4) for i, k in enumerate(names)}
        res["total"] = round(ev[0].elapsed_time(ev[4]), 4)
    res["view_changes_per_sec_resident"] = round(G / (res["total"] * 1e-3))
    res["what"] = f"{G} groups x 3, every group fails over at once; gpu ms between device events, third burst"
    e.close()
    return res


if __name__ == "__main__":
    main()
