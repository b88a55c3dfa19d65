#!/usr/bin/env python
"""The failover burst of scripts/bench_election.py (same seeds), its PREPARE replies applied through the dense calls and
through the list calls of include/gpx_viewchange.h, in ONE process, alternating: the dense host-pointer call, the list
host-pointer call and both _dev forms with events - and the acceptor pair over one PREPARE per group.  Not the judged
bench line; the numbers go to profiles/ and DESIGN.md.

Every pass is a fresh election (the next ballot): begin, pre-active proposals, then the 2 G replies through one form.
Link bytes are computed from the shapes."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gigapaxos_amd import Engine, load_hip, make_hri, S_OK  # noqa: E402
from gigapaxos_amd import viewchange as V  # noqa: E402
from gigapaxos_amd._abi import PlCounts, PrlCounts  # noqa: E402


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2] * 1e3, 3), "min_ms": round(xs[0] * 1e3, 3), "max_ms": round(xs[-1] * 1e3, 3),
            "runs": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    G, K, Wn, R = args.groups, 3, 8, args.repeats
    torch.cuda.init()  # before the engine's own HIP calls: one runtime, torch's
    lib = load_hip()
    e = Engine(lib, 1, G, kmax=K, window=Wn, max_batch=2 * G + 1024)
    rows = make_hri(G)
    rows["acc_slot"] = 5
    rows["acc_gc_slot"] = 4
    rows["next_proposal_slot"] = -1
    mem = np.tile(np.array([0, 1, 2], np.int32), (G, 1))
    allg = np.arange(G, dtype=np.int32)
    assert (e.create_groups(allg, mem, K, rows) == S_OK).all()
    rng = np.random.default_rng(0)
    # ---- the burst's columns (bench_election.py's draws, in its order) ----
    pre = allg[rng.random(G) < 0.3]
    n = 2 * G
    perm = rng.permutation(n)
    gi = np.concatenate([allg, allg])[perm].astype(np.int32)
    acc = np.concatenate([np.full(G, 1, np.int32), np.full(G, 2, np.int32)])[perm]
    has = rng.random(n) < 0.5
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum(has)
    m = int(off[n])
    ps = (5 + rng.integers(0, 2, m)).astype(np.int32)
    pbn, pbc = np.zeros(m, np.int32), np.zeros(m, np.int32)
    ph = (10 ** 9 + np.arange(m)).astype(np.int64)
    pfl = np.zeros(m, np.uint8)
    rc, first = np.full(n, 1, np.int32), np.full(n, 5, np.int32)
    pre_h = np.arange(1, pre.size + 1, dtype=np.int64)
    ballot = [0]

    def new_election():
        ballot[0] += 1
        assert (e.election_begin(allg, np.full(G, ballot[0], np.int32)) == 0).all()
        assert (e.propose(pre, handle=pre_h)[4] == 8).all()
        return np.full(n, ballot[0], np.int32)

    # dense outputs
    vk, stt = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    ec, em = np.zeros(n, np.int32), np.zeros(n, np.int32)
    es_, ek, ef = np.zeros(n * Wn, np.int32), np.zeros(n * Wn, np.uint8), np.zeros(n * Wn, np.uint8)
    eh = np.zeros(n * Wn, np.int64)
    # list outputs: every group is elected once, at most W entries each (the run needs far fewer)
    cap_h, cap_e = n, 4 * G
    hc = [np.zeros(cap_h, dt) for _, dt in V.HIT_COLS]
    ecl = [np.zeros(cap_e, dt) for _, dt in V.ENTRY_COLS]
    counts = PrlCounts()

    def dense_host(rb):
        t0 = time.perf_counter()
        lib.check(lib.fn["prepare_reply_batch"](e.h, n, _p(gi), _p(acc), _p(rb), _p(rc), _p(first), _p(off), _p(ps), _p(pbn),
                                                _p(pbc), _p(ph), _p(pfl), _p(vk), _p(ec), _p(em), _p(es_), _p(ek), _p(eh),
                                                _p(ef), _p(stt)), "prepare_reply_batch")
        dt = time.perf_counter() - t0
        assert int((vk == 2).sum()) == G and not stt.any()
        return dt

    def list_host(rb):
        t0 = time.perf_counter()
        lib.check(lib.fn["prepare_reply_lists"](e.h, n, _p(gi), _p(acc), _p(rb), _p(rc), _p(first), _p(off), _p(ps), _p(pbn),
                                                _p(pbc), _p(ph), _p(pfl), _p(vk), _p(stt), cap_h, cap_e, *[_p(a) for a in hc],
                                                *[_p(a) for a in ecl], C.byref(counts)), "prepare_reply_lists")
        dt = time.perf_counter() - t0
        assert counts.n_hits == counts.hits_done == G == counts.n_elected and counts.entries_done == counts.n_entries
        assert int((vk == 2).sum()) == G and not stt.any()
        return dt

    host = {"dense": [], "lists": []}
    checked = False
    for it in range(2 * (R + 1)):           # one unreported pass of each first (scratch, lazily allocated tables)
        form = "dense" if it % 2 == 0 else "lists"
        dt = (dense_host if form == "dense" else list_host)(new_election())
        if it >= 2:
            host[form].append(dt)
        if form == "lists" and not checked:   # the lists say what the planes of the pass before said
            k = int(counts.hits_done)
            r = hc[0][:k]
            assert (hc[6][:k] == ec[r]).all() and int(hc[6][:k].sum()) == counts.entries_done == int(ec.sum())
            j0 = hc[5][:k]
            nz = hc[6][:k] > 0
            assert (ecl[0][j0[nz]] == es_[r[nz]]).all() and (ecl[2][j0[nz]] == eh[r[nz]]).all()
            checked = True
    n_entries, n_hits = int(counts.n_entries), int(counts.n_hits)

    # ---- every column resident: the two _dev forms, alternating, with events on the engine's stream ----
    dev = torch.device("cuda:0")
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(ts)
    e.set_stream(ts.cuda_stream)
    T = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    VP = lambda t_: C.c_void_p(t_.data_ptr())  # noqa: E731
    d_allg, d_pre, d_h = T(allg), T(pre), T(pre_h)
    d_gi, d_acc, d_rc, d_first, d_off = T(gi), T(acc), T(rc), T(first), T(off)
    d_ps, d_pbn, d_pbc, d_ph, d_pfl = T(ps), T(pbn), T(pbc), T(ph), T(pfl)
    o_es = torch.zeros(G, dtype=torch.uint8, device=dev)
    o_p = [torch.zeros(pre.size, dtype=torch.int32, device=dev) for _ in range(4)]
    o_pst = torch.zeros(pre.size, dtype=torch.uint8, device=dev)
    o_vk, o_st = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2))
    o_ec, o_em = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))
    o_es_ = torch.zeros(n * Wn, dtype=torch.int32, device=dev)
    o_ek, o_ef = (torch.zeros(n * Wn, dtype=torch.uint8, device=dev) for _ in range(2))
    o_eh = torch.zeros(n * Wn, dtype=torch.int64, device=dev)
    l_h = [T(np.zeros(cap_h, dt)) for _, dt in V.HIT_COLS]
    l_e = [T(np.zeros(cap_e, dt)) for _, dt in V.ENTRY_COLS]
    l_c = torch.zeros(8, dtype=torch.int32, device=dev)
    resident = {"dense": [], "lists": []}
    e.profile(2)
    for it in range(2 * (R + 1)):
        form = "dense" if it % 2 == 0 else "lists"
        ballot[0] += 1
        d_bn = torch.full((G,), ballot[0], dtype=torch.int32, device=dev)
        d_rb = torch.full((n,), ballot[0], dtype=torch.int32, device=dev)
        lib.check(lib.fn["election_begin_dev"](e.h, G, VP(d_allg), VP(d_bn), VP(o_es)), "election_begin_dev")
        lib.check(lib.fn["propose_batch_h_dev"](e.h, pre.size, VP(d_pre), None, VP(d_h), VP(o_p[0]), VP(o_p[1]), VP(o_p[2]),
                                                VP(o_p[3]), VP(o_pst)), "propose_batch_h_dev")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        if form == "dense":
            lib.check(lib.fn["prepare_reply_batch_dev"](e.h, n, VP(d_gi), VP(d_acc), VP(d_rb), VP(d_rc), VP(d_first), VP(d_off),
                                                        m, VP(d_ps), VP(d_pbn), VP(d_pbc), VP(d_ph), VP(d_pfl), VP(o_vk),
                                                        VP(o_ec), VP(o_em), VP(o_es_), VP(o_ek), VP(o_eh), VP(o_ef), VP(o_st)),
                      "prepare_reply_batch_dev")
        else:
            lib.check(lib.fn["prepare_reply_lists_dev"](e.h, n, VP(d_gi), VP(d_acc), VP(d_rb), VP(d_rc), VP(d_first), VP(d_off),
                                                        m, VP(d_ps), VP(d_pbn), VP(d_pbc), VP(d_ph), VP(d_pfl), VP(o_vk),
                                                        VP(o_st), cap_h, cap_e, *[VP(x) for x in l_h], *[VP(x) for x in l_e],
                                                        VP(l_c)), "prepare_reply_lists_dev")
        ev[1].record()
        torch.cuda.synchronize()
        assert int((o_vk == 2).sum()) == G
        if form == "lists":
            assert l_c.cpu().numpy()[[0, 3, 5]].tolist() == [G, G, G]
        if it >= 2:
            resident[form].append(ev[0].elapsed_time(ev[1]) * 1e-3)
    prof = {k: v for k, v in e.profile_read().items() if k.startswith(("k_vl_", "k_bucket_prepare_reply", "k_hist", "k_scatter"))}

    # ---- the acceptor pair: one PREPARE per group; half of the groups have accepted slot 5, a quarter slot 6 too ----
    torch.cuda.synchronize()
    half, quarter = allg[::2].copy(), allg[::4].copy()
    for sel, slot in ((half, 5), (quarter, 6)):
        r = e.accept(sel, np.zeros(sel.size, np.int32), np.zeros(sel.size, np.int32), np.full(sel.size, slot, np.int32),
                     np.full(sel.size, 4, np.int32))
        assert (r[0][4] == S_OK).all()
    a_bn, a_bc, a_fs = np.full(G, 1 << 20, np.int32), np.full(G, 1, np.int32), np.full(G, 5, np.int32)
    rbn, rbc, rgc = (np.zeros(G, np.int32) for _ in range(3))
    rfl, rst = np.zeros(G, np.uint8), np.zeros(G, np.uint8)
    pm = np.zeros(G, np.uint64)
    pls, plb, plc = (np.zeros(G * Wn, np.int32) for _ in range(3))
    cap_pv = G
    pvo = np.zeros(G + 1, np.int32)
    pvs, pvb, pvc = (np.zeros(cap_pv, np.int32) for _ in range(3))
    pc = PlCounts()
    acceptor = {"dense": [], "lists": []}
    for it in range(2 * (R + 1)):
        form = "dense" if it % 2 == 0 else "lists"
        t0 = time.perf_counter()
        if form == "dense":
            lib.check(lib.fn["prepare_batch"](e.h, G, _p(allg), _p(a_bn), _p(a_bc), _p(a_fs), _p(rbn), _p(rbc), _p(rgc), _p(rfl),
                                              _p(pm), _p(pls), _p(plb), _p(plc), _p(rst)), "prepare_batch")
        else:
            lib.check(lib.fn["prepare_lists"](e.h, G, _p(allg), _p(a_bn), _p(a_bc), _p(a_fs), _p(rbn), _p(rbc), _p(rgc), _p(rfl),
                                              _p(rst), cap_pv, _p(pvo), _p(pvs), _p(pvb), _p(pvc), C.byref(pc)), "prepare_lists")
            assert pc.recs_done == G and pc.entries_done == pc.n_entries == half.size + quarter.size
        dt = time.perf_counter() - t0
        if it >= 2:
            acceptor[form].append(dt)
    assert int((pm != 0).sum()) == half.size and int(pvo[G]) == pc.n_entries

    in_bytes = n * 20 + (n + 1) * 4 + m * 21
    out = {
        "workload": f"{G} groups x 3 replicas, every group fails over at once; {n} PREPARE replies, {m} pvalues, window {Wn}; "
                    f"{n_hits} hits, {n_entries} list entries; acceptor pair: {G} PREPAREs, {int(pc.n_entries)} pvalues",
        "repeats_per_form": R,
        "coordinator_host_pointer": {k: stats(v) for k, v in host.items()},
        "coordinator_resident": {k: stats(v) for k, v in resident.items()},
        "acceptor_host_pointer": {k: stats(v) for k, v in acceptor.items()},
        "link_bytes": {
            "coordinator_in": in_bytes,
            "coordinator_out_dense": n * (10 + 14 * Wn),
            "coordinator_out_lists": n * 2 + 32 + n_hits * V.HIT_BYTES + n_entries * V.ENTRY_BYTES,
            "acceptor_in": G * 16,
            "acceptor_out_dense": G * (22 + 12 * Wn),
            "acceptor_out_lists": G * 14 + (G + 1) * 4 + 32 + int(pc.n_entries) * V.PV_BYTES,
        },
        "kernel_ms_total_resident_passes": {k: [int(v[0]), round(v[1], 4)] for k, v in sorted(prof.items())},
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    e.close()


if __name__ == "__main__":
    main()
