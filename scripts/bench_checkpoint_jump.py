#!/usr/bin/env python
"""Checkpoint transfer (include/gpx_checkpoint.h) against the parent's only device-side way to the same state (a side
figure, not the judged bench line).

One engine, 1 M groups x 3 replicas, window 8, every group lagging by d = 1, 8, 64 and 100,000 slots.  Three legs move
THE SAME groups forward by d slots, their repetitions interleaved in one process (median and spread of seven):
  cp_dev   gpx_checkpoint_batch_dev, one record per group, timed between device events
  cp_host  gpx_checkpoint_batch, pageable columns, by the wall clock
  commit   gpx_commit_batch_dev with d valued decisions per group - d calls of one decision per group each, the batch
           ordered by group, between device events - at d = 1, 8 and 64; at d = 100,000 it cannot be run
No leg needs a reset: every leg leaves all groups d slots further on, which is where the next one starts.  The bytes that
cross the link for the host twin follow from the column layouts and are asserted: 8 in and 10 out per record, 12 per run,
16 of counts."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DISTANCES = (1, 8, 64, 100_000)
COMMIT_UP_TO = 64


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2] * 1e3, 4), "min_ms": round(xs[0] * 1e3, 4), "max_ms": round(xs[-1] * 1e3, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()
    from gigapaxos_amd import Engine, hri_create, load_hip, S_OK, C_HASVALUE
    from gigapaxos_amd import checkpoint as CK

    G, K, Wn, R = a.groups, 3, 8, a.reps
    dense = (np.int32, np.int32, np.uint8, np.uint8)
    assert (CK.IN_BYTES, CK.OUT_BYTES, CK.RUN_BYTES, CK.COUNTS_BYTES) == (8, 10, 12, 16)
    assert sum(np.dtype(t).itemsize for t in dense) == CK.OUT_BYTES and 2 * 4 == CK.IN_BYTES and 3 * 4 == CK.RUN_BYTES
    lib = load_hip()
    allg = np.arange(G, dtype=np.int32)
    mem = np.tile(np.array([100, 101, 102], np.int32), (G, 1))
    e = Engine(lib, 100, G, kmax=K, window=Wn, max_batch=G + 1024)
    assert (e.create_groups(allg, mem, K, hri_create(G, K, 100)) == S_OK).all()
    dev = torch.device("cuda:0")
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(ts)
    e.set_stream(ts.cuda_stream)

    # device columns of the _dev legs
    t_g = torch.arange(G, dtype=torch.int32, device=dev)
    t_cp = torch.zeros(G, dtype=torch.int32, device=dev)
    t_dense = [torch.zeros(G * np.dtype(t).itemsize, dtype=torch.uint8, device=dev) for t in dense]
    t_runs = [torch.zeros(G, dtype=torch.int32, device=dev) for _ in range(3)]
    t_cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    t_zero = torch.zeros(G, dtype=torch.int32, device=dev)
    t_bc = torch.full((G,), 100, dtype=torch.int32, device=dev)
    t_med = torch.full((G,), -1, dtype=torch.int32, device=dev)      # the groups' accepted-GC slot: collects nothing
    t_kind = torch.full((G,), C_HASVALUE, dtype=torch.uint8, device=dev)
    t_status = torch.zeros(G, dtype=torch.uint8, device=dev)
    t_nr = torch.zeros(1, dtype=torch.int32, device=dev)
    t_slots = [torch.zeros(G, dtype=torch.int32, device=dev) for _ in range(COMMIT_UP_TO)]
    # pageable columns of the host twin
    h_cp = np.zeros(G, np.int32)
    h_dense = [np.zeros(G, t) for t in dense]
    h_runs = [np.zeros(G, np.int32) for _ in range(3)]
    h_cnt = CK.CpCounts()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    cur = [1]                                      # the slot every group is at

    def leg_cp_dev(d):
        t_cp.fill_(cur[0] + d - 1)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(ts)
        CK.checkpoint_batch_dev(e, G, t_g.data_ptr(), t_cp.data_ptr(), 0, [t.data_ptr() for t in t_dense],
                                [t.data_ptr() for t in t_runs], t_cnt.data_ptr())
        ev[1].record(ts)
        torch.cuda.synchronize()
        cur[0] += d
        assert t_cnt.cpu().tolist() == [G, 0, 0, 0]
        assert bool((t_dense[1].view(torch.int32) == cur[0]).all())
        return ev[0].elapsed_time(ev[1]) * 1e-3

    def leg_cp_host(d):
        h_cp[:] = cur[0] + d - 1
        t0 = time.perf_counter()
        rc = lib.fn["checkpoint_batch"](e.h, G, vp(allg), vp(h_cp), 0, *[vp(x) for x in h_dense], *[vp(x) for x in h_runs],
                                        C.byref(h_cnt))
        dt = time.perf_counter() - t0
        cur[0] += d
        assert rc == 0 and (h_cnt.n_adopted, h_cnt.n_nogroup, h_cnt.n_stopped, h_cnt.n_runs) == (G, 0, 0, 0)
        assert (h_dense[1] == cur[0]).all() and (h_dense[3] == S_OK).all()
        return dt

    def leg_commit(d):
        for j in range(d):
            t_slots[j].fill_(cur[0] + j)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(ts)
        for j in range(d):
            e.call_dev("commit_batch", G, t_g.data_ptr(), t_zero.data_ptr(), t_bc.data_ptr(), t_slots[j].data_ptr(),
                       t_med.data_ptr(), t_kind.data_ptr(), t_status.data_ptr(), *[t.data_ptr() for t in t_runs],
                       t_nr.data_ptr())
        ev[1].record(ts)
        torch.cuda.synchronize()
        cur[0] += d
        assert int(t_nr.cpu()[0]) == G and not bool(t_status.any())
        return ev[0].elapsed_time(ev[1]) * 1e-3

    out = {"config": {"groups": G, "k": K, "window": Wn, "reps_per_leg": R},
           "bytes_over_the_link_host_twin": {"in_per_record": CK.IN_BYTES, "out_per_record": CK.OUT_BYTES,
                                             "per_run": CK.RUN_BYTES, "counts": CK.COUNTS_BYTES,
                                             "per_call": G * (CK.IN_BYTES + CK.OUT_BYTES) + CK.COUNTS_BYTES},
           "cells": {}}
    for d in DISTANCES:
        legs = {"cp_dev": leg_cp_dev, "cp_host": leg_cp_host}
        if d <= COMMIT_UP_TO:
            legs["commit"] = leg_commit
        times = {k: [] for k in legs}
        names = list(legs)
        for rep in range(R + 1):                                     # the first repetition warms every leg
            for k in names[rep % len(names):] + names[:rep % len(names)]:
                dt = legs[k](d)
                if rep:
                    times[k].append(dt)
        cell = {k: stats(v) for k, v in times.items()}
        if "commit" in cell:
            cell["cp_dev_over_commit"] = round(cell["cp_dev"]["median_ms"] / cell["commit"]["median_ms"], 3)
        else:
            cell["commit"] = "cannot be run"
        out["cells"][f"d_{d}"] = cell
    snap, st = e.snapshot(allg[:: max(G // 1000, 1)])
    assert (st == S_OK).all() and (snap["acc_slot"] == cur[0]).all() and (snap["acc_gc_slot"] == -1).all()
    e.profile(2)
    for d in (1, 100_000):
        leg_cp_dev(d)
    prof = e.profile_read()
    e.profile(0)
    out["dev_kernels_ms"] = {k: round(v[1] / v[0], 5) for k, v in sorted(prof.items()) if k.startswith("k_cp_")}
    e.close()
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
