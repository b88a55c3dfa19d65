#!/usr/bin/env python
"""The deactivation sweep (include/gpx_sweep.h) against the call it replaces (a side figure, not the judged bench line).

One engine, 1 M groups x 3 replicas, window 8.  At four hit densities - none, 1 in 1,000, 1 in 10 and all - two legs
pause THE SAME groups, their repetitions interleaved in one process (median and spread of seven, as
scripts/bench_scan_hits.py reports them):
  sweep   gpx_pause_sweep over the whole table at min_age 1, pageable outputs: finds the idle groups itself
  retire  the parent's way, gpx_group_retire(GPX_RETIRE_PAUSE) on the list of exactly those groups - given its list for
          free: what a host pays to keep that list (a lastActive per group, updated for every record) is not in it
Before every timed call the groups of the cell's hit class are idle since the last tick and every other group has just
received an ACCEPT (untimed), and after it the paused groups are re-created from the rows the call returned (untimed).
The bytes that cross the link follow from the layouts and are asserted: 105 per paused group plus 16 for the sweep, 104
per listed group for the retire call.  For the zero-hit table the _dev form is also timed between device events, with
the bytes of the covered columns it reads per second beside a streaming read (a torch sum) of as many bytes in the same
run."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DENSITIES = (("none", 0), ("1_in_1000", 1000), ("1_in_10", 10), ("all", 1))
RETIRE_BYTES = 4 + 100 + 0      # gidx in, the row out (no status column is asked for)


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
    from gigapaxos_amd import Engine, hri_create, load_hip, make_hri, S_OK, HRI_DTYPE
    from gigapaxos_amd import sweep

    G, K, Wn, R = a.groups, 3, 8, a.reps
    assert sweep.HIT_BYTES == 105 and sweep.COUNTS_BYTES == 16 and HRI_DTYPE.itemsize == 100
    lib = load_hip()
    allg = np.arange(G, dtype=np.int32)
    mem = np.tile(np.array([100, 101, 102], np.int32), (G, 1))
    e = Engine(lib, 100, G, kmax=K, window=Wn, max_batch=G + 1024)
    assert (e.create_groups(allg, mem, K, hri_create(G, K, 100)) == S_OK).all()
    dev = torch.device("cuda:0")
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(ts)
    e.set_stream(ts.cuda_stream)
    outs = [np.zeros(G, dt) for _, dt in sweep.SWEEP_COLS]
    r_rows = make_hri(G)
    ballot = [0]

    def traffic(g):
        """an ACCEPT at a ballot number not used before for every group of g: its state changes, it stays caught up"""
        if g.size:
            ballot[0] += 1
            z = np.zeros(g.size, np.int32)
            out, _ = e.accept(g, np.full(g.size, ballot[0], np.int32), np.full(g.size, 100, np.int32), z + 1, z)
            assert (out[4] == S_OK).all()

    def tick():
        _, c = sweep.pause_sweep(e, None, min_age=255, cap=0)
        return c

    def restore(g, rows):
        if g.size:
            assert (e.create_groups(g, mem[: g.size], K, rows) == S_OK).all()

    out = {"config": {"groups": G, "k": K, "window": Wn, "reps_per_leg": R}, "cells": {}}
    tick()
    for name, every in DENSITIES:
        hits = np.ascontiguousarray(allg[::every] if every else allg[:0])
        others = np.setdiff1d(allg, hits).astype(np.int32)
        times = {"sweep": [], "retire": []}
        for rep in range(R + 1):                                     # the first repetition warms both legs
            for leg in (("sweep", "retire") if rep & 1 else ("retire", "sweep")):
                tick()                                               # re-created groups get their signature stored
                traffic(others)
                if leg == "sweep":
                    t0 = time.perf_counter()
                    (g, age, rows), c = sweep.pause_sweep(e, None, min_age=1, out=outs)
                    dt = time.perf_counter() - t0
                    assert (c.n_hits, c.n_nogroup, c.n_busy, c.n_paused) == (hits.size, 0, 0, hits.size)
                    assert g.shape[0] == hits.size and (g == hits).all()
                else:
                    t0 = time.perf_counter()
                    rc = lib.fn["group_retire"](e.h, hits.size, hits.ctypes.data_as(C.c_void_p), 0,
                                                r_rows.ctypes.data_as(C.c_void_p), None)
                    dt = time.perf_counter() - t0
                    assert rc == 0
                    rows = r_rows[: hits.size]
                restore(hits, rows)
                if rep:
                    times[leg].append(dt)
        cell = {"hits": int(hits.size),
                "bytes_over_the_link": {"sweep": int(hits.size) * sweep.HIT_BYTES + sweep.COUNTS_BYTES,
                                        "retire": int(hits.size) * RETIRE_BYTES}}
        for leg in times:
            cell[leg] = stats(times[leg])
        if hits.size:
            cell["sweep_over_retire"] = round(cell["sweep"]["median_ms"] / cell["retire"]["median_ms"], 3)
        out["cells"][name] = cell

    # ---- the table at rest: what one sweep reads, beside a streaming read of as many bytes ------------------------------
    covered = G * (4 * (10 + K) + 16 * Wn + 4 + 1)                   # state words, node_slots, acc_ring, signature, age
    for _ in range(2):
        tick()
    cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    blob = torch.ones(covered // 4, dtype=torch.int32, device=dev)
    t_sweep, t_read = [], []
    for rep in range(R + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record(ts)
        sweep.pause_sweep_dev(e, G, 0, 255, sweep.SWEEP_PEEK | sweep.SWEEP_HOLD, 0, [0, 0, 0], cnt.data_ptr())
        ev[1].record(ts)
        ev[2].record(ts)
        s = blob.sum()
        ev[3].record(ts)
        torch.cuda.synchronize()
        assert cnt.cpu().tolist() == [0, 0, 0, 0] and int(s) == covered // 4
        if rep:
            t_sweep.append(ev[0].elapsed_time(ev[1]) * 1e-3)
            t_read.append(ev[2].elapsed_time(ev[3]) * 1e-3)
    e.profile(2)
    for _ in range(R):
        sweep.pause_sweep_dev(e, G, 0, 255, sweep.SWEEP_PEEK | sweep.SWEEP_HOLD, 0, [0, 0, 0], cnt.data_ptr())
    e.sync()
    prof = e.profile_read()
    e.profile(0)
    at_rest = {"covered_bytes": covered, "dev_sweep": stats(t_sweep), "streaming_read": stats(t_read),
               "dev_kernels_ms": {k: round(v[1] / v[0], 5) for k, v in sorted(prof.items()) if k.startswith("k_sweep_")}}
    at_rest["sweep_GB_per_s"] = round(covered / (at_rest["dev_sweep"]["median_ms"] * 1e-3) / 1e9, 1)
    at_rest["streaming_read_GB_per_s"] = round(covered / (at_rest["streaming_read"]["median_ms"] * 1e-3) / 1e9, 1)
    out["table_at_rest"] = at_rest
    e.close()
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
