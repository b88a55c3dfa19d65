#!/usr/bin/env python
"""The retransmission sweep (include/gpx_timers.h) against what the parent offers (a side figure, not the judged bench
line).

One engine, 1 M groups x 3 replicas, window 8, every group with one outstanding slot: the whole table waits for accept
replies.  At four densities of DUE waits - none, 0.1 %, 1 % and all - three legs answer "which frames go out again now",
their repetitions interleaved in one process (median and spread of seven, as scripts/bench_pause_sweep.py reports them):
  dev       gpx_retransmit_sweep_dev over the whole table, outputs in device memory, between two device events
  host      gpx_retransmit_sweep, pageable outputs, wall time
  baseline  the parent's way: gpx_poke_scan_hits over the same table - every waiting group is a hit there - plus a numpy
            filter of its rows against stamps, counts and identities the HOST keeps per group (the bookkeeping the
            sweep takes over), wall time; the scan call's share of the leg is reported beside it
Before every timed call the table is brought to the same state, untimed: every wait re-armed at one instant, then all
but the cell's due class re-armed 1,001 ms later; the timed call comes 1,000 ms after that, so exactly the due class has
waited longer than the one threshold of 1,000 ms.  Every leg's answer is asserted to be that class.  The bytes that
cross the link follow from the layouts: 31 per due wait plus 16 for the sweep, 26 per WAITING group plus 16 for the
baseline.  For the zero-density table the tile kernels of both (k_rtx_tile, the parent's k_scan_poke_tile) are also
timed from the engine's profile and the two _dev calls between events, interleaved."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DENSITIES = (("none", 0), ("1_in_1000", 1000), ("1_in_100", 100), ("all", 1))
ROW_BYTES = 26                  # what gpx_poke_scan_hits returns per hit
THR = 1000


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
    from gigapaxos_amd import Engine, hri_create, load_hip, S_OK
    from gigapaxos_amd import scan, timers

    G, K, Wn, R = a.groups, 3, 8, a.reps
    assert timers.HIT_BYTES == 31 and timers.COUNTS_BYTES == 16
    lib = load_hip()
    allg = np.arange(G, dtype=np.int32)
    mem = np.tile(np.array([100, 101, 102], np.int32), (G, 1))
    e = Engine(lib, 100, G, kmax=K, window=Wn, max_batch=G + 1024)
    assert (e.create_groups(allg, mem, K, hri_create(G, K, 100)) == S_OK).all()
    assert (e.propose(allg)[4] == S_OK).all()                        # one outstanding slot everywhere
    dev = torch.device("cuda:0")
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(ts)
    e.set_stream(ts.cuda_stream)
    cfg = timers.make_cfg([THR])
    dts = [dt for _, dt in timers.RTX_COLS]
    d_out = [torch.zeros(G * dt.itemsize, dtype=torch.uint8, device=dev) for dt in dts]
    d_ptrs = [b.data_ptr() for b in d_out]
    d_cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    h_out = [np.zeros(G, dt) for dt in dts]
    s_out = [np.zeros(G, dt) for dt in dts[:8]]                      # the poke scan's eight columns
    # what a host keeps per group when the engine does not: the wait's identity, its stamp, its count
    h_id = np.zeros((G, 4), np.int32)
    h_since = np.zeros(G, np.int64)
    h_count = np.zeros(G, np.int32)
    clock, scan_s = [0], [0.0]

    def dev_sweep(n, gidx_t, now, cap):
        timers.retransmit_sweep_dev(e, n, gidx_t.data_ptr() if gidx_t is not None else 0, now, cfg, 0, cap,
                                    d_ptrs if cap else [0] * 10, d_cnt.data_ptr())

    def prepare(others_t, n_others):
        """untimed: every wait stamped at one instant, all but the due class 1,001 ms later; -> the instant to ask at"""
        clock[0] += 5 * THR
        dev_sweep(G, None, clock[0], 0)                              # arms whatever is new (the first call only)
        clock[0] += 5 * THR
        dev_sweep(G, None, clock[0], G)                              # everything is due: all re-armed now
        t0 = clock[0]
        clock[0] += THR + 1
        if n_others:
            dev_sweep(n_others, others_t, clock[0], n_others)
        e.sync()
        t1 = clock[0]
        clock[0] += THR
        return t0, t1, clock[0]

    def baseline(now):
        """gpx_poke_scan_hits, then the filter and the bookkeeping on the host"""
        t = time.perf_counter()
        cols, c = scan.poke_scan_hits(e, None, out=s_out)
        scan_s[0] = time.perf_counter() - t
        g, pk, sl, bn, bc = cols[0], cols[1], cols[2], cols[3], cols[4]
        ident = np.stack([pk.astype(np.int32), sl, bn, bc], axis=1)
        new = (ident != h_id[g]).any(axis=1)
        waited = now - h_since[g]
        due = ~new & (waited > THR)
        h_id[g[new]] = ident[new]
        h_since[g[new]] = now
        h_count[g[new]] = 0
        dg = g[due]
        h_count[dg] = np.minimum(h_count[dg] + 1, 255)
        h_since[dg] = now
        return dg, c

    out = {"config": {"groups": G, "k": K, "window": Wn, "reps_per_leg": R, "threshold_ms": THR},
           "box": {"gpu": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__},
           "build": "hipcc --offload-arch=gfx950 -O3 -std=c++17 (gigapaxos_amd/csrc/libgpx_hip.so)", "cells": {}}
    for name, every in DENSITIES:
        due = np.ascontiguousarray(allg[::every] if every else allg[:0])
        others = np.setdiff1d(allg, due).astype(np.int32)
        others_t = torch.from_numpy(others).to(dev) if others.size else None
        times = {"dev": [], "host": [], "baseline": [], "baseline_scan_alone": []}
        for rep in range(R + 1):                                     # the first repetition warms every leg
            order = ("dev", "host", "baseline") if rep & 1 else ("baseline", "host", "dev")
            for leg in order:
                t0, t1, now = prepare(others_t, others.size)
                if leg == "dev":
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    ev[0].record(ts)
                    dev_sweep(G, None, now, G)
                    ev[1].record(ts)
                    torch.cuda.synchronize()
                    dt = ev[0].elapsed_time(ev[1]) * 1e-3
                    assert d_cnt.cpu().tolist() == [due.size, 0, G, due.size]
                    got = d_out[0].cpu().numpy().view(np.int32)[:due.size]
                elif leg == "host":
                    t = time.perf_counter()
                    cols, c = timers.retransmit_sweep(e, now, cfg, out=h_out)
                    dt = time.perf_counter() - t
                    assert (c.n_hits, c.n_nogroup, c.n_waiting, c.n_fired) == (due.size, 0, G, due.size)
                    got = cols[0]
                else:
                    h_since[:] = t0                                  # the host's stamps, brought to the same state
                    h_since[others] = t1
                    if rep == 0 and name == DENSITIES[0][0]:
                        baseline(t0)                                 # the host learns the identities once
                        h_since[:] = t0
                        h_since[others] = t1
                    t = time.perf_counter()
                    got, c = baseline(now)
                    dt = time.perf_counter() - t
                    assert (c.n_hits, c.n_nogroup) == (G, 0)
                assert got.shape[0] == due.size and (got == due).all(), (name, leg)
                if rep:
                    times[leg].append(dt)
                    if leg == "baseline":
                        times["baseline_scan_alone"].append(scan_s[0])      # the call's share of the leg
        cell = {"due": int(due.size), "waiting": G,
                "bytes_over_the_link": {"sweep": int(due.size) * timers.HIT_BYTES + timers.COUNTS_BYTES,
                                        "baseline": G * ROW_BYTES + 16}}
        for leg in times:
            cell[leg] = stats(times[leg])
        cell["host_over_baseline"] = round(cell["host"]["median_ms"] / cell["baseline"]["median_ms"], 4)
        out["cells"][name] = cell

    # ---- nothing due: the sweep's tile kernel beside the parent's, interleaved --------------------------------------------
    prepare(torch.from_numpy(allg).to(dev), G)
    now = clock[0] - THR                                              # nobody has waited at all
    s_cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    t_rtx, t_poke = [], []
    for rep in range(R + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        for leg in ((0, 1) if rep & 1 else (1, 0)):
            ev[2 * leg].record(ts)
            if leg == 0:
                dev_sweep(G, None, now, 0)
            else:
                scan.poke_scan_hits_dev(e, G, 0, 0, [0] * 8, s_cnt.data_ptr())
            ev[2 * leg + 1].record(ts)
        torch.cuda.synchronize()
        assert d_cnt.cpu().tolist() == [0, 0, G, 0] and s_cnt.cpu().tolist()[:2] == [G, 0]
        if rep:
            t_rtx.append(ev[0].elapsed_time(ev[1]) * 1e-3)
            t_poke.append(ev[2].elapsed_time(ev[3]) * 1e-3)
    e.profile(2)                                                      # per-kernel times in a pass of their own
    for rep in range(R):
        for leg in ((0, 1) if rep & 1 else (1, 0)):
            if leg == 0:
                dev_sweep(G, None, now, 0)
            else:
                scan.poke_scan_hits_dev(e, G, 0, 0, [0] * 8, s_cnt.data_ptr())
    e.sync()
    prof = e.profile_read()
    e.profile(0)
    out["nothing_due"] = {
        "retransmit_sweep_dev": stats(t_rtx), "poke_scan_hits_dev": stats(t_poke),
        "kernels_ms": {k: round(v[1] / v[0], 5) for k, v in sorted(prof.items())
                       if k.startswith("k_rtx_") or k.startswith("k_scan_")}}
    e.close()
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
