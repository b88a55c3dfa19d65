#!/usr/bin/env python
"""Group images (include/gpx_image.h): one timed leg per form (a side figure, not the judged bench line).

Two engines, 1 M groups x 3 replicas, window 8, every group caught up (the only state the yardstick can move):
  export_dev   gpx_group_export_dev of the whole table of engine A into a device buffer, between device events
  import_dev   gpx_group_import_dev of those rows into the empty engine B, between device events
  export_host / import_host
               the host-pointer twins, pageable memory, wall clock
  move         image.move_groups of every group from A to B (export with GPX_IMG_EVICT, the destination column made
               on the device, import), wall clock
  yardstick    gpx_group_snapshot of the same groups of A and gpx_group_create of them on B: host-pointer calls (they
               have no device form), wall clock, and the kernels alone from the engine's profile
Repetitions are interleaved in one process; between them B is emptied (gpx_group_retire KILL, untimed).  Beside the
device legs: the bytes they move (state words read or written plus rows written or read) over the HBM peak."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12        # bytes / s, the data sheet's


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2] * 1e3, 4), "min_ms": round(xs[0] * 1e3, 4), "max_ms": round(xs[-1] * 1e3, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()
    from gigapaxos_amd import Engine, hri_create, load_hip, S_OK, RETIRE_KILL
    from gigapaxos_amd import image

    G, K, Wn, R = a.groups, 3, 8, a.reps
    lib = load_hip()
    stride = image.image_stride(K, Wn)
    allg = np.arange(G, dtype=np.int32)
    mem = np.tile(np.array([100, 101, 102], np.int32), (G, 1))
    ea = Engine(lib, 100, G, kmax=K, window=Wn, max_batch=G + 1024)
    eb = Engine(lib, 100, G, kmax=K, window=Wn, max_batch=G + 1024)
    assert (ea.create_groups(allg, mem, K, hri_create(G, K, 100)) == S_OK).all()
    dev = torch.device("cuda:0")
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(ts)
    for e in (ea, eb):
        e.set_stream(ts.cuda_stream)
    rows_d = torch.zeros(G * stride, dtype=torch.uint8, device=dev)
    cnt_d = torch.zeros(4, dtype=torch.int32, device=dev)
    st_d = torch.zeros(G, dtype=torch.uint8, device=dev)
    rows_h = np.zeros(G * stride, np.uint8)
    times = {k: [] for k in ("export_dev", "import_dev", "export_host", "import_host", "move", "snapshot", "create")}

    def empty(e):
        e.retire_groups(allg, RETIRE_KILL)

    def timed_dev(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(ts)
        fn()
        ev[1].record(ts)
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e-3

    for rep in range(R + 1):                                         # the first repetition warms every leg
        t = {}
        t["export_dev"] = timed_dev(lambda: image.export_groups_dev(ea, G, 0, 0, G, rows_d.data_ptr(), cnt_d.data_ptr()))
        assert cnt_d.cpu().tolist() == [G, G, G, G]
        t["import_dev"] = timed_dev(lambda: image.import_groups_dev(eb, G, rows_d.data_ptr(), 0, 0, st_d.data_ptr()))
        assert int(st_d.max()) == S_OK
        empty(eb)
        t0 = time.perf_counter()
        rows, c = image.export_groups(ea, None, 0, cap=G, out=rows_h)
        t["export_host"] = time.perf_counter() - t0
        assert c.as_tuple() == (G, G, G, G)
        t0 = time.perf_counter()
        st = image.import_groups(eb, rows_h, None, 0)
        t["import_host"] = time.perf_counter() - t0
        assert (st == S_OK).all()
        empty(eb)
        t0 = time.perf_counter()
        hri, st = ea.snapshot(allg)
        t["snapshot"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        st = eb.create_groups(allg, mem, K, hri)
        t["create"] = time.perf_counter() - t0
        assert (st == S_OK).all()
        empty(eb)
        t0 = time.perf_counter()
        st = image.move_groups(ea, eb, allg, allg)
        t["move"] = time.perf_counter() - t0
        assert (st == S_OK).all()
        assert (image.move_groups(eb, ea, allg, allg) == S_OK).all()  # and back, untimed
        if rep:
            for k, v in t.items():
                times[k].append(v)
    # the kernels alone
    for e in (ea, eb):
        e.profile(2)
    image.export_groups_dev(ea, G, 0, 0, G, rows_d.data_ptr(), cnt_d.data_ptr())
    image.import_groups_dev(eb, G, rows_d.data_ptr(), 0, 0, st_d.data_ptr())
    torch.cuda.synchronize()
    empty(eb)
    hri, _ = ea.snapshot(allg)
    eb.create_groups(allg, mem, K, hri)
    prof = {}
    for e in (ea, eb):
        for k, v in e.profile_read().items():
            if k.startswith(("k_image_", "k_group_")):
                prof[k] = round(prof.get(k, 0.0) + v[1], 5)
        e.profile(0)
    state = G * 4 * (11 + 2 * K + Wn + 4 * Wn)                       # flags + 10 words, members, node_slots, p_ring, acc_ring
    moved = state + G * stride
    out = {"config": {"groups": G, "k": K, "window": Wn, "reps_per_leg": R, "stride": stride},
           "legs": {k: stats(v) for k, v in times.items()}, "kernels_ms": dict(sorted(prof.items())),
           "bytes_moved_per_device_leg": moved, "hbm_peak_ms": round(moved / HBM_PEAK * 1e3, 4)}
    leg = out["legs"]
    yard = leg["snapshot"]["median_ms"] + leg["create"]["median_ms"]
    out["yardstick_ms"] = round(yard, 4)
    out["ratios"] = {"export_dev_plus_import_dev_over_yardstick": round((leg["export_dev"]["median_ms"] + leg["import_dev"]["median_ms"]) / yard, 4),
                     "export_host_plus_import_host_over_yardstick": round((leg["export_host"]["median_ms"] + leg["import_host"]["median_ms"]) / yard, 4),
                     "move_over_yardstick": round(leg["move"]["median_ms"] / yard, 4),
                     "export_dev_over_hbm_peak": round(leg["export_dev"]["median_ms"] / out["hbm_peak_ms"], 2),
                     "import_dev_over_hbm_peak": round(leg["import_dev"]["median_ms"] / out["hbm_peak_ms"], 2)}
    for e in (ea, eb):
        e.close()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
