#!/usr/bin/env python
"""Delta images (include/gpx_delta.h): what a snapshot costs when only a part of the table changed (a side figure, not
the judged bench line).

One engine, 1 M groups x 3 replicas, window 8, and a second one as the mirror.  Between two calls accept-reply traffic
(whole rounds: propose, a majority of accept replies, the commit) touches none, 1 in 1,000, 1 in 10 or all of the groups.
  delta_dev    gpx_group_export_delta_dev of the whole table into device buffers, between device events
  full_dev     the yardstick, the way to the same snapshot without marks: gpx_group_export_dev of the whole table, in the
               same process, between device events
  delta_host / full_host
               the host-pointer twins, pageable memory, wall clock
  mirror       image.mirror_groups (count, export, apply on the second engine), wall clock
Every timed delta call sees the same changed set: after the traffic the legs run dev, host, mirror, and between them the
marks of the touched groups are taken back by another round of traffic.  Repetitions are interleaved, medians of seven
with min and max.  The script asserts what crosses the link from the layouts: the stride per row written, 4 bytes per gone
group, 32 bytes of counts.  No time is fixed in advance; two expectations follow from the bytes moved and are reported
as met or missed with the numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DENSITIES = {"none": 0, "1 in 1000": 1000, "1 in 10": 10, "all": 1}


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
    gone_d = torch.zeros(G, dtype=torch.int32, device=dev)
    cnt_d = torch.zeros(8, dtype=torch.int32, device=dev)
    rows_h, gone_h = np.zeros(G * stride, np.uint8), np.zeros(G, np.int32)

    def traffic(g):
        if not g.size:
            return
        sl, bn, bc, med, st = ea.propose(g)
        assert (st == S_OK).all()
        for acc in (100, 101):
            ea.accept_reply(g, bn, bc, sl, np.full(g.size, acc, np.int32), np.zeros(g.size, np.int32))
        st, _ = ea.commit(g, bn, bc, sl, med, np.full(g.size, C_HASVALUE, np.uint8))
        assert (st == S_OK).all()

    def timed_dev(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(ts)
        fn()
        ev[1].record(ts)
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e-3

    c, st, _ = image.mirror_groups(ea, eb, full=True)                 # the baseline: marks on A, the mirror filled
    assert c.n_done == G and (st == S_OK).all()
    legs = ("delta_dev", "full_dev", "delta_host", "full_host", "mirror")
    times = {d: {k: [] for k in legs} for d in DENSITIES}
    link = {}
    for rep in range(R + 1):                                          # the first repetition warms every leg
        for dname, every in DENSITIES.items():
            g = allg[::every] if every else allg[:0]
            t = {}
            traffic(g)
            t["delta_dev"] = timed_dev(lambda: image.export_delta_dev(ea, G, 0, 0, G, rows_d.data_ptr(), G, gone_d.data_ptr(),
                                                                      cnt_d.data_ptr()))
            got = cnt_d.cpu().tolist()
            assert got == [G, g.size, g.size, g.size, g.size, 0, 0, 0], (dname, got)
            t["full_dev"] = timed_dev(lambda: image.export_groups_dev(ea, G, 0, 0, G, rows_d.data_ptr(), cnt_d.data_ptr()))
            assert cnt_d.cpu().tolist()[:4] == [G, G, G, G]
            traffic(g)
            t0 = time.perf_counter()
            rows, gone, c = image.export_delta(ea, None, 0, cap=G, cap_gone=G, out=rows_h, out_gone=gone_h)
            t["delta_host"] = time.perf_counter() - t0
            assert c.as_tuple() == (G, g.size, g.size, g.size, g.size, 0, 0, 0)
            # what crosses the link, from the layouts: rows written, gone groups, counts
            link[dname] = {"delta_bytes": g.size * stride + 0 * 4 + image.DELTA_COUNTS_BYTES,
                           "full_bytes": G * stride + image.COUNTS_BYTES}
            assert rows.nbytes == g.size * stride and gone.nbytes == 0
            t0 = time.perf_counter()
            rows, c = image.export_groups(ea, None, 0, cap=G, out=rows_h)
            t["full_host"] = time.perf_counter() - t0
            assert rows.nbytes == G * stride
            traffic(g)
            t0 = time.perf_counter()
            c, st, _ = image.mirror_groups(ea, eb)
            t["mirror"] = time.perf_counter() - t0
            assert c.n_done == g.size and (st == S_OK).all()
            if rep:
                for k, v in t.items():
                    times[dname][k].append(v)
    ea.profile(2)
    image.export_delta_dev(ea, G, 0, image.DELTA_FULL, G, rows_d.data_ptr(), G, gone_d.data_ptr(), cnt_d.data_ptr())
    image.export_groups_dev(ea, G, 0, 0, G, rows_d.data_ptr(), cnt_d.data_ptr())
    torch.cuda.synchronize()
    prof = {k: round(v[1], 5) for k, v in sorted(ea.profile_read().items()) if k.startswith(("k_image_", "k_delta_"))}
    out = {"config": {"groups": G, "k": K, "window": Wn, "reps_per_leg": R, "stride": stride},
           "densities": {d: {k: stats(v) for k, v in times[d].items()} for d in DENSITIES},
           "link_bytes": link, "kernels_ms_full_table": prof, "expectations": {}}
    for d in DENSITIES:
        leg = out["densities"][d]
        leg["delta_dev_over_full_dev"] = round(leg["delta_dev"]["median_ms"] / leg["full_dev"]["median_ms"], 3)
        leg["delta_host_over_full_host"] = round(leg["delta_host"]["median_ms"] / leg["full_host"]["median_ms"], 3)
    for d in ("none", "1 in 1000"):
        r = out["densities"][d]["delta_dev_over_full_dev"]
        out["expectations"][f"{d}: the delta call takes less than the full export"] = {"ratio": r, "met": r < 1.0}
    r = out["densities"]["all"]["delta_dev_over_full_dev"]
    out["expectations"]["all: the full export plus one more read of the state"] = {"ratio": r, "met": 1.0 <= r <= 2.0}
    for e in (ea, eb):
        e.close()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
