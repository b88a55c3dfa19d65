#!/usr/bin/env python
"""The log index on the device (include/gpx_logindex.h) against what a host does today and against the bytes its scans
read (a side figure, not the judged bench line).

Workload: --groups groups (default 1 M) and a table of --rows rows (default 10 M, then 100 M), fed in batches of --batch
records (default 1 M: one accept call's worth).  Record i names a uniformly random group and slot i // groups + 1, so a
group's slots ascend and a group holds rows / groups entries.  Per table size, in one process:
  add       the fill, gpx_logindex_add_dev per batch between two device events; the last batches through the host twin
            (pageable memory, wall time) - and every batch through the host loop
  files     gpx_logindex_files[_dev] over 4,096 ids
  lookup    one batch of distinct groups, each asking for the upper quarter of its slots; cap = all hits; then the same
            call with 1 .. all of the batch's records against the host loop over those records: a call scans the whole
            table however few records it has, the host loop touches only the groups named - where the two cross
  set_gc    one batch of distinct groups, 2 * reps calls with ascending GC slots (a call changes what the next one sees:
            even calls take the _dev form, odd ones the host twin, the host loop takes all of them)
  scans     the row scans alone, from the engine's profile in a pass of their own: the lookup scan with every group armed
            and with one armed (what the arming-word gather costs beyond the columns: the gather is taken either way, an
            armed group also has its range read and its hits parked), the file_rows scan, which reads no arming word,
            and the files histogram - each beside a device memcpy of the bytes of the columns it reads
  baseline  scripts/logindex_host_loop.cpp: LogIndex.java restated over per-group vectors, one thread, wall time
The three sides' counts are checked against each other."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
VP = C.c_void_p


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2] * 1e3, 4), "min_ms": round(xs[0] * 1e3, 4), "max_ms": round(xs[-1] * 1e3, 4),
            "n": len(xs)}


def host_loop_lib():
    d = tempfile.mkdtemp(prefix="gpx_logindex_bench_")
    so = os.path.join(d, "logindex_host_loop.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "scripts", "logindex_host_loop.cpp")])
    lib = C.CDLL(so)
    lib.li_new.restype = VP
    lib.li_new.argtypes = [C.c_int32]
    lib.li_free.argtypes = [VP]
    for name, args in (("li_add", [VP, C.c_int32] + [VP] * 6 + [C.c_int32]), ("li_set_gc", [VP, C.c_int32, VP, VP]),
                       ("li_lookup", [VP, C.c_int32] + [VP] * 4 + [C.c_longlong, VP, VP, VP]),
                       ("li_files", [VP, C.c_int32, C.c_int32, VP, VP, VP]), ("li_rows", [VP])):
        f = getattr(lib, name)
        f.restype, f.argtypes = C.c_longlong, args
    return lib


def batch_columns(rng, start, n, groups):
    """records start .. start + n of the workload"""
    i = start + np.arange(n, dtype=np.int64)
    return dict(gidx=rng.integers(0, groups, n, dtype=np.int32), slot=(i // groups + 1).astype(np.int32),
                bnum=np.zeros(n, np.int32), bcoord=np.full(n, 100, np.int32), off=i * 167, len=np.full(n, 163, np.int32))


def wall(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def run_size(a, rows, loop, memcpy):
    import torch
    from gigapaxos_amd import Engine, load_hip
    from gigapaxos_amd import logindex as L

    G, B = a.groups, a.batch
    dev = torch.device("cuda:0")
    e = Engine(load_hip(), 101, G, kmax=3, window=8, max_batch=B)
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(ts)
    e.set_stream(ts.cuda_stream)
    L.open(e, rows)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    P = lambda t: t.data_ptr()                                         # noqa: E731
    d_cnt = torch.zeros(32, dtype=torch.uint8, device=dev)
    d_status = torch.zeros(B, dtype=torch.uint8, device=dev)

    def counts():
        return L.LogIndexCounts.from_buffer_copy(d_cnt.cpu().numpy().tobytes())

    def timed(f):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(ts)
        f()
        ev[1].record(ts)
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e-3

    H = loop.li_new(G)
    rng = np.random.default_rng(27)
    ptr = lambda x: x.ctypes.data                                      # noqa: E731
    t = {k: [] for k in ("add_dev", "add_host", "add_baseline")}
    nb = (rows + B - 1) // B
    for b in range(nb):
        n = min(B, rows - b * B)
        c = batch_columns(rng, b * B, n, G)
        file = b * 64 // nb                                            # 64 files
        order = ("gidx", "slot", "bnum", "bcoord", "off", "len")
        if b >= nb - a.reps and nb > a.reps:                           # the last batches: the host twin
            dt, (st, hc) = wall(lambda: L.add(e, *[c[k] for k in order], file))
            assert hc.n_done == n
            t["add_host"].append(dt)
        else:
            d = [up(c[k]) for k in order]
            torch.cuda.synchronize()
            dt = timed(lambda: L.add_dev(e, n, 0, [P(x) for x in d], file, P(d_status), P(d_cnt)))
            assert counts().n_done == n
            if b:                                                      # the first call warms
                t["add_dev"].append(dt)
        dt, added = wall(lambda: loop.li_add(H, n, *[ptr(c[k]) for k in order], file))
        assert added == n
        t["add_baseline"].append(dt)
    res = {"rows": rows, "groups": G, "batch": B, "add": {k: stats(v) for k, v in t.items() if v}}
    assert loop.li_rows(H) == rows

    # ---- files ----
    NF = 4096
    d_fr, d_fg = torch.zeros(NF, dtype=torch.int32, device=dev), torch.zeros(NF, dtype=torch.int32, device=dev)
    d_fm = torch.zeros(1, dtype=torch.int32, device=dev)
    b_fr, b_fg, b_fm = np.zeros(NF, np.int32), np.zeros(NF, np.int32), np.zeros(1, np.int32)
    t = {k: [] for k in ("dev", "host", "baseline")}
    for rep in range(a.reps + 1):
        dt = timed(lambda: L.files_dev(e, 0, NF, P(d_fr), P(d_fg), P(d_fm), P(d_cnt)))
        th, (h_rows, h_groups, h_lo, _) = wall(lambda: L.files(e, 0, NF))
        tb, _ = wall(lambda: loop.li_files(H, 0, NF, ptr(b_fr), ptr(b_fg), ptr(b_fm)))
        if rep == 0:
            assert (d_fr.cpu().numpy() == b_fr).all() and (d_fg.cpu().numpy() == b_fg).all() and int(d_fm.item()) == b_fm[0] == h_lo
            assert (h_rows == b_fr).all() and (h_groups == b_fg).all() and b_fr.sum() == rows
        else:
            t["dev"].append(dt), t["host"].append(th), t["baseline"].append(tb)
    res["files"] = {k: stats(v) for k, v in t.items()}

    # ---- lookup: a batch of distinct groups, the upper quarter of each group's slots ----
    per = max(rows // G, 1)
    qg = rng.permutation(G)[:min(B, G)].astype(np.int32)
    nq = qg.shape[0]
    lo = np.full(nq, per - per // 4 + 1, np.int32)
    cap = rows
    d_q, d_lo = up(qg), up(lo)
    outs = [torch.zeros(cap, dtype=torch.int64 if k == "off" else torch.int32, device=dev) for k, _ in L.LOOKUP_COLS]
    b_off, b_len, s = np.zeros(cap, np.int64), np.zeros(cap, np.int32), C.c_ulonglong(0)
    t = {k: [] for k in ("dev", "host", "baseline")}
    for rep in range(a.reps + 1):
        dt = timed(lambda: L.lookup_dev(e, nq, P(d_q), P(d_lo), 0, 0, cap, [P(x) for x in outs], P(d_status), P(d_cnt)))
        hits = counts().n_hits
        th, (ho, _, hc) = wall(lambda: L.lookup(e, qg, lo, cap=hits))
        tb, bh = wall(lambda: loop.li_lookup(H, nq, ptr(qg), ptr(lo), None, None, cap, ptr(b_off), ptr(b_len), C.byref(s)))
        if rep == 0:
            assert hits == bh == hc.n_hits == hc.n_done and hits > 0
            assert np.array_equal(np.sort(outs[6][:hits].cpu().numpy()), np.sort(b_off[:hits])) and np.array_equal(ho["off"], outs[6][:hits].cpu().numpy())
        else:
            t["dev"].append(dt), t["host"].append(th), t["baseline"].append(tb)
    res["lookup"] = dict({k: stats(v) for k, v in t.items()}, records=int(nq), hits=int(hits))

    # ---- where the batch gets too small: a call scans the whole table however few records it has ----
    sweep = []
    for k in (1, 16, 256, 4096, 65536, nq):
        td, tb = [], []
        for rep in range(a.reps + 1):
            td.append(timed(lambda: L.lookup_dev(e, k, P(d_q), P(d_lo), 0, 0, cap, [P(x) for x in outs], P(d_status), P(d_cnt))))
            kh = counts().n_hits
            dt, bh = wall(lambda: loop.li_lookup(H, k, ptr(qg), ptr(lo), None, None, cap, ptr(b_off), ptr(b_len), C.byref(s)))
            tb.append(dt)
            assert kh == bh
        sweep.append({"records": int(k), "hits": int(kh), "dev_ms": stats(td[1:])["median_ms"], "baseline_ms": stats(tb[1:])["median_ms"]})
    res["lookup_by_batch"] = sweep

    # ---- the scans alone, and the bytes they read ----
    one = up(np.array([0], np.int32))
    e.profile(2)
    for _ in range(a.reps):
        L.lookup_dev(e, nq, P(d_q), P(d_lo), 0, 0, 0, [0] * 8, 0, P(d_cnt))
    e.sync()
    armed = {k: v[1] / v[0] for k, v in e.profile_read().items()}
    e.profile(0), e.profile(2)
    for _ in range(a.reps):
        L.lookup_dev(e, 1, P(one), P(d_lo), 0, 0, 0, [0] * 8, 0, P(d_cnt))
        L.file_rows_dev(e, 5, 0, [0] * 8, P(d_cnt))
        L.files_dev(e, 0, NF, P(d_fr), P(d_fg), P(d_fm), P(d_cnt))
    e.sync()
    plain = {k: v[1] / v[0] for k, v in e.profile_read().items()}
    e.profile(0)
    src, dst = torch.zeros(rows * 9 + 16, dtype=torch.uint8, device=dev), torch.zeros(rows * 9 + 16, dtype=torch.uint8, device=dev)

    def copy_ms(nbytes):
        xs = []
        for rep in range(a.reps + 1):
            def f():
                if memcpy:
                    assert memcpy(P(dst), P(src), nbytes, 3, ts.cuda_stream) == 0
                else:
                    dst[:nbytes].copy_(src[:nbytes])
            xs.append(timed(f))
        return round(sorted(xs[1:])[len(xs[1:]) // 2] * 1e3, 4)
    res["scans"] = {
        "memcpy": "hipMemcpyAsync" if memcpy else "torch copy_",
        "lookup_scan_all_armed_ms": round(armed["k_li_scan_lookup"], 4), "lookup_scan_one_armed_ms": round(plain["k_li_scan_lookup"], 4),
        "lookup_scan_bytes": rows * 9, "memcpy_9B_per_row_ms": copy_ms(rows * 9),
        "file_rows_scan_ms": round(plain["k_li_scan_file"], 4), "files_rows_hist_ms": round(plain["k_li_files_rows"], 4),
        "files_groups_hist_ms": round(plain["k_li_files_groups"], 4), "file_scan_bytes": rows * 5, "memcpy_5B_per_row_ms": copy_ms(rows * 5),
        "kernels_ms": {k: round(v, 4) for k, v in sorted({**plain, **armed}.items()) if k.startswith("k_li_")}}
    del src, dst, outs

    # ---- set_gc: ascending GC slots over one batch of distinct groups ----
    t = {k: [] for k in ("dev", "host", "baseline")}
    steps = 2 * a.reps + 2
    d_gc = torch.zeros(nq, dtype=torch.int32, device=dev)
    alive = rows
    for r in range(steps):
        gc = np.full(nq, r + 1 if per < 2 * steps else per * (r + 1) // (2 * steps), np.int32)   # half the slots in the end
        tb, died = wall(lambda: loop.li_set_gc(H, nq, ptr(qg), ptr(gc)))
        if r % 2 == 0:
            d_gc.copy_(up(gc))
            torch.cuda.synchronize()
            dt = timed(lambda: L.set_gc_dev(e, nq, P(d_q), P(d_gc), 0, P(d_status), P(d_cnt)))
            c = counts()
        else:
            dt, (_, c) = wall(lambda: L.set_gc(e, qg, gc))
        alive -= died
        assert (c.n_stale, c.n_alive, c.n_done) == (died, alive, nq), (r, c.n_stale, died)
        if r >= 2:                                                     # the first call of each form warms
            t["dev" if r % 2 == 0 else "host"].append(dt), t["baseline"].append(tb)
    res["set_gc"] = dict({k: stats(v) for k, v in t.items()}, records=int(nq), rows_alive_after=int(alive))

    # ---- compact, once ----
    dt = timed(lambda: L.compact_dev(e, P(d_cnt)))
    c = counts()
    assert c.n_rows == alive == loop.li_rows(H)
    res["compact"] = {"dev_ms": round(dt * 1e3, 4), "rows_moved": int(alive), "bytes_moved": int(alive) * 37}
    for k in ("add", "files", "lookup", "set_gc"):
        leg = res[k]
        d = leg.get("dev", leg.get("add_dev"))
        bl = leg.get("baseline", leg.get("add_baseline"))
        h = leg.get("host", leg.get("add_host"))
        leg["baseline_over_dev"] = round(bl["median_ms"] / d["median_ms"], 1)
        if h:
            leg["baseline_over_host"] = round(bl["median_ms"] / h["median_ms"], 2)
    sc = res["scans"]
    sc["lookup_scan_over_memcpy"] = round(sc["lookup_scan_all_armed_ms"] / sc["memcpy_9B_per_row_ms"], 2)
    sc["file_scan_over_memcpy"] = round(sc["file_rows_scan_ms"] / sc["memcpy_5B_per_row_ms"], 2)
    sc["armed_over_one_armed"] = round(sc["lookup_scan_all_armed_ms"] / sc["lookup_scan_one_armed_ms"], 2)
    sc["lookup_scan_over_file_scan"] = round(sc["lookup_scan_one_armed_ms"] / sc["file_rows_scan_ms"], 2)
    loop.li_free(H)
    e.close()
    torch.cuda.empty_cache()
    return res


def main():
    from bench_journal_pack import hip_memcpy
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, nargs="+", default=[10_000_000, 100_000_000])
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    a = ap.parse_args()
    assert a.reps >= 3
    loop = host_loop_lib()
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()
    memcpy = hip_memcpy()
    res = {"command": "scripts/bench_logindex.py " + " ".join(sys.argv[1:]), "reps": a.reps, "sizes": []}
    for rows in a.rows:
        res["sizes"].append(run_size(a, rows, loop, memcpy))
        print(json.dumps(res["sizes"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
