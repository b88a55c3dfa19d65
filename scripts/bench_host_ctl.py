"""Per-call time of the control-plane host-pointer calls (profiles/r14_host_ctl_stage.txt, section 5): every twin on one
engine at n = 1,000 and then on another at n = 100,000.  Prints one JSON line: per size and twin the median of the whole
Python binding ("name") and the median of the library call alone, taken around the ctypes call with the first call left
out ("lib:name").  The library is the built one, or GPX_HIP_LIB's: run it in alternating processes to compare two builds.
    python scripts/bench_host_ctl.py"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gigapaxos_amd import Engine, hri_create, load_hip, scan, sweep, RETIRE_PAUSE
from gigapaxos_amd import wire as W

ME = 100
CUR = [None]   # the dict the wrapped library calls of the current run() append to
def i32(n, v=0): return np.full(n, v, np.int32)

def run(n, reps):
    lib = load_hip()
    G = n + 8
    e = Engine(lib, ME, G, kmax=3, window=8, max_batch=1 << 18, flags=1)
    we = W.WireEngine(e)
    g = np.arange(n, dtype=np.int32)
    raw = {}
    CUR[0] = raw
    def wrap(fn):
        for name, f in list(fn.items()):
            if getattr(f, "_wrapped", False): continue
            def mk(name, f):
                def w(*a):
                    t0 = time.perf_counter(); r = f(*a); CUR[0].setdefault(name, []).append(time.perf_counter() - t0); return r
                w._wrapped = True
                return w
            fn[name] = mk(name, f)
    wrap(e.lib.fn); wrap(we.lib.fn)
    mem = np.zeros((n, 3), np.int32); mem[:] = (ME, ME + 1, ME + 2)
    rows = hri_create(n, 3, ME)
    names = [b"svc-%d" % i for i in range(n)]
    res = {}
    def t(label, fn, reps=reps):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        res[label] = round(float(np.median(ts)) * 1e6, 1)
    t("group_create", lambda: e.create_groups(g, mem, 3, rows))
    t("names_bind", lambda: we.bind(names, g))
    t("names_lookup", lambda: we.lookup(names))
    t("names_coordinator", lambda: W.names_coordinator(we, g, 1))
    t("election_scan", lambda: W.election_scan(we, g, (ME,), (), False))
    t("gap_scan", lambda: W.gap_scan(we, g, 1))
    t("poke_scan", lambda: e.poke_scan(g))
    t("election_scan_hits", lambda: scan.election_scan_hits(e, g, (ME,), (), True))
    t("poke_scan_hits", lambda: scan.poke_scan_hits(e, g))
    t("gap_scan_hits", lambda: scan.gap_scan_hits(e, g, 1, require=0))
    t("pause_sweep", lambda: sweep.pause_sweep(e, g, 0, sweep.SWEEP_PEEK))
    t("group_snapshot", lambda: e.snapshot(g))
    sl, bn, bc, md, st = e.propose(g)
    d = e.accept_reply(np.concatenate([g, g]), i32(2 * n), i32(2 * n, ME), np.concatenate([sl, sl]),
                       np.concatenate([i32(n, ME), i32(n, ME + 1)]), i32(2 * n))
    t("wire_pack_commits", lambda: we.pack_commits(d))
    frames, _, _ = we.pack_commits(d)
    buf_off = W.concat_frames(frames)
    t("wire_decode", lambda: we.decode(None, buf_off=buf_off))
    (rb, rc, rm, rf, ast), _ = e.accept(g, i32(n), i32(n, ME), sl, i32(n))
    t("wire_pack_accept_replies", lambda: we.pack_accept_replies(g, sl, rb, rc, rm, ast, i32(n, ME), np.arange(n, dtype=np.int64)))
    t("prepare_batch", lambda: e.prepare(g, i32(n, 1), i32(n, ME + 1), i32(n)))
    est = (g * 37 % 900).astype(np.int32)
    t("request_batch", lambda: W.request_batch(we, g, est, None, None, max_bytes=4096, max_size=16))
    t("election_begin", lambda: e.election_begin(g, i32(n, 2)))
    t("prepare_reply_batch", lambda: e.prepare_reply(g, i32(n, ME + 1), i32(n, 2), i32(n, ME), i32(n), None), reps=max(reps // 4, 2))
    t("names_unbind", lambda: we.unbind(g))
    t("group_retire", lambda: e.retire_groups(g, RETIRE_PAUSE))
    e.close()
    for k, v in raw.items():
        if len(v) >= 3: res["lib:" + k] = round(float(np.median(v[1:])) * 1e6, 1)   # without the first call
    return res

out = {"n=1000": run(1000, 200), "n=100000": run(100000, 24)}
print(json.dumps(out))
