#!/usr/bin/env python
"""Packed 8-byte vote records (include/gpx_packed.h) against the column forms of gpx_accept_reply_batch_async, at
bench.py's end-to-end shape: one step = gpx_propose_batch_async(G) + the votes of G groups x K replicas from
gpx_host_alloc memory, three steps in flight (GPX_ASYNC_DEPTH=6), every round its own seeded round.

Three legs in ONE process, each on an engine of its own fed the same rounds, their bursts of `--burst` steps interleaved
(six-columns, common-ballot, packed, six-columns, ...), so that whatever else the host and the link are doing falls on all
three alike:
  six_columns    24 B per vote in
  common_ballot  16 B per vote in (bnum == bcoord == NULL) - bench.py's end-to-end leg, the yardstick
  packed          8 B per vote + 32 B per exception row in (gpx_accept_reply_packed_async)
Packing (gpx_votes_pack into gpx_host_alloc memory) happens outside the timed bursts and is reported as host
microseconds per call.  Also reported: the link's peaks from the same run (bench.link_peaks) and k_votes_unpack's time
between device events (gpx_votes_unpack_dev under gpx_profile_enable)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from collections import deque

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("six_columns", "common_ballot", "packed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3, help="bursts per leg")
    ap.add_argument("--burst", type=int, default=8, help="steps per burst")
    ap.add_argument("--in-flight", type=int, default=3)
    ap.add_argument("--no-pin", action="store_true", help="do not move the process next to the GPU")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()
    from bench import link_peaks, pin_to_gpu_numa_node
    from gigapaxos_amd import Engine, hri_create, load_hip, streams, S_OK
    from gigapaxos_amd._abi import _p
    from gigapaxos_amd.packed import pack_votes

    pinned = None if a.no_pin else pin_to_gpu_numa_node(0)
    G, K, F = a.groups, a.k, a.in_flight
    members = list(range(100, 100 + K))
    nv = G * K
    n_rounds = 1 + a.blocks * a.burst
    lib = load_hip()
    mem = np.tile(np.array(members, np.int32), (G, 1))
    os.environ["GPX_ASYNC_DEPTH"] = str(2 * F)
    eng = {}
    for leg in LEGS:
        e = Engine(lib, 100, G, kmax=K, window=8, max_batch=nv + 1024)
        assert (e.create_groups(np.arange(G, dtype=np.int32), mem, K, hri_create(G, K, 100)) == S_OK).all()
        eng[leg] = e
    del os.environ["GPX_ASYNC_DEPTH"]
    owner = eng[LEGS[0]]  # the input blocks: DMA memory is DMA memory to every engine
    link = link_peaks(torch, torch.device("cuda:0"), owner)

    hg = owner.host_alloc(G)
    hg[:] = np.arange(G, dtype=np.int32)
    rounds, packs, pack_us = [], [], []
    for r in range(n_rounds):
        cols = []
        for c in streams.vote_round(G, members, r, 100):
            b = owner.host_alloc(nv)
            b[:] = c
            cols.append(b)
        rounds.append(cols)
        rec, exc = owner.host_alloc(2 * nv, np.uint32), owner.host_alloc(8 * 1024, np.int32)  # (a clean round needs no row)
        t0 = time.perf_counter()
        p = pack_votes(cols, lib=lib, rec_out=rec, exc_out=exc)
        pack_us.append((time.perf_counter() - t0) * 1e6)
        assert p.needed == p.n_exc == 0 and (p.bnum, p.bcoord) == (0, 100)
        packs.append((p, p.struct()))
    ring = {}
    for leg in LEGS:
        e = eng[leg]
        ring[leg] = [([e.host_alloc(G) for _ in range(4)] + [e.host_alloc(G, np.uint8)],
                      [e.host_alloc(nv) for _ in range(5)] + [e.host_alloc(nv, np.uint8)],
                      e.host_alloc(1), e.host_alloc(nv, np.uint8)) for _ in range(F)]
    fn = lib.fn

    def submit(leg, r, s):
        e = eng[leg]
        o, d, no, st = ring[leg][s % F]
        c = rounds[r]
        tp, ta = C.c_uint64(0), C.c_uint64(0)
        rc = fn["propose_batch_async"](e.h, G, _p(hg), None, *[_p(x) for x in o], C.byref(tp))
        outs = [_p(x) for x in d] + [_p(no), _p(st)]
        if leg == "packed":
            rc |= fn["accept_reply_packed_async"](e.h, C.byref(packs[r][1]), *outs, C.byref(ta))
        else:
            six = leg == "six_columns"
            rc |= fn["accept_reply_batch_async"](e.h, nv, _p(c[0]), _p(c[1]) if six else None, _p(c[2]) if six else None,
                                                 0, 100, _p(c[3]), _p(c[4]), _p(c[5]), *outs, C.byref(ta))
        assert rc == 0, (leg, r, rc)
        return e, tp, ta, no

    def wait(t):
        e, tp, ta, no = t
        assert fn["engine_wait"](e.h, tp) == 0 and fn["engine_wait"](e.h, ta) == 0
        return int(no[0])

    for leg in LEGS:  # warm: every set of device columns (and the packed areas) allocated; the repeated round only
        for t in [submit(leg, 0, s) for s in range(F)]:  # brings late votes and leaves one more slot outstanding
            wait(t)
    times = {leg: [] for leg in LEGS}
    for b in range(a.blocks):
        for j in range(len(LEGS)):
            leg = LEGS[(b + j) % len(LEGS)]  # the order rotates from block to block
            flying = deque()
            t0 = time.perf_counter()
            for i in range(a.burst):
                r = 1 + b * a.burst + i
                flying.append(submit(leg, r, i))
                if len(flying) == F:
                    assert wait(flying.popleft()) == G
            while flying:
                assert wait(flying.popleft()) == G
            times[leg].append((time.perf_counter() - t0) / a.burst)
    g = np.arange(G, dtype=np.int32)
    snaps = [eng[leg].snapshot(g)[0].tobytes() for leg in LEGS]
    assert snaps[0] == snaps[1] == snaps[2], "the three forms left different group state"

    # k_votes_unpack alone, between device events (records already in HBM)
    e = eng["packed"]
    p = packs[1][0]
    d_rec = torch.from_numpy(p.rec.view(np.int32).reshape(-1).copy()).cuda()
    d_cols = [torch.empty(nv, dtype=torch.int32, device="cuda") for _ in range(6)]
    torch.cuda.synchronize()
    for reps in (3, 20):  # warm, then measured
        e.profile(2)
        for _ in range(reps):
            e.votes_unpack_dev(p, d_rec.data_ptr(), 0, [c.data_ptr() for c in d_cols])
        e.sync()
        launches, total_ms = e.profile_read()["k_votes_unpack"]
    e.profile(0)
    assert launches == 20
    unpack_ms = total_ms / launches

    peak = link["hipHostMalloc"]["both_directions_each_GBps"]
    b_out = G * 17 + nv + G * 21 + 4
    out = {"config": {"groups": G, "k": K, "votes_per_step": nv, "steps_in_flight": F, "blocks": a.blocks,
                      "burst": a.burst, "host_memory": "hipHostMalloc (gpx_host_alloc)",
                      "pinned_to_gpu_numa_node": pinned is not None, "stream": "pcg64 vote_round, one seeded round per step"},
           "link": link, "legs": {}}
    for leg, per_vote in zip(LEGS, (24, 16, 8)):
        ms = sorted(t * 1e3 for t in times[leg])
        te = sum(times[leg]) / len(times[leg])
        b_in = G * 4 + nv * per_vote
        out["legs"][leg] = {"ms_per_step": round(te * 1e3, 4), "ms_per_step_bursts": [round(x, 4) for x in ms],
                            "bytes_in_per_step": b_in, "bytes_out_per_step": b_out,
                            "pcie_in_GBps": round(b_in / te / 1e9, 1), "pcie_out_GBps": round(b_out / te / 1e9, 1),
                            "achieved_over_link_peak": {"in": round(b_in / te / 1e9 / max(peak, 1e-9), 3),
                                                        "out": round(b_out / te / 1e9 / max(peak, 1e-9), 3)}}
    cb = out["legs"]["common_ballot"]["ms_per_step"]
    out["packed_over_common_ballot"] = {"ms_per_step": round(out["legs"]["packed"]["ms_per_step"] / cb, 3),
                                        "bytes_in": round(out["legs"]["packed"]["bytes_in_per_step"] /
                                                          out["legs"]["common_ballot"]["bytes_in_per_step"], 3)}
    out["pack_host_us_per_call"] = {"median": round(float(np.median(pack_us[1:])), 1), "max": round(max(pack_us[1:]), 1),
                                    "what": "gpx_votes_pack of %d votes into gpx_host_alloc memory, one thread, outside the timed bursts" % nv}
    out["k_votes_unpack"] = {"ms_per_launch": round(unpack_ms, 5), "launches": launches, "votes": nv,
                             "GBps": round(nv * 32 / (unpack_ms * 1e-3) / 1e9, 1),
                             "what": "8 B read + 24 B written per vote, device events around gpx_votes_unpack_dev; repeated launches over "
                                     "the same buffers (they fit the 256 MB Infinity Cache: not an HBM rate)"}
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    del rounds, packs, ring, hg, rec, exc, cols, b, p, c
    for leg in LEGS:
        eng[leg].close(force=True)


if __name__ == "__main__":
    main()
