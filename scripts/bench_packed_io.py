#!/usr/bin/env python
"""Packed outputs (include/gpx_packed_out.h) on top of packed votes (include/gpx_packed.h), at bench.py's end-to-end
shape: one step = a propose call over G groups + the votes of G groups x K replicas from gpx_host_alloc memory, three
steps in flight (GPX_ASYNC_DEPTH=6), every round its own seeded round.

Three legs in ONE process, each on an engine of its own fed the same rounds, their bursts of `--burst` steps interleaved
and rotated, so that whatever else the host and the link are doing falls on all three alike:
  common_ballot  16 B per vote in, plain columns out (17 B per proposal, 21 B per decision) - bench.py's leg, the yardstick
  packed          8 B per vote in (gpx_accept_reply_packed_async), plain columns out - the best form before this one
  packed_io       8 B per vote in, ONE packed buffer out per call (gpx_propose_packed_out_async,
                  gpx_accept_reply_packed_io_async): 4 B per proposal, 8 B per decision; the per-vote status stays a byte
The outbound bytes of the packed_io leg are a fact of the format and are ASSERTED against the model; the time is
reported, beside the link's peaks from the same run (bench.link_peaks).  Also reported: the pack kernels' time between
device events (the _dev calls under gpx_profile_enable) and the host's unpack time, outside the timed bursts."""
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

LEGS = ("common_ballot", "packed", "packed_io")


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
    from gigapaxos_amd.packed_out import PackedOut, packed_out_bytes, unpack_decisions, unpack_proposals, RECORDS

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
    rounds, packs = [], []
    for r in range(n_rounds):
        cols = []
        for c in streams.vote_round(G, members, r, 100):
            b = owner.host_alloc(nv)
            b[:] = c
            cols.append(b)
        rounds.append(cols)
        rec, exc = owner.host_alloc(2 * nv, np.uint32), owner.host_alloc(8 * 1024, np.int32)  # (a clean round needs no row)
        p = pack_votes(cols, lib=lib, rec_out=rec, exc_out=exc)
        assert p.needed == p.n_exc == 0 and (p.bnum, p.bcoord) == (0, 100)
        packs.append((p, p.struct()))
    ring = {}
    for leg in LEGS:
        e = eng[leg]
        if leg == "packed_io":
            ring[leg] = [(e.host_alloc(packed_out_bytes(G), np.uint8), e.host_alloc(packed_out_bytes(nv), np.uint8), None,
                          e.host_alloc(nv, np.uint8)) for _ in range(F)]
        else:
            ring[leg] = [([e.host_alloc(G) for _ in range(4)] + [e.host_alloc(G, np.uint8)],
                          [e.host_alloc(nv) for _ in range(5)] + [e.host_alloc(nv, np.uint8)],
                          e.host_alloc(1), e.host_alloc(nv, np.uint8)) for _ in range(F)]
    fn = lib.fn

    def submit(leg, r, s):
        e = eng[leg]
        o, d, no, st = ring[leg][s % F]
        c = rounds[r]
        tp, ta = C.c_uint64(0), C.c_uint64(0)
        if leg == "packed_io":
            rc = fn["propose_packed_out_async"](e.h, G, _p(hg), None, _p(o), o.nbytes, C.byref(tp))
            rc |= fn["accept_reply_packed_io_async"](e.h, C.byref(packs[r][1]), _p(d), d.nbytes, _p(st), C.byref(ta))
            no = d[8:12].view(np.int32)  # the header's n: the call's n_out
        else:
            rc = fn["propose_batch_async"](e.h, G, _p(hg), None, *[_p(x) for x in o], C.byref(tp))
            outs = [_p(x) for x in d] + [_p(no), _p(st)]
            if leg == "packed":
                rc |= fn["accept_reply_packed_async"](e.h, C.byref(packs[r][1]), *outs, C.byref(ta))
            else:
                rc |= fn["accept_reply_batch_async"](e.h, nv, _p(c[0]), None, None, 0, 100, _p(c[3]), _p(c[4]), _p(c[5]),
                                                     *outs, C.byref(ta))
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

    # the last step of the packed_io and packed legs handled the same round: the same outputs, and the bytes the format promises
    s_last = (a.burst - 1) % F
    o_p, o_d, _, st_io = ring["packed_io"][s_last]
    po, pd = PackedOut(o_p, lib=lib), PackedOut(o_d, lib=lib)
    assert (po.form, po.n_exc, po.n) == (RECORDS, 0, G) and (pd.form, pd.n_exc, pd.n) == (RECORDS, 0, G)
    r32 = lambda x: (x + 31) & ~31  # noqa: E731
    b_out_io = (32 + r32(4 * G)) + (32 + r32(8 * G)) + nv  # the model: 4 + 8 B per group, 1 B per vote, two headers
    assert po.nbytes + pd.nbytes + nv == b_out_io, (po.nbytes, pd.nbytes, b_out_io)
    unpack_us = []
    for _ in range(5):
        t0 = time.perf_counter()
        props, dec = unpack_proposals(o_p, lib=lib), unpack_decisions(o_d, lib=lib)
        unpack_us.append((time.perf_counter() - t0) * 1e6)
    pl_o, pl_d, pl_no, pl_st = ring["packed"][s_last]
    assert int(pl_no[0]) == G and all((x == y).all() for x, y in zip(props, pl_o))
    assert all((x == y[:G]).all() for x, y in zip(dec, pl_d)) and (st_io == pl_st).all()

    # the pack kernels alone, between device events (columns already in HBM)
    e = eng["packed_io"]
    d_p = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in props]
    d_d = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in dec]
    d_n = torch.full((4,), G, dtype=torch.int32, device="cuda")
    d_out = torch.empty(packed_out_bytes(nv), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    kern = {}
    for what in ("proposals", "decisions"):
        for reps in (3, 20):  # warm, then measured
            e.profile(2)
            for _ in range(reps):
                if what == "proposals":
                    e.proposals_pack_dev(G, [t.data_ptr() for t in d_p], d_out.data_ptr())
                else:  # the grid is sized for the capacity, as in the asynchronous call
                    e.decisions_pack_dev(d_n.data_ptr(), G, [t.data_ptr() for t in d_d], d_out.data_ptr())
            e.sync()
            prof = e.profile_read()
        assert prof["k_po_count"][0] == prof["k_po_write"][0] == 20
        kern[what] = {"k_po_count_ms": round(prof["k_po_count"][1] / 20, 5), "k_po_write_ms": round(prof["k_po_write"][1] / 20, 5)}
    e.profile(0)

    peak = link["hipHostMalloc"]["both_directions_each_GBps"]
    b_out_plain = G * 17 + nv + G * 21 + 4
    out = {"config": {"groups": G, "k": K, "votes_per_step": nv, "steps_in_flight": F, "blocks": a.blocks,
                      "burst": a.burst, "host_memory": "hipHostMalloc (gpx_host_alloc)",
                      "pinned_to_gpu_numa_node": pinned is not None, "stream": "pcg64 vote_round, one seeded round per step"},
           "link": link, "legs": {}}
    for leg, per_vote, b_out in zip(LEGS, (16, 8, 8), (b_out_plain, b_out_plain, b_out_io)):
        ms = sorted(t * 1e3 for t in times[leg])
        te = sum(times[leg]) / len(times[leg])
        b_in = G * 4 + nv * per_vote
        out["legs"][leg] = {"ms_per_step": round(te * 1e3, 4), "ms_per_step_bursts": [round(x, 4) for x in ms],
                            "bytes_in_per_step": b_in, "bytes_out_per_step": b_out,
                            "pcie_in_GBps": round(b_in / te / 1e9, 1), "pcie_out_GBps": round(b_out / te / 1e9, 1),
                            "achieved_over_link_peak": {"in": round(b_in / te / 1e9 / max(peak, 1e-9), 3),
                                                        "out": round(b_out / te / 1e9 / max(peak, 1e-9), 3)}}
    pk, io = out["legs"]["packed"], out["legs"]["packed_io"]
    lo, hi = pk["ms_per_step_bursts"][0], pk["ms_per_step_bursts"][-1]
    out["packed_io_over_packed"] = {
        "ms_per_step": round(io["ms_per_step"] / pk["ms_per_step"], 3),
        "bytes_out": round(io["bytes_out_per_step"] / pk["bytes_out_per_step"], 3),
        "packed_bursts_ms": [lo, hi], "packed_io_bursts_ms": io["ms_per_step_bursts"],
        "verdict": ("faster: every packed_io burst below the packed leg's fastest" if io["ms_per_step_bursts"][-1] < lo else
                    "faster on average, bursts overlap" if io["ms_per_step"] < lo else
                    "no faster: inside the packed leg's own spread" if io["ms_per_step"] <= hi else "slower"),
        "bound_by": "inbound" if io["achieved_over_link_peak"]["in"] > io["achieved_over_link_peak"]["out"] else "outbound"}
    out["pack_kernels"] = dict(kern, entries=G, what="device events around gpx_proposals_pack_dev / gpx_decisions_pack_dev, "
                               "20 launches each over the same buffers (they fit the Infinity Cache: not an HBM rate)")
    out["unpack_host_us_per_step"] = {"median": round(float(np.median(unpack_us)), 1), "max": round(max(unpack_us), 1),
                                      "what": "gpx_proposals_unpack + gpx_decisions_unpack of %d entries each, one thread, "
                                              "outside the timed bursts" % G}
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    del rounds, packs, ring, hg, rec, exc, cols, b, p, c, o_p, o_d, st_io, po, pd, pl_o, pl_d, pl_no, pl_st
    for leg in LEGS:
        eng[leg].close(force=True)


if __name__ == "__main__":
    main()
