#!/usr/bin/env python3
"""In-process sweep (profiles/r16_stream_policy.txt, r17_two_word_staging.txt): several builds of the library side by side, the same seeded rounds, a fresh engine per line,
5 warm-up + 20 timed steps between device events, lines alternating direction.
    python scripts/inprocess_sweep.py --lines 7 [--k 5] [--sorted] [--mix] [--groups N] name=path ..."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=5)
    ap.add_argument("--groups", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--sorted", action="store_true")
    ap.add_argument("--mix", action="store_true")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--brackets", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("libs", nargs="+")
    a = ap.parse_args()
    import torch
    from gigapaxos_amd import Engine, hri_create, streams, S_OK, ORDERED_PROPOSE
    from gigapaxos_amd._abi import GpxLib

    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    torch.cuda.synchronize()
    G, K = a.groups, a.k
    members = list(range(100, 100 + K))
    cfg_id = 3 if K == 3 else 4
    R = a.warmup + a.steps + a.brackets
    rounds = [streams.vote_round_survey(G, members, r, 100, config_id=cfg_id, shuffled=not a.sorted, mix=a.mix) for r in range(R)]
    nvmax = max(c[0].shape[0] for c in rounds)
    pool = [[torch.from_numpy(c).to(dev) for c in cols] for cols in rounds]
    libs = [(s.split("=")[0], GpxLib(s.split("=")[1], "gpx_", device_api=True)) for s in a.libs]
    tstream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(tstream)
    mem = np.tile(np.array(members, np.int32), (G, 1))
    g_all = torch.arange(G, dtype=torch.int32, device=dev)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)  # noqa: E731
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)  # noqa: E731
    p = [i32(G) for _ in range(4)] + [u8(G)]
    d = [i32(nvmax) for _ in range(5)] + [u8(nvmax)]
    v_st = u8(nvmax)
    n_out = torch.zeros(R, dtype=torch.int32, device=dev)
    P = lambda t: t.data_ptr()  # noqa: E731
    res = {name: {"ms": [], "kern": []} for name, _ in libs}
    sums = {}

    def line(name, lib):
        eng = Engine(lib, 100, G, kmax=K, window=8, max_batch=nvmax + 1024, device=0)
        eng.set_stream(tstream.cuda_stream)
        eng.set_ordered_batches(ORDERED_PROPOSE)
        assert (eng.create_groups(np.arange(G, dtype=np.int32), mem, K, hri_create(G, K, 100)) == S_OK).all()

        def step(r):
            c = pool[r]
            eng.call_dev("propose_batch", G, P(g_all), 0, *[P(t) for t in p])
            eng.call_dev("accept_reply_batch", int(c[0].shape[0]), *[P(t) for t in c], *[P(t) for t in d], n_out[r:].data_ptr(), P(v_st))
        for r in range(a.warmup):
            step(r)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(tstream)
        for r in range(a.warmup, a.warmup + a.steps):
            step(r)
        e1.record(tstream)
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.steps
        eng.profile(2)
        for r in range(a.warmup + a.steps, R):
            step(r)
        torch.cuda.synchronize()
        prof = eng.profile_read()
        eng.profile(0)
        kern = {k: round(v[1] * 1000.0 / max(v[0], 1), 2) for k, v in prof.items()}
        # what the line computed: the decision counts of every round and a checksum of the last round's columns
        chk = (n_out.cpu().numpy().tolist(), [int(t[: int(n_out[R - 1].item())].to(torch.int64).sum().item()) for t in d])
        eng.close()
        res[name]["ms"].append(round(ms, 4))
        res[name]["kern"].append(kern)
        sums.setdefault(name, chk)
        assert sums[name] == chk, name
        print(name, round(ms, 4), json.dumps(kern), flush=True)

    for i in range(a.lines):
        for name, lib in (libs if i % 2 == 0 else libs[::-1]):
            line(name, lib)
    first = sums[libs[0][0]]
    for name, _ in libs:
        ks = sorted(set().union(*[set(k) for k in res[name]["kern"]]))
        med = {k: float(np.median([x.get(k, 0.0) for x in res[name]["kern"]])) for k in ks}
        print("SUMMARY", name, "ms", res[name]["ms"], "median", float(np.median(res[name]["ms"])), "kern", json.dumps(med),
              "same_results_as_first", sums[name] == first, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"))


if __name__ == "__main__":
    main()
