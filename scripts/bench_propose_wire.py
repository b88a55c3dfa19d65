#!/usr/bin/env python
"""The coordinator's request -> ACCEPT path on one MI355X, frames resident in HBM (not the judged bench line):

  REQUEST frames -> gpx_wire_decode_dev -> gpx_wire_request_sizes_dev -> gpx_request_batch_dev
  -> gpx_propose_batch_dev -> gpx_wire_pack_accepts_dev

Per-phase GPU time with torch events on the engine's stream, the pack's GB/s of bytes read (request frames) plus
written (ACCEPT frames) against the 8 TB/s of HBM, and as a yardstick in the same run the acceptor's
gpx_wire_decode_dev of the ACCEPT frames just packed.  Shapes:
  single   1 M groups with one 64-byte request each
  latched  10 k groups x 100 requests of 64 bytes latched into batches
  skew     one 2,000 x 1 KB batch among 100 k single 64-byte requests"""
import argparse
import json
import os
import struct
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gigapaxos_amd import Engine, hri_create, load_hip, S_OK  # noqa: E402
from gigapaxos_amd import wire as W  # noqa: E402

HBM_GBPS = 8000.0


def request_rows(name_rows, value_len, rid0):
    """REQUEST frames of equal length (the request part of W.accept_frames_fixed), requestID = rid0 + index"""
    buf, off = W.accept_frames_fixed(name_rows, 0, 0, 0, 0, 0, 0, value_len=value_len)
    n = name_rows.shape[0]
    f = buf.reshape(n, -1)[:, :int(off[1]) - 22].copy()
    f[:, 4:8] = np.frombuffer(struct.pack(">i", W.WT_REQUEST), np.uint8)
    o = 13 + name_rows.shape[1]
    rid = np.arange(rid0, rid0 + n, dtype=np.int64)
    f[:, o:o + 4], f[:, o + 4:o + 8] = W._be32_cols(rid >> 32), W._be32_cols(rid & 0xFFFFFFFF)
    return f


def shape(name, rng):
    """-> (groups, list of (group of each request, request rows))"""
    if name == "single":
        G = 1_000_000
        return G, [(np.arange(G), 64)]
    if name == "latched":
        G = 10_000
        return G, [(rng.permutation(np.repeat(np.arange(G), 100)), 64)]
    G = 100_001
    return G, [(np.arange(G - 1), 64), (np.full(2000, G - 1), 1024)]


def run(lib, name, rounds, rng):
    G, parts = shape(name, rng)
    names = W.fixed_names(np.arange(G))
    rows, lens = [], []
    for gsel, vlen in parts:
        r = request_rows(names[gsel], vlen, len(lens))
        rows.append(r.reshape(-1))
        lens += [r.shape[1]] * r.shape[0]
    buf = np.concatenate(rows)
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    n = len(lens)
    dev = torch.device("cuda:0")
    eng = Engine(lib, 100, G, kmax=3, window=8, max_batch=2 * max(n, G) + 1024)
    we = W.WireEngine(eng)
    mem = np.tile(np.array([100, 101, 102], np.int32), (G, 1))
    assert (eng.create_groups(np.arange(G, dtype=np.int32), mem, 3, hri_create(G, 3, 100)) == S_OK).all()
    nb_, noff = np.ascontiguousarray(names.reshape(-1)), np.arange(G + 1, dtype=np.int32) * names.shape[1]
    st, rows_g = np.zeros(G, np.uint8), np.arange(G, dtype=np.int32)  # (arrays alive across the call)
    we.lib.check(we.lib.fn["names_bind"](eng.h, G, nb_.ctypes.data, noff.ctypes.data, rows_g.ctypes.data,
                                         st.ctypes.data), "names_bind")
    assert (st == S_OK).all()
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(ts)
    eng.set_stream(ts.cuda_stream)
    i32 = lambda k: torch.zeros(max(k, 1), dtype=torch.int32, device=dev)  # noqa: E731
    u8 = lambda k: torch.zeros(max(k, 1), dtype=torch.uint8, device=dev)  # noqa: E731
    i64 = lambda k: torch.zeros(max(k, 1), dtype=torch.int64, device=dev)  # noqa: E731
    P = lambda t: t.data_ptr()  # noqa: E731
    d_buf, d_off = torch.from_numpy(buf).to(dev), torch.from_numpy(off).to(dev)
    fst, fg, ft = u8(n), i32(n), i32(n)
    rg, rs, ri, rf = i32(n), u8(n), i64(n), i32(n)
    counts = i32(8)
    est, wgt, leader, bst = i32(n), i32(n), i32(n), u8(n)
    bc = [i32(n) for _ in range(5)]
    bstop, nbt = u8(n), i32(1)
    pc = [i32(n) for _ in range(4)]
    pst = u8(n)
    cap = int(off[-1]) + 32 * n + 4096
    out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    foff, flen, fgi, fba, fof = i64(n + 1), i32(n), i32(n), i32(n), i32(n)
    nfo, nbo = i32(1), i64(1)
    acols = [i32(n) for _ in range(5)] + [u8(n), i32(n), i64(n), i32(n)]
    torch.cuda.synchronize()
    names_ph = ("decode", "request_sizes", "request_batch", "propose", "pack_accepts", "accept_decode")
    t = dict.fromkeys(names_ph, 0.0)
    nB = nF = nbytes = 0
    for r in range(rounds):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        ev[0].record()
        W.decode_dev(we, n, P(d_buf), P(d_off), P(fst), P(fg), P(ft), requests=(n, [P(rg), P(rs), P(ri), P(rf)]),
                     counts_ptr=P(counts))
        ev[1].record()
        W.request_sizes_dev(we, n, P(d_buf), P(d_off), n, P(rf), P(est), P(wgt))
        ev[2].record()
        we.lib.check(we.lib.fn["request_batch_dev"](eng.h, n, W._VP(P(rg)), W._VP(P(est)), W._VP(P(wgt)),
                                                    W._VP(P(rs)), 4 << 20, 2000, W._VP(P(leader)), W._VP(P(bst)),
                                                    *[W._VP(P(c)) for c in bc], W._VP(P(bstop)), W._VP(P(nbt))),
                     "request_batch_dev")
        ev[3].record()
        # propose_batch_dev takes a host count: the batches of this shape (known up front; checked below)
        nb_host = {"single": n, "latched": G * ((100 + 1999) // 2000), "skew": G}[name]
        eng.call_dev("propose_batch", nb_host, P(bc[0]), P(bstop), *[P(c) for c in pc], P(pst))
        ev[4].record()
        W.pack_accepts_dev(we, n, P(d_buf), P(d_off), n, P(rf), P(leader), nb_host, P(nbt),
                           (P(bc[0]), P(bc[1]), P(bc[2])), [P(c) for c in pc] + [P(pst)], P(out), cap, P(foff),
                           P(flen), P(fgi), P(fba), P(fof), P(nfo), P(nbo))
        ev[5].record()
        # the yardstick: the acceptor's decode of the frames just packed (frame i with its pad bytes, which a
        # ByteBuffer reader ignores; the offsets get their closing entry on the device)
        foff[nb_host:nb_host + 1].copy_(nbo)
        ev[6].record()
        W.decode_dev(we, nb_host, P(out), P(foff), P(fst), P(fg), P(ft), accepts=(nb_host, [P(c) for c in acols]),
                     counts_ptr=P(counts))
        ev[7].record()
        torch.cuda.synchronize()
        nB, nF, nbytes = int(nbt[0]), int(nfo[0]), int(nbo[0])
        assert nB == nb_host and nF == nB and nbytes <= cap, (nB, nb_host, nF, nbytes)
        assert int(counts[2]) == nF and int(counts[4]) == 0, counts.tolist()
        if r > 0:
            for k, ph in enumerate(names_ph):
                a, b = (k, k + 1) if k < 5 else (6, 7)
                t[ph] += ev[a].elapsed_time(ev[b])
    k = rounds - 1
    ms = {ph: round(t[ph] / k, 4) for ph in names_ph}
    read_b = int(off[-1])
    res = {"shape": name, "groups": G, "requests": n, "proposals": nB, "frames": nF, "request_bytes": read_b,
           "accept_bytes": nbytes, "ms": ms,
           "pack_GBps_read_plus_written": round((read_b + nbytes) / (ms["pack_accepts"] * 1e-3) * 1e-9, 1),
           "pack_fraction_of_8TBps": round((read_b + nbytes) / (ms["pack_accepts"] * 1e-3) * 1e-9 / HBM_GBPS, 3),
           "chain_ms": round(sum(ms[p] for p in names_ph[:5]), 4)}
    eng.profile(2)
    W.pack_accepts_dev(we, n, P(d_buf), P(d_off), n, P(rf), P(leader), nB, P(nbt), (P(bc[0]), P(bc[1]), P(bc[2])),
                       [P(c) for c in pc] + [P(pst)], P(out), cap, P(foff), P(flen), P(fgi), P(fba), P(fof), P(nfo),
                       P(nbo))
    eng.sync()
    res["kernels_us"] = {kk: round(v[1] * 1e3, 1) for kk, v in eng.profile_read().items()}
    eng.profile(0)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--shapes", default="single,latched,skew")
    args = ap.parse_args()
    lib = load_hip()
    rng = np.random.default_rng(0)
    res = {"bench": "propose_wire", "shapes": [run(lib, s, args.rounds, rng) for s in args.shapes.split(",")]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
