#!/usr/bin/env python
"""The journal compaction (include/gpx_journal_gc.h) against a plain device copy, against the parent commit's way on the
device, and against what a host does today (a side figure, not the judged bench line).

Workload: a journal of 1 M entries of 163 bytes (the frame of scripts/bench_journal_pack.py: a single-request ACCEPT
with a 64-byte value), under three keep patterns: every second entry kept, runs of 64 kept and dropped alternately,
everything kept.  Per pattern, the legs' repetitions interleaved in one process (median and spread of --reps, default
three; one more repetition in front warms every leg):
  dev       gpx_journal_gc_dev, everything in device memory, between two device events
  memcpy    hipMemcpyAsync device-to-device of the kept bytes: the copy's own roofline
  pack      the parent commit's way: the same selection through gpx_journal_pack_dev in its frame_len form, the
            survivors as frames; the selection (frame offsets, lengths, columns) is computed beforehand and not timed
  host      gpx_journal_gc, pageable memory, wall time end to end
  baseline  compactLogfile's loop restated in C++ (scripts/journal_gc_host_loop.cpp), one thread, wall time
k_jg_copy and k_jr_copy alone (and the other kernels) come from the engine's profile in a pass of their own, in the same
run.  Every leg's bytes are checked against the others once.  The bytes the host twin moves over the link follow from
its two passes.  With --resources the static resource lines of the four kernels (scripts/kernel_resources.py, no GPU
needed, taken beforehand) are copied into the result."""
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


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2] * 1e3, 4), "min_ms": round(xs[0] * 1e3, 4), "max_ms": round(xs[-1] * 1e3, 4)}


def host_loop_lib():
    d = tempfile.mkdtemp(prefix="gpx_journal_gc_bench_")
    so = os.path.join(d, "journal_gc_host_loop.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "scripts", "journal_gc_host_loop.cpp")])
    lib = C.CDLL(so)
    lib.journal_gc_host_loop.restype = C.c_longlong
    lib.journal_gc_host_loop.argtypes = [C.c_void_p, C.c_longlong] + [C.c_void_p] * 4
    return lib


def patterns(n):
    i = np.arange(n)
    yield "every_second_kept", (i & 1) == 1
    yield "runs_of_64", ((i >> 6) & 1) == 0
    yield "all_kept", np.ones(n, bool)


def main():
    from bench_journal_pack import hip_memcpy
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1_000_000)
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--resources", default=None, help="output of scripts/kernel_resources.py: its k_jg_ lines go into the result")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    a = ap.parse_args()
    assert a.reps >= 3

    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()
    from gigapaxos_amd import Engine, load_hip, hri_create, S_OK, wire as W
    from gigapaxos_amd import journal as J, journal_gc as JG

    loop = host_loop_lib()
    memcpy = hip_memcpy()
    n, G = a.entries, a.groups
    e = Engine(load_hip(), 101, G, kmax=3, window=8, max_batch=n)
    mem = np.tile(np.array([100, 101, 102], np.int32), (G, 1))
    assert (e.create_groups(np.arange(G), mem, 3, hri_create(G, 3, 100)) == S_OK).all()     # every acceptor's GC slot is -1
    gc_slot = np.full(G, -1, np.int32)
    dev = torch.device("cuda:0")
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(ts)
    e.set_stream(ts.cuda_stream)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731

    # the journal: <be32 len><frame> for every frame of the pack bench's generator
    g = np.arange(n, dtype=np.int64) % G
    block, off = W.accept_frames_fixed(W.fixed_names(g), 0, 1 + np.arange(n) % 8, 0, 100, 0, 100, value_len=64)
    ln = int(off[1] - off[0])
    assert (np.diff(off) == ln).all()
    size = n * (4 + ln)
    file = J.aligned_bytes((size + 15) // 16 * 16)
    rows2d = file[:size].reshape(n, 4 + ln)
    rows2d[:, :4] = np.frombuffer(ln.to_bytes(4, "big"), np.uint8)
    rows2d[:, 4:] = block.reshape(n, ln)
    del block
    e_gidx = g.astype(np.int32)
    e_off = np.arange(n, dtype=np.int64) * (4 + ln)
    e_len = np.full(n, ln, np.int32)
    e_bnum, e_bcoord = np.zeros(n, np.int32), np.full(n, 100, np.int32)
    d_file = up(file)
    d_in = [up(c) for c in (e_gidx, e_off, e_len, e_bnum, e_bcoord)]
    res = {"reps": a.reps, "entries": n, "entry_bytes": 4 + ln, "file_bytes": size, "memcpy": "hipMemcpyAsync" if memcpy else "torch copy_",
           "patterns": {}}
    if a.resources:
        res["kernel_resources"] = [s.rstrip() for s in open(a.resources) if s.startswith("kernel ") or "k_jg_" in s or "k_jr_copy" in s]
    for name, keep in patterns(n):
        e_slot = np.where(keep, 0, -1).astype(np.int32)                 # slot - (-1) > 0 iff kept
        nk = int(keep.sum())
        kb = nk * (4 + ln)
        d_slot = up(e_slot)
        d_out = torch.zeros(kb + 16, dtype=torch.uint8, device=dev)
        d_out2 = torch.zeros(kb + 16, dtype=torch.uint8, device=dev)
        d_copy = torch.zeros(kb + 16, dtype=torch.uint8, device=dev)
        d_ver = torch.zeros(n, dtype=torch.uint8, device=dev)
        d_rows = [torch.zeros(max(nk, 1) * dt.itemsize, dtype=torch.uint8, device=dev) for _, dt in JG.ROW_COLS]
        d_cnt = torch.zeros(64, dtype=torch.uint8, device=dev)
        # the parent commit's way, its selection made beforehand: the survivors as frames of the file
        sel = np.nonzero(keep)[0]
        p_off, p_len = up(e_off[sel] + 4), up(e_len[sel])
        p_cols = [up(c[sel]) for c in (e_gidx, e_slot, e_bnum, e_bcoord)]
        p_fl, p_st = up(np.ones(nk, np.uint8)), up(np.zeros(nk, np.uint8))
        p_rows = [torch.zeros(max(nk, 1) * dt.itemsize, dtype=torch.uint8, device=dev) for _, dt in J.ROW_COLS]
        p_cnt = torch.zeros(32, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def dev_call():
            JG.journal_gc_dev(e, n, d_file.data_ptr(), size, 0, [d_in[0].data_ptr(), d_slot.data_ptr(), d_in[1].data_ptr(),
                                                                 d_in[2].data_ptr(), d_in[3].data_ptr(), d_in[4].data_ptr(), 0],
                              0, 0, d_out.data_ptr(), kb, nk, d_ver.data_ptr(), [r.data_ptr() for r in d_rows], d_cnt.data_ptr())

        def pack_call():
            J.journal_pack_dev(e, nk, d_file.data_ptr(), size, nk, p_off.data_ptr(), p_len.data_ptr(), 0,
                               [c.data_ptr() for c in p_cols], p_fl.data_ptr(), p_st.data_ptr(), 0, 0, d_out2.data_ptr(), kb, nk,
                               [r.data_ptr() for r in p_rows], p_cnt.data_ptr())

        def plain_copy():
            if memcpy:
                assert memcpy(d_copy.data_ptr(), d_file.data_ptr(), kb, 3, ts.cuda_stream) == 0
            else:
                d_copy[:kb].copy_(d_file[:kb])
        dev_call(), pack_call()                                         # the answers every other leg is held against
        torch.cuda.synchronize()
        c = JG.JournalGcCounts.from_buffer_copy(d_cnt.cpu().numpy().tobytes())
        assert (c.n_keep, c.n_done, c.n_bad, c.keep_bytes, c.bytes_done, c.named_bytes) == (nk, nk, 0, kb, kb, size), name
        assert c.unchanged == int(nk == n)
        ref = d_out[:kb].cpu().numpy()
        assert np.array_equal(ref, rows2d[keep].reshape(-1)), name + ": the device form's bytes"
        assert np.array_equal(d_out2[:kb].cpu().numpy(), ref), name + ": the pack's bytes"
        t = {k: [] for k in ("dev", "memcpy", "pack", "host", "baseline")}
        for rep in range(a.reps + 1):                                   # the first repetition warms every leg
            order = ("dev", "memcpy", "pack", "host", "baseline")
            for leg in (order if rep & 1 else order[::-1]):
                if leg in ("dev", "memcpy", "pack"):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    ev[0].record(ts)
                    {"dev": dev_call, "memcpy": plain_copy, "pack": pack_call}[leg]()
                    ev[1].record(ts)
                    torch.cuda.synchronize()
                    dt = ev[0].elapsed_time(ev[1]) * 1e-3
                elif leg == "host":
                    t0 = time.perf_counter()
                    out, k_rows, ver, hc = JG.journal_gc(e, file, e_gidx, e_slot, e_off, e_len, e_bnum, e_bcoord, in_bytes=size,
                                                         cap_bytes=kb, cap_entries=nk)
                    dt = time.perf_counter() - t0
                    if rep == 0:
                        assert (hc.n_done, hc.bytes_done, hc.unchanged) == (nk, kb, int(nk == n))
                        assert np.array_equal(out, ref), "the host twin's bytes are not the device form's"
                else:
                    s = C.c_ulonglong(0)
                    t0 = time.perf_counter()
                    got = loop.journal_gc_host_loop(file.ctypes.data, size, e_gidx.ctypes.data, e_slot.ctypes.data, gc_slot.ctypes.data,
                                                    C.byref(s))
                    dt = time.perf_counter() - t0
                    assert got == kb
                if rep:
                    t[leg].append(dt)
        # the twin's outcome-only form of this pattern: what GPX_JG_SKIP_UNCHANGED saves on an untouched file
        t0 = time.perf_counter()
        _, _, _, hc = JG.journal_gc(e, file, e_gidx, e_slot, e_off, e_len, in_bytes=size, flags=JG.JG_COUNT_ONLY)
        t_count = time.perf_counter() - t0
        e.profile(2)                                                    # per-kernel times in a pass of their own
        for _ in range(a.reps):
            dev_call(), pack_call()
        e.sync()
        prof = e.profile_read()
        e.profile(0)
        cell = {k: stats(v) for k, v in t.items()}
        cell["host_count_only_ms"] = round(t_count * 1e3, 4)
        cell["kernels_ms"] = {k: round(v[1] / v[0], 4) for k, v in prof.items() if k.startswith(("k_jg_", "k_jr_"))}
        cell.update(entries=n, kept=nk, kept_bytes=kb, runs=int(c.n_runs_done))
        m = cell["memcpy"]["median_ms"]
        cell["dev_over_memcpy"] = round(cell["dev"]["median_ms"] / m, 2)
        cell["dev_over_pack"] = round(cell["dev"]["median_ms"] / cell["pack"]["median_ms"], 2)
        cell["jg_copy_over_jr_copy"] = round(cell["kernels_ms"]["k_jg_copy"] / cell["kernels_ms"]["k_jr_copy"], 2)
        cell["jg_copy_over_memcpy"] = round(cell["kernels_ms"]["k_jg_copy"] / m, 2)
        cell["jg_copy_GBps_read_plus_write"] = round(2 * kb / cell["kernels_ms"]["k_jg_copy"] / 1e6, 1)
        pass1 = {"to_device": 20 * n, "to_host": 64 + n}                # four row columns in; the counts and verdicts back
        chunks = -(-kb // (64 << 20)) if nk else 0                      # windows of 64 MiB; dropped bytes inside a window cross too
        span = size if nk else 0
        cell["link_bytes"] = {
            "dev": {"to_device": 0, "to_host": 64},
            "host_outcome_only": pass1,
            "host": {"to_device": pass1["to_device"] + (span + 29 * n if nk else 0),
                     "to_host": pass1["to_host"] + (64 * max(chunks, 1) + kb + 32 * nk if nk else 0)},
            "baseline": {"to_device": 0, "to_host": 0}}
        res["patterns"][name] = cell
        print("# %s: %s" % (name, json.dumps(cell)), file=sys.stderr, flush=True)
        del d_out, d_out2, d_copy
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    e.close()


if __name__ == "__main__":
    main()
