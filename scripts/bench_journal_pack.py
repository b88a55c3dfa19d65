#!/usr/bin/env python
"""The journal batches (include/gpx_journal.h) against a plain device copy and against what a host does today (a side
figure, not the judged bench line).

Shapes: 1 M single-request ACCEPT frames (gigapaxos_amd.wire.accept_frames_fixed, the generator scripts/bench_wire.py
uses) with 100 %, 50 % and 1 % of the records to log, and 10,000 frames of 64 KiB, all to log.  Per shape, the legs'
repetitions interleaved in one process (median and spread of at least seven, the first repetition of every leg a
warm-up):
  dev       gpx_journal_pack_dev, everything in device memory, between two device events
  memcpy    hipMemcpyAsync device-to-device of n_bytes in the same run: the copy's own roofline (reads and writes what
            k_jr_copy reads and writes, without the prefixes and without any gap in the source)
  host      gpx_journal_pack, pageable memory, wall time end to end
  baseline  what a host does today: r_flags and status copied back from the device, then FileLogger::logBatch's loop in
            C++ (scripts/journal_host_loop.cpp) over host-resident frames on one thread, wall time
k_jr_copy alone (and the other three kernels) come from the engine's profile in a pass of their own.  Every leg's bytes
are checked against the others once.  The bytes that cross the link follow from the layouts."""
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


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2] * 1e3, 4), "min_ms": round(xs[0] * 1e3, 4), "max_ms": round(xs[-1] * 1e3, 4)}


def host_loop_lib():
    d = tempfile.mkdtemp(prefix="gpx_journal_bench_")
    so = os.path.join(d, "journal_host_loop.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "scripts", "journal_host_loop.cpp")])
    lib = C.CDLL(so)
    lib.journal_host_loop.restype = C.c_longlong
    lib.journal_host_loop.argtypes = [C.c_int] + [C.c_void_p] * 5
    return lib


def hip_memcpy():
    """hipMemcpyAsync of the runtime torch already loaded, or None"""
    for name in ("libamdhip64.so.7", "libamdhip64.so.6", "libamdhip64.so"):
        try:
            f = C.CDLL(name).hipMemcpyAsync
        except (OSError, AttributeError):
            continue
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        return f
    return None


def shapes(n_small, n_big, big_len):
    from gigapaxos_amd import wire as W
    g = np.arange(n_small, dtype=np.int64) % 1_000_000
    block, off = W.accept_frames_fixed(W.fixed_names(g), 0, 1 + np.arange(n_small) % 8, 0, 100, 0, 100, value_len=64)
    rng = np.random.default_rng(1)
    for name, one_in in (("accepts_100pct", 1), ("accepts_50pct", 2), ("accepts_1pct", 100)):
        fl = np.where(rng.integers(0, one_in, n_small) == 0, 1, 2).astype(np.uint8)
        yield name, block, off, fl
    big = rng.integers(0, 256, n_big * big_len, dtype=np.uint8)
    yield "frames_64k", big, np.arange(n_big + 1, dtype=np.int64) * big_len, np.ones(n_big, np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--big", type=int, default=10_000)
    ap.add_argument("--big-len", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    a = ap.parse_args()
    assert a.reps >= 7

    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()
    from gigapaxos_amd import Engine, load_hip
    from gigapaxos_amd import journal as J

    loop = host_loop_lib()
    memcpy = hip_memcpy()
    N = max(a.records, a.big)
    e = Engine(load_hip(), 101, 64, kmax=3, window=8, max_batch=N)
    dev = torch.device("cuda:0")
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(ts)
    e.set_stream(ts.cuda_stream)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    res = {"reps": a.reps, "memcpy": "hipMemcpyAsync" if memcpy else "torch copy_", "shapes": {}}
    for name, block, off, r_flags in shapes(a.records, a.big, a.big_len):
        n = r_flags.shape[0]
        status = np.zeros(n, np.uint8)
        i32 = np.arange(n, dtype=np.int32)
        cols = [i32 % 1_000_000, 1 + i32 % 8, np.zeros(n, np.int32), np.full(n, 100, np.int32)]
        lens = np.diff(off)
        sel = r_flags & 1 == 1
        n_bytes, n_ent = int((lens[sel] + 4).sum()), int(sel.sum())
        d_block, d_off, d_fl, d_st = up(block), up(off), up(r_flags), up(status)
        d_cols = [up(c) for c in cols]
        d_out = torch.zeros(n_bytes + 16, dtype=torch.uint8, device=dev)
        d_copy = torch.zeros(n_bytes + 16, dtype=torch.uint8, device=dev)
        d_rows = [torch.zeros(max(n_ent, 1) * dt.itemsize, dtype=torch.uint8, device=dev) for _, dt in J.ROW_COLS]
        d_cnt = torch.zeros(32, dtype=torch.uint8, device=dev)
        h_out = J.aligned_bytes(n_bytes)
        h_fl, h_st = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        torch.cuda.synchronize()

        def dev_call():
            J.journal_pack_dev(e, n, d_block.data_ptr(), block.shape[0], n, d_off.data_ptr(), 0, 0,
                               [c.data_ptr() for c in d_cols], d_fl.data_ptr(), d_st.data_ptr(), 0, 0, d_out.data_ptr(),
                               n_bytes, n_ent, [r.data_ptr() for r in d_rows], d_cnt.data_ptr())

        def plain_copy():
            if memcpy:
                assert memcpy(d_copy.data_ptr(), d_block.data_ptr(), min(n_bytes, block.shape[0]), 3, ts.cuda_stream) == 0
            else:
                d_copy[:min(n_bytes, block.shape[0])].copy_(d_block[:min(n_bytes, block.shape[0])])
        t = {k: [] for k in ("dev", "memcpy", "host", "baseline")}
        dev_call()                                                     # the answer every other leg is held against
        torch.cuda.synchronize()
        c = J.JournalCounts.from_buffer_copy(d_cnt.cpu().numpy().tobytes())
        assert (c.n_entries, c.n_done, c.n_bad, c.n_bytes, c.bytes_done) == (n_ent, n_ent, 0, n_bytes, n_bytes)
        ref = d_out[:n_bytes].cpu().numpy()
        first = int(np.argmax(sel))                                    # every frame of a shape has the same length
        assert ref[:4].tobytes() == int(lens[first]).to_bytes(4, "big"), (name, ref[:8].tolist())
        assert ref[4:4 + 64].tobytes() == block[int(off[first]):int(off[first]) + 64].tobytes(), name
        for rep in range(a.reps + 1):                                  # the first repetition warms every leg
            order = ("dev", "memcpy", "host", "baseline") if rep & 1 else ("baseline", "host", "memcpy", "dev")
            for leg in order:
                if leg in ("dev", "memcpy"):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    ev[0].record(ts)
                    dev_call() if leg == "dev" else plain_copy()
                    ev[1].record(ts)
                    torch.cuda.synchronize()
                    dt = ev[0].elapsed_time(ev[1]) * 1e-3
                elif leg == "host":
                    t0 = time.perf_counter()
                    out, rows, c = J.journal_pack(e, block, off, *cols, r_flags, status, cap_bytes=n_bytes, cap_entries=n_ent,
                                                  out=h_out)
                    dt = time.perf_counter() - t0
                    if rep == 0:
                        assert (c.n_done, c.bytes_done) == (n_ent, n_bytes), (c.n_done, c.bytes_done, n_ent, n_bytes)
                        assert np.array_equal(out, ref), "the host twin's bytes are not the device form's"
                else:
                    t0 = time.perf_counter()
                    h_fl[:] = d_fl.cpu().numpy()                       # the two columns that say what to log
                    h_st[:] = d_st.cpu().numpy()
                    s = C.c_ulonglong(0)
                    got = loop.journal_host_loop(n, block.ctypes.data, off.ctypes.data, h_fl.ctypes.data, h_st.ctypes.data,
                                                 C.byref(s))
                    dt = time.perf_counter() - t0
                    assert got == n_bytes
                if rep:
                    t[leg].append(dt)
        e.profile(2)                                                   # per-kernel times in a pass of their own
        for _ in range(a.reps):
            dev_call()
        e.sync()
        prof = e.profile_read()
        e.profile(0)
        cell = {k: stats(v) for k, v in t.items()}
        cell["kernels_ms"] = {k: round(v[1] / v[0], 4) for k, v in prof.items() if k.startswith("k_jr_")}
        cell.update(records=n, entries=n_ent, n_bytes=n_bytes, frame_block_bytes=int(block.shape[0]))
        m = cell["memcpy"]["median_ms"]
        cell["dev_over_memcpy"] = round(cell["dev"]["median_ms"] / m, 2)
        cell["copy_kernel_over_memcpy"] = round(cell["kernels_ms"]["k_jr_copy"] / m, 2)
        cell["copy_kernel_GBps_read_plus_write"] = round(2 * n_bytes / cell["kernels_ms"]["k_jr_copy"] / 1e6, 1)
        cell["link_bytes"] = {
            "dev": {"to_device": 0, "to_host": 32},
            "host": {"to_device": int(block.shape[0]) + 8 * (n + 1) + 18 * n, "to_host": 32 + n_bytes + J.ROW_BYTES * n_ent},
            "baseline": {"to_device": 0, "to_host": 2 * n}}
        res["shapes"][name] = cell
        print("# %s: %s" % (name, json.dumps(cell)), file=sys.stderr, flush=True)
        del d_block, d_out, d_copy
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
