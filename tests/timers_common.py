"""Scenarios of the retransmission sweep (include/gpx_timers.h).  A History applies one sequence of operations to a HIP
engine (None on a machine without a GPU) and to the CPU oracle; the expected answer of a sweep is tests/timers_model.py
over the ORACLE's dense poke rows (orc_poke_scan).  The model's timer words live in the History and are compared with
the engine's through the call's outputs over successive sweeps.  The scenario functions are shared: the GPU file runs
them against the HIP library, tests/test_retransmit_sweep_model.py runs them on the oracle alone to show that none is
vacuous."""
import numpy as np

from gigapaxos_amd import Engine, hri_create, S_OK, RETIRE_KILL, C_HASVALUE
from tests import timers_model as M

ME = 100
SENTINEL = 0xA5
PAD = 9                                   # entries behind cap that no call may touch
T = 1024                                  # entries per workgroup of the first launch
G3 = 3000                                 # two full tiles and a partial one
EDGES = np.array([0, 1023, 1024, 2047, 2048, 2999])
ACCEPT_MS = [100, 150, 225]               # 100 * 1.5^c
PREPARE_MS = [40, 60, 90]


def engine(lib, n_groups, kmax=3, k=3, window=8):
    e = Engine(lib, ME, n_groups, kmax=kmax, window=window, max_batch=max(n_groups, 1 << 12))
    g = np.arange(n_groups, dtype=np.int32)
    mem = np.zeros((n_groups, kmax), np.int32)
    mem[:, :k] = np.arange(ME, ME + k)
    rows = hri_create(n_groups, k, ME)
    rows["node_slots"][:, :k] = (g[:, None] * 7 + np.arange(k)[None, :] * 3) % 5
    assert (e.create_groups(g, mem, k, rows) == S_OK).all()
    return e


def propose(e, g):
    g = np.asarray(g, np.int32)
    out = e.propose(g)
    assert (out[4] == S_OK).all()
    return out


def replies(e, g, slot, acceptors, bnum=0):
    """accept replies of `acceptors` for (slot, ballot (bnum, ME)) of the groups g -> decisions"""
    g = np.asarray(g, np.int32)
    n = 0
    for acc in acceptors:
        n += e.accept_reply(g, np.full(g.size, bnum, np.int32), np.full(g.size, ME, np.int32),
                            np.broadcast_to(np.asarray(slot, np.int32), g.shape), np.full(g.size, acc, np.int32),
                            np.zeros(g.size, np.int32)).gidx.shape[0]
    return n


def majority(k):
    return range(ME, ME + k // 2 + 1)


def decide(e, g, slot=1, k=3, bnum=0):
    g = np.asarray(g, np.int32)
    if g.size:
        assert replies(e, g, slot, majority(k), bnum) == g.size


def whole_round(e, g, k=3):
    """propose, a majority of accept replies, the decision committed: the acceptor's slot moves on"""
    g = np.asarray(g, np.int32)
    sl, bn, bc, med, st = propose(e, g)
    assert replies(e, g, sl, majority(k)) == g.size
    status, _ = e.commit(g, bn, bc, sl, med, np.full(g.size, C_HASVALUE, np.uint8))
    assert (status == S_OK).all()


class History:
    def __init__(self, hip_lib, oracle_lib, n_groups, cfg=(ACCEPT_MS, PREPARE_MS), **kw):
        self.n, self.k = n_groups, kw.get("k", 3)
        self.eh = engine(hip_lib, n_groups, **kw) if hip_lib is not None else None
        self.eo = engine(oracle_lib, n_groups, **kw)
        self.T = M.Timers(n_groups)
        self.accept_ms, self.prepare_ms = cfg
        self.stats = dict(hits=0, waiting_not_due=0, rekeyed=0, sweeps=0)

    def do(self, op):
        for e in (self.eh, self.eo):
            if e is not None:
                op(e)

    def close(self):
        for e in (self.eh, self.eo):
            if e is not None:
                e.close()

    def rows(self, gidx, n):
        """the oracle's dense poke rows of the entries, and their groups"""
        if gidx is None:
            groups = np.arange(n, dtype=np.int64)
            cols = self.eo.poke_scan(np.arange(n, dtype=np.int32))
        else:
            groups = np.asarray(gidx, np.int64)
            cols = self.eo.poke_scan(np.asarray(gidx, np.int32))
        return groups, dict(zip(("poke", "slot", "bnum", "bcoord", "median_cp", "flags", "heard", "status"), cols))


# ---- the two forms of the call, into sentinel-filled buffers with padding behind cap --------------------------------------
def filled(count, dtype):
    return np.frombuffer(bytes([SENTINEL]) * (count * np.dtype(dtype).itemsize), dtype).copy()


def untouched(a):
    return (np.asarray(a).view(np.uint8) == SENTINEL).all()


def call_host(eh, gidx, n, now, cfg, flags, cap, null_cols=False, alloc=False):
    from gigapaxos_amd import timers

    if null_cols:
        out = None
    elif alloc:                            # memory from gpx_host_alloc
        out = [eh.host_alloc(cap + PAD, dt) for _, dt in timers.RTX_COLS]
        for a in out:
            a.view(np.uint8)[...] = SENTINEL
    else:
        out = [filled(cap + PAD, dt) for _, dt in timers.RTX_COLS]
    cols, counts = timers.retransmit_sweep(eh, now, cfg, gidx, flags, cap=cap, n=n, out=out)
    if out is not None:
        for c, a in zip(cols, out):
            assert c.shape[0] == max(0, min(counts.n_hits, cap)) and c.ctypes.data == a.ctypes.data
    if alloc:
        pageable = [a.copy() for a in out]
        del cols, c, a
        eh.host_free(*out)
        out = pageable
    return out, counts


def call_dev(eh, gidx, n, now, cfg, flags, cap, null_cols=False):
    """the _dev form: device buffers everywhere, the counts read from device memory after one engine sync"""
    import torch
    from gigapaxos_amd import timers

    dts = [dt for _, dt in timers.RTX_COLS]
    bufs = [] if null_cols else [torch.full(((cap + PAD) * dt.itemsize,), SENTINEL, dtype=torch.uint8, device="cuda")
                                 for dt in dts]
    cnt = torch.full((16 + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    g = None if gidx is None else torch.from_numpy(np.ascontiguousarray(gidx, np.int32)).cuda()
    torch.cuda.synchronize()
    timers.retransmit_sweep_dev(eh, n, 0 if g is None else g.data_ptr(), now, cfg, flags, cap,
                                [b.data_ptr() for b in bufs] if bufs else [0] * len(dts), cnt.data_ptr())
    eh.sync()
    raw = cnt.cpu().numpy()
    assert untouched(raw[16:])
    counts = timers.RtxCounts.from_buffer_copy(raw[:16].tobytes())
    out = None if null_cols else [b.cpu().numpy().view(dt) for b, dt in zip(bufs, dts)]
    return out, counts


def check(H, now, flags=0, cap=None, form="dev", gidx=None, n=None, null_cols=False, what=""):
    """One call: the model over the oracle's rows, and - where there is a HIP engine - the call itself against it, bit
    for bit: counts, the ten columns, the sentinel from the last written entry on.  Returns the model's answer."""
    n = (H.n if gidx is None else len(gidx)) if n is None else n
    cap = n if cap is None else cap
    groups, rows = H.rows(gidx, n)
    before = H.T.key.copy()
    r = M.sweep(H.T, groups, rows, now, H.accept_ms, H.prepare_ms, flags, cap)
    r["groups"] = groups
    if not flags & M.PEEK:
        armed = groups[r["armed"]]
        H.stats["hits"] += r["due"].size
        H.stats["waiting_not_due"] += r["counts"][2] - r["counts"][0]
        H.stats["rekeyed"] += int((before[armed] != 0).sum())
        H.stats["sweeps"] += 1
    if H.eh is None:
        return r
    from gigapaxos_amd import timers

    cfg = timers.make_cfg(H.accept_ms, H.prepare_ms)
    if form == "dev":
        out, counts = call_dev(H.eh, gidx, n, now, cfg, flags, cap, null_cols)
    else:
        out, counts = call_host(H.eh, gidx, n, now, cfg, flags, cap, null_cols, alloc=form == "host_alloc")
    tag = f"{what} {form} now={now} flags={flags} cap={cap}"
    got = (counts.n_hits, counts.n_nogroup, counts.n_waiting, counts.n_fired)
    print(f"{tag}: counts {got}, model {r['counts']}")
    assert got == r["counts"], tag
    k = r["hits"].size
    if out is not None:
        for a, name in zip(out, M.OUT_COLS):
            assert a[:k].tolist() == r["cols"][name].tolist(), f"{tag}: column {name}"
        assert all(untouched(a[k:]) for a in out), f"{tag}: written at or beyond entry {k}"
    return r


def peek_all(H, now, cap=None, **kw):
    """both forms, twice the host one: a peek changes nothing, so all three see the same"""
    for form in ("host", "dev", "host"):
        r = check(H, now, M.PEEK, cap, form, **kw)
    return r


def hit_set(name, n=G3):
    if name == "edges":
        return EDGES
    if name == "hole":                      # tile 0 nothing but hits, tile 1 empty, the partial tile 2 nothing but hits
        return np.concatenate([np.arange(0, T), np.arange(2 * T, n)])
    if name == "all":
        return np.arange(n)
    assert name == "none"
    return np.zeros(0, np.int64)


# ---- the scenarios -------------------------------------------------------------------------------------------------------
def waiting_table(hip_lib, oracle_lib, n, chosen, **kw):
    """every group proposes; all but `chosen` get their majority and stop waiting"""
    H = History(hip_lib, oracle_lib, n, **kw)
    allg = np.arange(n, dtype=np.int32)
    H.do(lambda e: propose(e, allg))
    H.do(lambda e: decide(e, np.setdiff1d(allg, chosen), 1, H.k))
    return H


def hits_by_construction(hip_lib, oracle_lib, name):
    chosen = hit_set(name)
    H = waiting_table(hip_lib, oracle_lib, G3, chosen)
    r = check(H, 1000, what="arm")
    assert r["counts"] == (0, 0, chosen.size, 0) and r["armed"].tolist() == chosen.tolist()
    r = peek_all(H, 1100, what="at the threshold")                      # strict: 100 ms is not longer than 100 ms
    assert r["counts"] == (0, 0, chosen.size, 0)
    r = peek_all(H, 1101, what=name)
    assert r["groups"][r["hits"]].tolist() == chosen.tolist()
    r = check(H, 1101, what=name)
    assert r["groups"][r["hits"]].tolist() == chosen.tolist() and r["counts"] == (chosen.size, 0, chosen.size, chosen.size)
    assert set(r["cols"]["count"].tolist()) <= {1} and set(r["cols"]["waited"].tolist()) <= {101}
    assert set(r["cols"]["slot"].tolist()) <= {1} and set(r["cols"]["poke"].tolist()) <= {M.POKE_ACCEPT}
    r = check(H, 1102, form="host", what="re-armed")
    assert r["counts"] == (0, 0, chosen.size, 0)
    H.close()
    return H.stats


def six_sweeps_of_backoff(hip_lib, oracle_lib):
    n = T + 1
    chosen = np.arange(0, n, 3)
    H = waiting_table(hip_lib, oracle_lib, n, chosen)
    gone, heard = int(chosen[5]), int(chosen[7])
    fired = []
    for step, now in enumerate([0, 101, 251, 252, 478, 704]):
        if step == 3:                       # between two sweeps: one gets its majority, one a single reply
            H.do(lambda e: decide(e, [gone], 1, H.k))
            H.do(lambda e: replies(e, [heard], 1, [ME + 1]))
        peek_all(H, now, what=f"sweep {step}")
        r = check(H, now, form="dev" if step & 1 else "host", what=f"sweep {step}")
        fired.append((r["counts"][0], sorted(set(r["cols"]["count"].tolist())), sorted(set(r["cols"]["waited"].tolist()))))
        if step == 3:
            i = r["groups"][r["hits"]].tolist().index(heard)
            assert r["cols"]["heard"][i] != 0 and gone not in r["groups"][r["hits"]]
    m = chosen.size
    assert fired == [(0, [], []), (m, [1], [101]), (0, [], []), (m - 1, [2], [151]), (m - 1, [3], [226]),
                     (m - 1, [4], [226])], fired
    H.close()
    return H.stats


def prepare_kind(hip_lib, oracle_lib):
    n = T + 1
    H = History(hip_lib, oracle_lib, n)
    allg = np.arange(n, dtype=np.int32)
    running = allg[allg % 3 == 0]
    accepting = allg[allg % 3 == 1][:100]
    H.do(lambda e: propose(e, accepting))
    H.do(lambda e: e.election_begin(running, np.ones(running.size, np.int32)))
    r = check(H, 10, what="arm")
    assert r["counts"] == (0, 0, running.size + accepting.size, 0)
    r = check(H, 51, form="host", what="the PREPAREs' own table")       # 41 ms: longer than 40, not than 100
    assert r["groups"][r["hits"]].tolist() == running.tolist() and set(r["cols"]["poke"].tolist()) == {M.POKE_PREPARE}
    assert set(r["cols"]["bnum"].tolist()) == {1}
    # prepare replies: a majority elects some - each reply carries an accepted pvalue for slot 1, which the new
    # coordinator must propose again: they wait as ACCEPT now, a new key - a single reply changes `heard` only, and one
    # group meets a higher ballot and is preempted
    elected, single, preempted = running[:40], running[40:60], running[60:61]

    def reply(e, g, acceptor, bnum=1, bcoord=ME):
        e.prepare_reply(g, np.full(g.size, acceptor, np.int32), np.full(g.size, bnum, np.int32),
                        np.full(g.size, bcoord, np.int32), np.ones(g.size, np.int32),
                        [[(1, 0, ME, 7 + int(x), 0)] for x in g])
    H.do(lambda e: [reply(e, elected, a) for a in majority(H.k)])
    H.do(lambda e: reply(e, single, ME + 1))
    H.do(lambda e: reply(e, preempted, ME + 1, 5, ME + 1))
    groups, rows = H.rows(None, n)
    assert (rows["poke"][elected] == M.POKE_ACCEPT).all() and (rows["poke"][single] == M.POKE_PREPARE).all()
    assert rows["poke"][preempted[0]] == M.POKE_NONE and (rows["heard"][single] != 0).all()
    r = check(H, 112, what="after the election")                          # 61 ms on: the second PREPARE threshold
    hit = r["groups"][r["hits"]]
    assert np.isin(accepting, hit).all()                                   # 102 ms after their arming
    assert not np.isin(elected, hit).any() and np.isin(elected, r["groups"][r["armed"]]).all()
    assert np.isin(single, hit).all() and not np.isin(preempted, hit).any()
    r = check(H, 213, form="host", what="elected ones fire as ACCEPTs")
    i = np.isin(r["groups"][r["hits"]], elected)
    assert i.sum() == elected.size and set(r["cols"]["poke"][i].tolist()) == {M.POKE_ACCEPT}
    assert set(r["cols"]["count"][i].tolist()) == {1} and set(r["cols"]["waited"][i].tolist()) == {101}
    H.close()
    return H.stats


def saturation(hip_lib, oracle_lib):
    n = 300
    chosen = np.arange(3, n, 15)
    H = waiting_table(hip_lib, oracle_lib, n, chosen, cfg=([0, 1], [0, 1]))
    check(H, 0, form="host", what="arm")
    now, r = 0, None
    for step in range(258):
        now += 2
        r = check(H, now, form="host" if step % 50 else "dev", what=f"step {step}")
        assert r["counts"] == (chosen.size, 0, chosen.size, chosen.size)
        assert set(r["cols"]["count"].tolist()) == {min(step + 1, 255)}
    r = check(H, now + 1, form="dev", what="the last threshold, not due")    # 1 ms is not longer than 1 ms
    assert r["counts"][0] == 0 and set(H.T.count[chosen].tolist()) == {255}
    H.close()
    return H.stats


def clock_wrap(hip_lib, oracle_lib):
    n = 200
    chosen = np.arange(0, n, 2)
    H = waiting_table(hip_lib, oracle_lib, n, chosen)
    start = 2**31 - 1 - 50
    check(H, start, what="arm")
    r = check(H, 2**31 - 1, form="host", what="the last positive instant")
    assert r["counts"][0] == 0
    r = check(H, 2**31 + 60, what="across 2^31")                           # -2^31 + 60 as the call sees it
    assert r["counts"][0] == chosen.size and set(r["cols"]["waited"].tolist()) == {111} and M.wrap32(2**31 + 60) < 0
    r = check(H, 2**31, form="host", what="the clock stepped back")
    assert r["counts"][0] == 0
    r = check(H, 2**32 - 30, what="before 2^32")                           # far beyond the second threshold
    assert r["counts"][0] == chosen.size and set(r["cols"]["count"].tolist()) == {2}
    r = check(H, 2**32 + 196, form="host", what="across 2^32")           # 226 ms: the third threshold is 225
    assert r["counts"][0] == chosen.size and set(r["cols"]["waited"].tolist()) == {226}
    H.close()
    return H.stats


def cap_cuts(hip_lib, oracle_lib):
    chosen = np.arange(0, G3, 30)                                          # 100 waits over three tiles
    H = waiting_table(hip_lib, oracle_lib, G3, chosen)
    check(H, 0, what="arm")
    r = check(H, 500, cap=0, form="host", null_cols=True, what="counts only")
    assert r["counts"] == (100, 0, 100, 0)
    r = check(H, 500, cap=0, form="dev", null_cols=True, what="counts only")
    assert r["counts"] == (100, 0, 100, 0)                                 # the call before changed nothing
    r = check(H, 500, cap=30, what="cut")
    assert r["counts"] == (100, 0, 100, 30) and r["groups"][r["hits"]].tolist() == chosen[:30].tolist()
    r = check(H, 500, cap=69, form="host", what="the next ones")
    assert r["counts"] == (70, 0, 100, 69) and r["groups"][r["hits"]].tolist() == chosen[30:99].tolist()
    r = check(H, 501, cap=70, what="the last one")
    assert r["counts"] == (1, 0, 100, 1) and r["cols"]["waited"].tolist() == [501]
    r = check(H, 502, cap=G3, form="host", what="nothing left")
    assert r["counts"] == (0, 0, 100, 0)
    H.close()
    return H.stats


def peek_twice(hip_lib, oracle_lib):
    n = T + 1
    chosen = np.arange(1, n, 4)
    H = waiting_table(hip_lib, oracle_lib, n, chosen)
    r0 = peek_all(H, 0, what="a peek arms nothing")
    assert r0["counts"] == (0, 0, chosen.size, 0) and not H.T.key.any()
    check(H, 0, what="arm")
    a = peek_all(H, 300, cap=50, what="first peek")
    b = peek_all(H, 300, cap=50, what="second peek")
    r = check(H, 300, cap=50, what="the real sweep")
    for x in (a, b):
        assert x["counts"][:3] == r["counts"][:3] and x["counts"][3] == 0
        assert all(x["cols"][c].tolist() == r["cols"][c].tolist() for c in M.OUT_COLS)
    assert r["counts"] == (chosen.size, 0, chosen.size, 50)
    H.close()
    return H.stats


def listed_sweep(hip_lib, oracle_lib):
    chosen = np.arange(0, G3, 2)
    H = waiting_table(hip_lib, oracle_lib, G3, chosen)
    dead = np.arange(10, G3, 97, dtype=np.int32)
    H.do(lambda e: e.retire_groups(dead, RETIRE_KILL))
    rng = np.random.default_rng(5)
    lst = rng.permutation(np.arange(0, G3, 3))
    lst = np.concatenate([lst[:500], [-1, G3, G3 + 5, -2**31, 2**31 - 1], lst[500:]]).astype(np.int32)
    assert lst.size % 64 and np.unique(lst).size == lst.size and np.isin(dead, lst).any()
    r = check(H, 40, gidx=lst, what="listed, arm")
    assert r["counts"][1] == 5 + np.isin(dead, lst).sum() and r["counts"][2] > 300
    H.do(lambda e: decide(e, np.setdiff1d(chosen[::7], dead), 1, H.k))    # some stop waiting
    r = peek_all(H, 141, gidx=lst, what="listed")
    r = check(H, 141, cap=200, gidx=lst, what="listed, cut")
    hit = r["groups"][r["hits"]].tolist()
    assert len(hit) == 200 and hit == [g for g in lst.tolist() if g in set(hit)]       # in entry order
    r = check(H, 141, form="host", gidx=lst, what="listed, the rest")
    assert r["counts"][0] > 50
    r = check(H, 150, form="host", what="the whole table: the unlisted ones are armed only now")
    assert r["counts"][0] == 0 and r["armed"].size > 500
    H.close()
    return H.stats


def shapes(hip_lib, oracle_lib, kmax, k, window):
    n = T + 1
    chosen = np.arange(0, n, 3, dtype=np.int32)
    others = np.setdiff1d(np.arange(n), chosen)[::2].astype(np.int32)
    H = History(hip_lib, oracle_lib, n, kmax=kmax, k=k, window=window)
    H.do(lambda e: whole_round(e, others, k))                              # slot 1 decided and committed: the head of line moves
    H.do(lambda e: propose(e, chosen))
    check(H, 5, what="arm")
    H.do(lambda e: propose(e, others))                                     # slot 2
    r = check(H, 106, form="host", what=f"K={k} W={window}")
    assert set(r["cols"]["slot"].tolist()) == {1}
    assert r["counts"] == (chosen.size, 0, chosen.size + others.size, chosen.size)
    if k > 1:
        H.do(lambda e: replies(e, chosen[::2], 1, [ME + 1]))
    r = check(H, 257, cap=100, what=f"K={k} W={window}")
    assert r["counts"][0] == chosen.size + others.size and r["counts"][3] == 100
    if k > 1:
        assert (r["cols"]["heard"][np.isin(r["groups"][r["hits"]], chosen[::2])] != 0).all()
    r = check(H, 257, form="host", what=f"K={k} W={window}, the rest")
    H.close()
    return H.stats


def many_tiles(hip_lib, oracle_lib, n):
    """one due group in a thousand among waiting ones: the due ones are armed 60 ms before the others"""
    allg = np.arange(n, dtype=np.int32)
    due = allg[::1000]
    late = allg[1::1000]
    H = waiting_table(hip_lib, oracle_lib, n, np.union1d(due, late))
    r = check(H, 0, gidx=due, what="arm the due ones")
    assert r["counts"] == (0, 0, due.size, 0)
    r = check(H, 60, form="host", what="arm the others")
    assert r["counts"] == (0, 0, due.size + late.size, 0) and r["armed"].size == late.size
    if H.eh is not None:
        H.eh.profile(2)
    r = check(H, 101, cap=0, null_cols=True, what="counts only")
    prof0 = {k_: v[0] for k_, v in H.eh.profile_read().items()} if H.eh is not None else None
    r = check(H, 101, cap=due.size + 7, what="one in a thousand")
    assert r["counts"] == (due.size, 0, due.size + late.size, due.size) and r["groups"][r["hits"]].tolist() == due.tolist()
    if H.eh is not None:
        prof = {k_: v[0] for k_, v in H.eh.profile_read().items()}
        H.eh.profile(0)
        assert prof0 == {"k_rtx_tile": 1, "k_rtx_offsets": 1}, prof0        # cap == 0: nothing to move
        assert prof == {"k_rtx_tile": 2, "k_rtx_offsets": 2, "k_rtx_move": 1}, prof
    H.close()
    return H.stats


def host_twin(hip_lib, oracle_lib):
    n = G3
    chosen = np.arange(0, n, 5)
    H = waiting_table(hip_lib, oracle_lib, n, chosen)
    check(H, 0, form="host_alloc", what="arm")
    for form in ("host", "host_alloc", "dev"):
        peek_all(H, 900, what="before " + form)
    for j, form in enumerate(("host", "host_alloc", "dev")):
        r = check(H, 900 + j, cap=200, form=form, what="twin")
        assert r["counts"] == (chosen.size - 200 * j, 0, chosen.size, 200)
    H.close()
    return H.stats


def end_to_end(hip_lib, oracle_lib):
    """the ACCEPTs of 30 groups are lost; the sweep, once due, returns exactly those, and sending them again decides"""
    n = G3
    allg = np.arange(n, dtype=np.int32)
    lost = allg[50::100]
    rest = np.setdiff1d(allg, lost)
    H = History(hip_lib, oracle_lib, n)
    sl, bn, bc, med, st = propose(H.eo, allg)
    if H.eh is not None:
        assert all((x == y).all() for x, y in zip(propose(H.eh, allg), (sl, bn, bc, med, st)))

    def deliver(e, g, slot, bnum, bcoord, median):
        """the ACCEPT reaches this node's acceptor, and a majority of replies comes back"""
        out, _ = e.accept(g, bnum, bcoord, slot, median)
        assert (out[4] == S_OK).all()
        assert replies(e, g, slot, majority(H.k)) == g.size
    H.do(lambda e: deliver(e, rest, sl[rest], bn[rest], bc[rest], med[rest]))
    r = check(H, 7, what="arm")
    assert r["counts"] == (0, 0, lost.size, 0)
    r = check(H, 107, form="host", what="not yet")
    assert r["counts"][0] == 0
    r = check(H, 108, what="due")
    c = r["cols"]
    assert c["gidx"].tolist() == lost.tolist() and r["counts"] == (30, 0, 30, 30)
    assert (c["slot"] == sl[lost]).all() and (c["bnum"] == bn[lost]).all() and (c["bcoord"] == bc[lost]).all()
    assert (c["median_cp"] == med[lost]).all() and (c["poke"] == M.POKE_ACCEPT).all()
    H.do(lambda e: deliver(e, c["gidx"], c["slot"], c["bnum"], c["bcoord"], c["median_cp"]))
    r = check(H, 300, form="host", what="decided")
    assert r["counts"] == (0, 0, 0, 0) and not H.T.key.any()
    H.close()
    return H.stats
