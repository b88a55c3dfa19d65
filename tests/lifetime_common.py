"""What one call leaves behind for a later one: drivers of tests/test_lifetime_gpu.py (engine against oracle) and
tests/test_lifetime_model.py (the same drivers oracle against oracle, on the CPU).

The engine does not clear its scratch between calls: the kernels tag words with a per-call EPOCH and compare tags, and a
few arrival / ticket counters only ever count up.  Two switches, read when the HIP engine is created, bring the wrap
branches and the counters' 2^31 / 2^32 boundaries within a test's reach:

  GPX_TEST_EPOCH_WRAP=n     X.epoch, one_epoch, small_epoch and w_epoch take their wrap branch on reaching n: the epoch
                            values of an engine are 1 .. n-1, round and round
  GPX_TEST_COUNTER_BASE=v   gx_arrive (with the sixteen device arrival words) and small_drawn (with *small_draw) start at v

The oracle has no epochs and ignores both.  Everything here goes through the C-ABI; the host-side dispatch arithmetic
that decides which kernel consumes which counter (gpx_engine.hip: xchg_ctl, gpx_accept_batch_dev, propose_dev_impl) is
restated below and asserted against gpx_profile_read by the GPU tests, so that neither can drift unnoticed."""
import numpy as np

from gigapaxos_amd import (Engine, hri_create, streams, S_OK, S_UNORDERED, ORDERED_PROPOSE, ORDERED_ACCEPT,
                           ORDERED_COMMIT, C_HASVALUE)
from gigapaxos_amd._abi import Decisions, ExecRuns, GpxError

SWITCHES = ("GPX_TEST_EPOCH_WRAP", "GPX_TEST_COUNTER_BASE")
MEMBERS = [100, 101, 102]
MASK_PAC = ORDERED_PROPOSE | ORDERED_ACCEPT | ORDERED_COMMIT
BATCH_OPS = ("propose", "accept", "accept_reply", "commit", "prepare")   # the fuzz's entry points that open a call epoch (begin_front)

# ---- gpx_engine.hip restated -------------------------------------------------------------------------------------------
GPX_DBLOCK = 256            # records per workgroup of k_ac_pers / k_ac_one / k_propose_pers / k_propose_one
GPX_DCHUNK = 1024           # records per chunk (= workgroup) of k_ac_small
GPX_GX_LINES = 16           # grid_exchange's arrival counters: the grid is padded to a multiple of them
PERS_MAX_CHUNKS = dict(propose=128, accept=192, commit=192)   # pers_max_chunks[0], [1], [1]
GPX_SMALL_DIRECT_MAX_N = 65536


def epoch_values(calls, wrap):
    """The epoch of each of `calls` consecutive launches of an engine under GPX_TEST_EPOCH_WRAP=wrap: 1 .. wrap-1."""
    return [i % (wrap - 1) + 1 for i in range(calls)]


def wraps(calls, wrap):
    """How often the wrap branch ran during `calls` launches (the first is launch number `wrap`)."""
    return 0 if calls < wrap else 1 + (calls - wrap) // (wrap - 1)


def exchange_increment(op, n):
    """gx_arrive's increment of an ordered, promised call of n records that may take the one-launch form (one engine on
    the device: two workgroups per CU hold every such grid), or 0 where the call takes check + work kernel instead."""
    nch = (n + GPX_DBLOCK - 1) // GPX_DBLOCK
    if nch > PERS_MAX_CHUNKS[op]:
        return 0
    return (max(nch, 1) + GPX_GX_LINES - 1) // GPX_GX_LINES


def small_chunks(n):
    """small_drawn's increment of a k_ac_small launch over n records."""
    return (n + GPX_DCHUNK - 1) // GPX_DCHUNK


def ordered_kernel(op, n, lazy, one_launch=True):
    """The work kernel of an ordered, PROMISED batch through the device-pointer calls (lazy: GPX_LAZY_OUTPUTS set)."""
    if op == "propose":
        return "k_propose_pers" if one_launch and exchange_increment(op, n) else "k_propose_one"
    if n <= GPX_SMALL_DIRECT_MAX_N and not lazy:
        return "k_ac_small"
    return "k_ac_pers" if one_launch and exchange_increment(op, n) else "k_ac_one"


def crossing(base, increments, boundary):
    """Launches that started below / at or above `boundary` when a 32-bit cumulative counter starts at `base` and grows
    by `increments` (zeros: launches that do not touch it), and whether one launch straddles the boundary."""
    v, before, after, straddle = base, 0, 0, False
    for inc in increments:
        if inc == 0:
            continue
        if v < boundary:
            before += 1
            straddle |= v + inc > boundary
        else:
            after += 1
        v += inc
    return before, after, straddle, v


# ---- the switches ------------------------------------------------------------------------------------------------------
def assert_switch_is_read(monkeypatch, lib, name):
    """The library reads THIS spelling of the switch: a value that cannot be meant makes gpx_engine_create refuse, so a
    misspelt name fails the test instead of running the 2^32 path green.  This shows that the name is read, NOT that the
    wrap branch runs: an epoch wrap has, by design, no effect a caller could see, and a library that parsed the value and
    then lost it would pass every case here.  That the branches run with the clears they hold is shown by the mutant
    builds of profiles/r10_lifetime_tests.txt (a forgotten clear fails these tests, which it could not if the branch
    were not taken).  GPX_TEST_COUNTER_BASE does have an effect that surfaces: the host's targets and the device's
    arrival words must both start at the base - with only one of them moved, grid_exchange's pollers wait for arrivals
    2^31 away, give up, and the call or gpx_engine_sync answers GPX_EDEVICE; the chunk draw of k_ac_small would hand out
    chunks beyond the batch and leave records unanswered, which the comparison with the oracle sees."""
    import pytest
    monkeypatch.setenv(name, "not-a-number")
    with pytest.raises(GpxError):
        Engine(lib, 100, 64, kmax=3, window=8, max_batch=1024)
    monkeypatch.delenv(name)


class Counted:
    """An engine and the number of its batch calls (those that open a call epoch: n > 0)."""

    def __init__(self, e):
        self._e = e
        self.calls = {op: 0 for op in BATCH_OPS}
        self.sizes = []   # (op, n) of every batch call, in order

    def __getattr__(self, name):
        return getattr(self._e, name)

    def _count(self, op, g):
        n = int(np.asarray(g).shape[0])
        if n:
            self.calls[op] += 1
            self.sizes.append((op, n))

    def propose(self, g, *a, **kw):
        self._count("propose", g)
        return self._e.propose(g, *a, **kw)

    def accept(self, g, *a, **kw):
        self._count("accept", g)
        return self._e.accept(g, *a, **kw)

    def accept_reply(self, g, *a, **kw):
        self._count("accept_reply", g)
        return self._e.accept_reply(g, *a, **kw)

    def commit(self, g, *a, **kw):
        self._count("commit", g)
        return self._e.commit(g, *a, **kw)

    def prepare(self, g, *a, **kw):
        self._count("prepare", g)
        return self._e.prepare(g, *a, **kw)

    @property
    def total(self):
        return sum(self.calls.values())


def run_cell_counted(lib_a, lib_b, c, ordered, steps=None):
    """geometry_common.run_cell with engine a's batch calls counted and its launch profile returned whole:
    (statuses seen, Counted, {kernel: launches})."""
    from tests.geometry_common import run_cell
    return run_cell(lib_a, lib_b, c, ordered=ordered, profile=True, steps=steps, counted=Counted)


# kernels that read a word tagged with the call epoch (*X.unsorted, rec_tag, D.mark, A.ref[3]): at least one of them
# runs in every ACCEPT, COMMIT and accept-reply call
EPOCH_READERS = ("k_ac_small", "k_order_check", "k_emit_runs_direct", "k_emit_runs16", "k_emit_runs", "k_emit_dec16",
                 "k_ar_tiny", "k_runs_check", "k_ar_runs", "k_ar_runs_pers", "k_one_count", "k_ac_pers", "k_ac_one")
# ... and with the proposals' work kernels: at least one of these runs in EVERY batch call
CALL_KERNELS = EPOCH_READERS + ("k_propose_pers", "k_propose_one", "k_propose_small", "k_propose_direct")


class ProfiledEngines:
    """Drivers of other test modules create and close their engines themselves.  While this is installed every HIP
    engine has its launch profile switched on at creation and read at close(): `profiles` holds one {kernel: launches}
    per closed engine that launched anything, so that a leg which reuses such a driver can still assert how many calls
    ran under its wrap."""

    def __init__(self, monkeypatch, lib):
        self.profiles = []
        init0, close0, me = Engine.__init__, Engine.close, self

        def init(eng, lib_, *a, **kw):
            init0(eng, lib_, *a, **kw)
            if lib_ is lib:
                eng.profile(2)

        def close(eng, *a, **kw):
            if eng.h and eng.lib is lib:
                prof = {k: v[0] for k, v in eng.profile_read().items()}
                if prof:
                    me.profiles.append(prof)
            return close0(eng, *a, **kw)
        monkeypatch.setattr(Engine, "__init__", init)
        monkeypatch.setattr(Engine, "close", close)

    def calls(self):
        """Per engine: launches of the kernels of which every batch call runs at least one."""
        return [sum(p.get(k, 0) for k in CALL_KERNELS) for p in self.profiles]


# leg (a): the cell of each back end in the default run, and the wrap it runs under (big-accept-commit makes a dozen calls)
CELL_WRAP = {"partition-k3-w4": 5, "tiles-k3-w8": 5, "runs-k3-w4": 5, "big-accept-commit-k3-w8": 3, "wide-s11-w8": 5}


def cell_steps(name, wrap):
    """Steps of a cell's fuzz under GPX_TEST_EPOCH_WRAP=wrap: its own (CELLS stays as it is), except the cell of the big
    ACCEPT / COMMIT batches: its dozen steps are a dozen batch calls, of which seven or eight are ACCEPT, COMMIT or
    accept-reply calls (the ones whose kernels read the tagged words) - a copy with more steps serves there."""
    if name == "big-accept-commit-k3-w8":
        return 30 if wrap <= 5 else 80
    return None


# ---- the device-pointer calls behind the host calls' signatures ----------------------------------------------------------
class DevEngine:
    """A HIP engine driven through the *_dev calls (torch tensors), answering like Engine's host calls, so that one
    driver serves the engine (GPU) and a second oracle (CPU model).  gpx_compact_last_dev follows EVERY call - the last
    before a wrap and the first after it included; `raw` keeps the count word as the call itself left it (negative:
    the batch was irregular and its outputs were parked)."""

    def __init__(self, e):
        import torch
        self.e, self.t = e, torch
        self.raw = None
        self.kernels = []   # per call: the kernels the engine's profile names
        self.launches = {}  # kernel -> launches over all calls

    def __getattr__(self, name):
        return getattr(self.e, name)

    def _dev(self, a, dtype=None):
        return self.t.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()

    def _z(self, n, u8=False):
        return self.t.zeros(max(n, 1), dtype=self.t.uint8 if u8 else self.t.int32, device="cuda")

    def _begin(self):
        """torch's fills and copies run on torch's stream, the engine's kernels on its own: the first must be done"""
        self.t.cuda.synchronize()
        self.e.profile(2)

    def _finish(self, word):
        self.e.sync()
        self.raw = int(word.item()) if word is not None else None
        self.e.compact_last_dev()
        self.e.sync()
        prof = self.e.profile_read()
        self.kernels.append(set(prof))
        for k, v in prof.items():
            self.launches[k] = self.launches.get(k, 0) + v[0]
        return int(word.item()) if word is not None else None

    def propose(self, g, is_stop=None):
        g = np.ascontiguousarray(g, np.int32)
        n = g.shape[0]
        o = [self._z(n) for _ in range(4)] + [self._z(n, True)]
        stop = self._dev(is_stop, np.uint8) if is_stop is not None else None
        gd = self._dev(g)
        self._begin()
        self.e.call_dev("propose_batch", n, gd.data_ptr(), stop.data_ptr() if stop is not None else 0,
                        *[t.data_ptr() for t in o])
        self._finish(None)
        return tuple(t.cpu().numpy()[:n] for t in o)

    def accept(self, g, bnum, bcoord, slot, median, a_flags=None):
        n = np.asarray(g).shape[0]
        cols = [self._dev(c, np.int32) for c in (g, bnum, bcoord, slot, median)]
        fl = self._dev(a_flags, np.uint8) if a_flags is not None else self._z(n, True)
        o = [self._z(n) for _ in range(3)] + [self._z(n, True), self._z(n, True)] + [self._z(n) for _ in range(3)] + [self._z(1)]
        self._begin()
        self.e.call_dev("accept_batch", n, *[c.data_ptr() for c in cols], fl.data_ptr(), *[t.data_ptr() for t in o])
        m = self._finish(o[-1])
        h = [t.cpu().numpy() for t in o]
        return tuple(x[:n] for x in h[:5]), ExecRuns(h[5][:m], h[6][:m], h[7][:m])

    def commit(self, g, bnum, bcoord, slot, median, c_kind=None):
        n = np.asarray(g).shape[0]
        cols = [self._dev(c, np.int32) for c in (g, bnum, bcoord, slot, median)]
        kind = self._dev(c_kind, np.uint8) if c_kind is not None else self._z(n, True)
        o = [self._z(n, True)] + [self._z(n) for _ in range(3)] + [self._z(1)]
        self._begin()
        self.e.call_dev("commit_batch", n, *[c.data_ptr() for c in cols], kind.data_ptr(), *[t.data_ptr() for t in o])
        m = self._finish(o[-1])
        h = [t.cpu().numpy() for t in o]
        return h[0][:n], ExecRuns(h[1][:m], h[2][:m], h[3][:m])

    def accept_reply(self, g, bnum, bcoord, slot, acceptor, max_cp, unaligned=False, status=True):
        """unaligned: every input column 4 bytes off a 16-byte boundary (the partition front end takes the call);
        status False: no status column (NULL) - the answer's status is then None."""
        n = np.asarray(g).shape[0]
        t = self.t
        if unaligned:
            cols = []
            for c in (g, bnum, bcoord, slot, acceptor, max_cp):
                p = t.zeros(n + 8, dtype=t.int32, device="cuda")
                v = p[1:n + 1]
                v.copy_(t.from_numpy(np.ascontiguousarray(c, np.int32)))
                assert v.data_ptr() % 16 != 0
                cols.append(v)
        else:
            cols = [self._dev(c, np.int32) for c in (g, bnum, bcoord, slot, acceptor, max_cp)]
        d = [self._z(n) for _ in range(5)] + [self._z(n, True)]
        no, st = self._z(1), self._z(n, True)
        self._begin()
        self.e.call_dev("accept_reply_batch", n, *[c.data_ptr() for c in cols], *[x.data_ptr() for x in d], no.data_ptr(),
                        st.data_ptr() if status else 0)
        m = self._finish(no)
        h = [x.cpu().numpy()[:m] for x in d]
        return Decisions(h[0], h[1], h[2], h[3], h[4], h[5], st.cpu().numpy()[:n] if status else None)


# ---- leg (b) / (c) / (d): a script of ordered batches, irregular next to regular -----------------------------------------
# One step = one engine call on a population of groups that move together (`s`: every group has executed the slots
# below s).  REGULAR steps are the batches the work kernels finish alone: a proposal batch; ACCEPTs that release no
# commit; COMMITs that execute exactly one run per record.  IRREGULAR steps write D.mark, tags and - when the promise is
# broken - the verdict word:
#   PH   placeholders (commits without a value) for slot s: nothing executes
#   AR   the ACCEPTs of slot s release those commits                                  (s += 1)
#   C3   COMMIT of slot s+1 for every third group and of slot s for the others: a third executes nothing
#   AX   an ACCEPT batch that breaks the promise (a descent in the middle): refused from there on
#   CX   a COMMIT batch of slot s that breaks the promise: the groups before the descent execute s
#   PX   a PROPOSE batch with a repeated group (the strict promise): refused from there on
# and the regular steps that bring the population level again:
#   C3b  slot s for that third (two slots execute per commit: still one run per record), C3c  slot s+1 for the others (s += 2)
#   CXb  slot s for the groups from the descent on                                     (s += 1)
#   P    proposals,  A  ACCEPTs of slot s,  C  COMMITs of slot s                       (s += 1)
IRREGULAR = {"PH", "AR", "C3", "AX", "CX", "PX"}
BLOCKS = [["PH", "AR", "C3", "AX"], ["C3b", "C3c", "P", "C"], ["PH", "AR", "CX", "PX"], ["CXb", "P", "A", "C"]]


ORDERED_CALLS = 24   # leg (b): six blocks, five wraps under n = 5
SMALL_BASE = (1 << 32) - 37


def small_plan():
    """Leg (c): a population of 1,000 groups (one chunk per launch) and one of 65,536 (64 chunks).  Five launches of one
    chunk, then the large population's first launch draws chunks 2^32 - 32 .. 2^32 + 31."""
    pops = [Population(0, 1000), Population(1000, 65536)]
    return pops, [0] * 5 + [1, 0] * 10, 1000 + 65536


def small_increments(log):
    """small_drawn's increment per call: k_ac_small runs in every ACCEPT / COMMIT call of at most 65,536 records."""
    return [small_chunks(x["n"]) if x["op"] in ("accept", "commit") else 0 for x in log]


def exchange_plan():
    """Leg (d): one engine, ordered batches of 2,500 .. 65,000 records (test_many_engines_gpu.py's sizes).  Four one-launch
    calls of one increment each, then one of four: the counters start five below the boundary and pass it inside that
    launch."""
    sizes = [2_500, 13_000, 40_000, 65_000, 30_000]
    lo = np.concatenate([[0], np.cumsum(sizes)])
    pops = [Population(int(lo[i]), m) for i, m in enumerate(sizes)]
    return pops, [0, 0, 0, 0, 1] + [2, 3, 4, 0, 1] * 7, int(lo[-1])


def exchange_increments(log):
    return [exchange_increment(x["op"], x["n"]) for x in log]


def ordered_kinds(calls):
    """The step kinds of a script of `calls` calls: blocks of four irregular and four regular steps in turn, so that with
    GPX_TEST_EPOCH_WRAP=5 (epoch values 1 .. 4) every epoch value meets an irregular batch and, one cycle later, a
    regular one - and the other way round."""
    out = []
    while len(out) < calls:
        out += BLOCKS[(len(out) // 4) % len(BLOCKS)]
    return out[:calls]


def pairing(irregular, wrap):
    """Per epoch value: has it seen irregular -> regular and regular -> irregular one cycle apart?  `irregular`: one
    flag per call of an engine whose every call draws an epoch."""
    cyc = wrap - 1
    ir, ri = set(), set()
    for i in range(len(irregular) - cyc):
        v = i % cyc + 1
        if irregular[i] and not irregular[i + cyc]:
            ir.add(v)
        if not irregular[i] and irregular[i + cyc]:
            ri.add(v)
    return ir, ri


class Population:
    """Groups lo .. lo+m-1 of a table and the script's state for them."""

    def __init__(self, lo, m):
        self.g = np.arange(lo, lo + m, dtype=np.int32)
        self.m, self.s, self.v = m, 1, m // 2 + 3
        self.i = 0   # position in its own kind sequence

    def batch(self, kind):
        """(op, args of Engine.<op>, index of the first violation or None) of the next step; advances the state."""
        g, m, s, v = self.g, self.m, self.s, self.v
        z, bc = np.zeros(m, np.int32), np.full(m, 100, np.int32)
        hv = np.full(m, C_HASVALUE, np.uint8)
        third = (np.arange(m) % 3) == 0
        full = lambda x: np.full(m, x, np.int32)  # noqa: E731
        gb = g.copy()
        gb[v] = gb[v - 1] - 7
        if kind == "P":
            return "propose", (g,), None
        if kind == "PX":
            q = min(m, 2000)
            return "propose", (np.concatenate([g[:q // 2], g[q // 2 - 1:q]]),), q // 2
        if kind in ("A", "AR"):
            if kind == "AR":
                self.s += 1
            return "accept", (g, z, bc, full(s), z), None
        if kind == "AX":
            return "accept", (gb, z, bc, full(s), z), v
        if kind == "C":
            self.s += 1
            return "commit", (g, z, bc, full(s), z, hv), None
        if kind == "PH":
            return "commit", (g, z, bc, full(s), z, np.zeros(m, np.uint8)), None
        if kind == "C3":
            return "commit", (g, z, bc, np.where(third, s + 1, s).astype(np.int32), z, hv), None
        if kind == "C3b":
            k = int(third.sum())
            return "commit", (g[third], z[:k], bc[:k], np.full(k, s, np.int32), z[:k], hv[:k]), None
        if kind == "C3c":
            k = int((~third).sum())
            self.s += 2
            return "commit", (g[~third], z[:k], bc[:k], np.full(k, s + 1, np.int32), z[:k], hv[:k]), None
        if kind == "CX":
            return "commit", (gb, z, bc, full(s), z, hv), v
        if kind == "CXb":
            k = m - v
            self.s += 1
            return "commit", (g[v:], z[:k], bc[:k], np.full(k, s, np.int32), z[:k], hv[:k]), None
        raise ValueError(kind)


def is_irregular(op, n, answer):
    """What the ORACLE's answer says about a step: did the batch break its promise, release a commit (ACCEPT) or fail
    to execute exactly one run per record (COMMIT)?  Proposals: only a broken promise."""
    if op == "propose":
        return bool((answer[4] == S_UNORDERED).any())
    st, runs = (answer[0][4], answer[1]) if op == "accept" else answer
    if (st == S_UNORDERED).any():
        return True
    return runs.gidx.shape[0] != (0 if op == "accept" else n)


def same_answer(op, a, b, what):
    if op == "propose":
        for x, y in zip(a, b):
            assert x.tolist() == y.tolist(), what
        return
    (sa, xa), (sb, xb) = a, b
    if op == "accept":
        for x, y in zip(sa, sb):
            assert x.tolist() == y.tolist(), what
    else:
        assert sa.tolist() == sb.tolist(), what
    assert xa.as_tuple_array().tolist() == xb.as_tuple_array().tolist(), what + " (execution runs)"


def make_ordered_pair(lib_a, lib_b, G, mask_a, mask_b, max_batch=None):
    ea = Engine(lib_a, 100, G, kmax=3, window=8, max_batch=max_batch or G + 64)
    eb = Engine(lib_b, 100, G, kmax=3, window=8, max_batch=max_batch or G + 64)
    mem = np.tile(np.array(MEMBERS, np.int32), (G, 1))
    for e, mask in ((ea, mask_a), (eb, mask_b)):
        assert (e.create_groups(np.arange(G), mem, 3, hri_create(G, 3, 100)) == S_OK).all()
        e.set_ordered_batches(mask)
    return ea, eb


def run_ordered_script(ea, eb, pops, schedule, promised=True):
    """Applies the script to engine a (an Engine, a DevEngine or a second oracle) and to the oracle b.  `schedule`: the
    population index of each call; each population follows ordered_kinds on its own.  Every answer is compared; a
    broken promise must be refused from its first violation on, nothing before it.  Returns one record per call:
    dict(op, n, kind, irregular (by the oracle's answer), pop)."""
    log = []
    kinds = ordered_kinds(len(schedule))
    for c, p in enumerate(schedule):
        pop = pops[p]
        kind = kinds[pop.i]
        pop.i += 1
        op, args, first = pop.batch(kind)
        n = args[0].shape[0]
        a, b = getattr(ea, op)(*args), getattr(eb, op)(*args)
        what = f"call {c} ({kind}, {op} of {n} records, population {p})"
        same_answer(op, a, b, what)
        if first is not None and promised:
            st = b[4] if op == "propose" else (b[0][4] if op == "accept" else b[0])
            assert (st[first:] == S_UNORDERED).all() and not (st[:first] == S_UNORDERED).any(), what
        irr = is_irregular(op, n, b)
        if promised:
            assert irr == (kind in IRREGULAR), (what, irr)
        log.append(dict(op=op, n=n, kind=kind, irregular=irr, pop=p, raw=getattr(ea, "raw", None)))
    return log


def assert_same_rows(ea, eb, G, seed=5):
    from tests.parity_common import assert_same_state
    g = np.arange(G, dtype=np.int32)
    assert ea.snapshot(g)[0].tobytes() == eb.snapshot(g)[0].tobytes()
    assert_same_state(ea, eb, np.random.default_rng(seed).integers(0, G, 100))
    assert ea.counters() == eb.counters()


# ---- leg (b), the runs call: its one-launch form draws from the same one_epoch ------------------------------------------
# P<x> proposes slot x everywhere; R<x> brings every acceptor's votes for it as three ascending runs (regular: every
# group decides); RL<x> loses a fifth of them (irregular); RF<x> brings them all again (irregular: most groups have
# decided already); RX breaks the promise (a shuffled batch: refused whole).  Blocks of four regular / four irregular calls.
RUNS_SCRIPT = ["P1", "R1", "P2", "P3", "RL2", "RF2", "RL3", "RF3",
               "P4", "R4", "P5", "P6", "RX", "RL5", "RF5", "RX",
               "R6", "P7", "R7", "P8", "RL8", "RX", "RF8", "RX"]


def run_runs_script(ea, eb, G, seed=7):
    """Returns per call dict(kind, irregular, n, raw).  Engine a's accept_reply answers are the oracle's; RX is refused
    whole."""
    rng = np.random.default_rng(seed)
    g = np.arange(G, dtype=np.int32)
    log = []
    for c, step in enumerate(RUNS_SCRIPT):
        if step == "RX":
            kind, slot = "RX", 1
        elif step[:2] in ("RL", "RF"):
            kind, slot = step[:2], int(step[2:])
        else:
            kind, slot = step[0], int(step[1:])
        what = f"call {c} ({step})"
        if kind == "P":
            a, b = ea.propose(g), eb.propose(g)
            same_answer("propose", a, b, what)
            assert (b[0] == slot).all() and (b[4] == S_OK).all(), what
            log.append(dict(kind=kind, irregular=False, n=G, raw=None))
            continue
        cols = [x.copy() for x in streams.vote_round_runs(G, MEMBERS, 0, 100, config_id=3)]
        cols[3][:] = slot
        cols[5][:] = slot - 1
        if kind == "RL":
            keep = rng.random(cols[0].shape[0]) > 0.2
            cols = [np.ascontiguousarray(x[keep]) for x in cols]
        if kind == "RX":
            order = rng.permutation(cols[0].shape[0])
            cols = [np.ascontiguousarray(x[order]) for x in cols]
        da, db = ea.accept_reply(*cols), eb.accept_reply(*cols)
        assert da.as_tuple_array().tolist() == db.as_tuple_array().tolist(), what
        assert da.status.tolist() == db.status.tolist(), what
        if kind == "RX":
            assert (db.status == S_UNORDERED).all() and db.gidx.shape[0] == 0, what
        irr = db.gidx.shape[0] != G
        assert irr == (kind != "R"), (what, db.gidx.shape[0])
        log.append(dict(kind=kind, irregular=irr, n=cols[0].shape[0], raw=getattr(ea, "raw", None)))
    return log


# ---- leg (g): accept-reply calls of every shape on one engine -------------------------------------------------------------
FRONT_ENDS = ("tiny", "tiles", "partition", "runs")
# shape -> front end
SHAPES = {
    "tiny": "tiny",              # at most 1,024 votes: k_ar_tiny
    "few tiles": "tiles",        # a few 4,096-vote tiles
    "many tiles": "tiles",       # every group's votes, three times over: hundreds of tiles
    "wide": "tiles",             # only groups out of lock-step: every tile goes wide
    "escapes": "tiles",          # groups in lock-step and a few that are not: narrow tiles, escaped votes
    "unaligned": "partition",    # device columns 4 bytes off: the partition front end
    "runs": "runs",              # the acceptors' ascending runs under GPX_TRY_REPLY_RUNS
    "shuffled hint": "tiles",    # a shuffled call under the same hint: the check, then the tiles
    "no status": "tiles",        # status == NULL
    "lost acceptor": "tiles",    # two votes per group: the in-place prediction (three per output) misses
    "mix": "tiles",              # duplicates, other ballots, non-members, far slots
}


def alternation_sequence(seed, calls=44):
    """Shapes of leg (g)'s accept-reply calls: first a walk through every ordered pair of front ends (an Euler circuit
    of the complete digraph on four nodes, loops included: 17 calls, consecutive, nothing in between), the shape of each
    drawn among those of its front end; then seeded draws from all shapes.  Checked before an engine is touched."""
    rng = np.random.default_rng(seed)
    by_fe = {fe: [s for s, f in SHAPES.items() if f == fe] for fe in FRONT_ENDS}
    # Hierholzer on K4 with loops
    out = {a: list(rng.permutation(len(FRONT_ENDS))) for a in range(4)}
    stack, circuit = [0], []
    while stack:
        a = stack[-1]
        if out[a]:
            stack.append(int(out[a].pop()))
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    seq = [str(rng.choice(by_fe[FRONT_ENDS[a]])) for a in circuit]
    names = list(SHAPES)
    # every shape at least once, then draws
    rest = [s for s in names if s not in seq]
    seq += [str(x) for x in rng.permutation(rest)]
    while len(seq) < calls:
        seq.append(str(rng.choice(names)))
    pairs = {(SHAPES[a], SHAPES[b]) for a, b in zip(seq[:17], seq[1:17])}
    assert len(circuit) == 17 and len(pairs) == 16, (circuit, sorted(pairs))
    assert set(seq) == set(names)
    return seq


def lockstep_rows(G, rng):
    """Hot-restore rows: the odd groups at slots of their own (test_tiles_gpu.py), the even ones at slot 1."""
    rows = hri_create(G, 3, 100)
    odd = (np.arange(G) % 2) == 1
    base = rng.integers(1000, 2_000_000, G).astype(np.int32)
    rows["acc_slot"][odd] = base[odd]
    rows["acc_gc_slot"][odd] = base[odd] - 1
    rows["next_proposal_slot"][odd] = base[odd]
    rows["node_slots"][odd, :3] = (base[odd] - 1)[:, None]
    return rows


def shape_votes(shape, G, slot_of, rng):
    """Six vote columns of one call of `shape`; slot_of[g] = the slot group g's votes are for."""
    even, odd = np.arange(0, G, 2, dtype=np.int32), np.arange(1, G, 2, dtype=np.int32)
    reps, members, shuffle = 1, MEMBERS, True
    if shape == "tiny":
        sel = rng.choice(G, 300, replace=False)
    elif shape == "few tiles":
        sel = rng.choice(even, 3300, replace=False)
    elif shape == "many tiles":  # hundreds of 12,288-vote tiles, one round of them on the chip
        sel = np.arange(min(G, 1_033_000))
        reps = max(1, 2_700_000 // (3 * sel.shape[0]))
    elif shape == "wide":
        sel = rng.choice(odd, min(odd.shape[0], 60_000), replace=False)
    elif shape == "escapes":
        sel = np.concatenate([rng.choice(even, 50_000, replace=False), rng.choice(odd, 400, replace=False)])
    elif shape == "lost acceptor":
        sel, members = rng.choice(even, 40_000, replace=False), MEMBERS[:2]
    elif shape == "runs":
        sel, shuffle = np.sort(rng.choice(G, 30_000, replace=False)), False
    else:  # unaligned, shuffled hint, no status, mix
        sel = rng.choice(G, 20_000, replace=False)
    sel = np.asarray(sel, np.int32)
    k = len(members)
    if shuffle:
        gi = np.repeat(sel, k * reps)
        acc = np.tile(np.array(members, np.int32), sel.shape[0] * reps)
    else:  # every acceptor's replies in turn, groups ascending
        gi = np.tile(sel, k)
        acc = np.repeat(np.array(members, np.int32), sel.shape[0])
    n = gi.shape[0]
    cols = [gi, np.zeros(n, np.int32), np.full(n, 100, np.int32), slot_of[gi].astype(np.int32), acc,
            (slot_of[gi] - 1).astype(np.int32)]
    if shape == "mix":
        odd_v = rng.integers(0, n, n // 50)
        cols[1][odd_v] = rng.choice([0, 1], odd_v.shape[0])
        cols[2][odd_v] = rng.choice([99, 101, 70_000], odd_v.shape[0])
        far = rng.integers(0, n, n // 100)
        cols[3][far] += rng.integers(-3, 5000, far.shape[0]).astype(np.int32)
        cols[4][rng.integers(0, n, n // 100)] = 7777
        dup = rng.integers(0, n, n // 20)
        cols = [np.concatenate([c, c[dup]]) for c in cols]
        n = cols[0].shape[0]
    if shuffle:
        order = rng.permutation(n)
        cols = [c[order] for c in cols]
    return [np.ascontiguousarray(c, np.int32) for c in cols]


def runs_kernels(n):
    """The runs check of a call of n votes under GPX_TRY_REPLY_RUNS or the promise (one engine on the device): ONE launch
    up to pers_max_chunks[2] = 256 workgroups of 256 votes, the check kernel and the work kernel beyond."""
    return {"k_ar_runs_pers"} if (n + 255) // 256 <= 256 else {"k_runs_check", "k_ar_runs"}


def shape_route(shape, geo, n):
    """(front end, kernels that must have run, kernels that must not) of a call of `shape` with n votes."""
    from tests.geometry_common import ar_route, ar_kernels
    if shape == "unaligned":
        return "partition", ar_kernels(("partition", 1)), {"k_scatter_tiles", "k_ar_tiny"}
    if shape == "runs":  # (the tiles or the partition are launched behind the check's gate word and return at once)
        return "runs", {"k_emit_dec_runs"} | runs_kernels(n), {"k_ar_tiny"}
    route = ar_route(geo, n)
    want = set(ar_kernels(route))
    if shape == "shuffled hint":
        want |= runs_kernels(n)
    return route[0], want, ({"k_scatter_ar16"} if route[0] == "tiles" else set()) | ({"k_ar_tiny"} if route[0] != "tiny" else set())


class HostAsDev:
    """An engine behind the host calls where the driver expects DevEngine's accept_reply (the CPU model's engine a)."""

    def __init__(self, e):
        self.e, self.raw, self.kernels = e, None, []

    def __getattr__(self, name):
        return getattr(self.e, name)

    def accept_reply(self, *cols, unaligned=False, status=True):
        return self.e.accept_reply(*cols)


def make_alternation_pair(lib_a, lib_b, G, seed):
    rng = np.random.default_rng(seed)
    nmax = max(3 * G * max(1, 2_700_000 // (3 * G)), 1 << 16)
    ea = Engine(lib_a, 100, G, kmax=3, window=8, max_batch=nmax + nmax // 16 + 4096)
    eb = Engine(lib_b, 100, G, kmax=3, window=8, max_batch=nmax + nmax // 16 + 4096)
    mem = np.tile(np.array(MEMBERS, np.int32), (G, 1))
    rows = lockstep_rows(G, rng)
    for e in (ea, eb):
        assert (e.create_groups(np.arange(G), mem, 3, rows) == S_OK).all()
    return ea, eb


def run_alternation(ea, eb, G, seq, seed, check=None):
    """Leg (g): the accept-reply calls of `seq` on ONE pair of engines (a: DevEngine or HostAsDev), proposals, ACCEPTs
    and COMMITs between the calls behind the 17-call walk.  check(c, shape, n, kernels of the call): the caller's
    per-call assertion.  Returns per call dict(shape, n, decided)."""
    from gigapaxos_amd import TRY_REPLY_RUNS
    rng = np.random.default_rng(seed)
    g = np.arange(G, dtype=np.int32)
    for _ in range(3):  # three slots outstanding everywhere
        same_answer("propose", ea.propose(g), eb.propose(g), "opening proposals")
    newest = (eb.snapshot(g)[0]["next_proposal_slot"].astype(np.int64) - 1).astype(np.int32)
    vote = newest - 2   # the slot each group's next votes are for: its oldest undecided one
    log = []
    for c, shape in enumerate(seq):
        if c in (20, 32):  # slots stay outstanding: every group proposes again
            pa, pb = ea.propose(g), eb.propose(g)
            same_answer("propose", pa, pb, f"proposals of every group before call {c}")
            ok = pb[4] == S_OK
            newest[ok] = pb[0][ok]
        if c >= 17 and c % 3 == 2:
            sub = np.unique(rng.choice(G, 5000)).astype(np.int32)
            pa, pb = ea.propose(sub), eb.propose(sub)
            same_answer("propose", pa, pb, f"proposals before call {c}")
            ok = pb[4] == S_OK
            newest[sub[ok]] = pb[0][ok]
            same_answer("accept", ea.accept(sub, pb[1], pb[2], pb[0], pb[3]), eb.accept(sub, pb[1], pb[2], pb[0], pb[3]),
                        f"ACCEPTs before call {c}")
            hv = np.full(sub.shape[0], C_HASVALUE, np.uint8)
            same_answer("commit", ea.commit(sub, pb[1], pb[2], pb[0], pb[3], hv), eb.commit(sub, pb[1], pb[2], pb[0], pb[3], hv),
                        f"COMMITs before call {c}")
        cols = shape_votes(shape, G, np.minimum(vote, newest), rng)
        n = cols[0].shape[0]
        voted = np.unique(cols[0])
        vote[voted] = np.minimum(vote[voted] + 1, newest[voted] + 1)
        hint = shape in ("runs", "shuffled hint")
        if hint:
            ea.set_ordered_batches(TRY_REPLY_RUNS), eb.set_ordered_batches(TRY_REPLY_RUNS)
        da = ea.accept_reply(*cols, unaligned=shape == "unaligned", status=shape != "no status")
        db = eb.accept_reply(*cols)
        if hint:
            ea.set_ordered_batches(0), eb.set_ordered_batches(0)
        what = f"call {c} ({shape}, {n} votes)"
        assert da.as_tuple_array().shape == db.as_tuple_array().shape and (da.as_tuple_array() == db.as_tuple_array()).all(), what
        if da.status is not None:
            assert (da.status == db.status).all(), what + " status"
        if check:
            check(c, shape, n, ea.kernels[-1] if ea.kernels else set())
        log.append(dict(shape=shape, n=n, decided=int(db.gidx.shape[0])))
    sample = np.unique(np.concatenate([rng.integers(0, G, 20_000), np.arange(0, min(G, 2048))])).astype(np.int32)
    assert ea.snapshot(sample)[0].tobytes() == eb.snapshot(sample)[0].tobytes()
    assert ea.counters() == eb.counters()
    return log


def skewed_frames(names, tile, ntiles, rng, light_slots):
    """A burst whose tiles of `tile` frames are heavy and light in turn: BATCHED_ACCEPT_REPLYs with 48 slots in
    descending order (the decoder sorts them itself, slot by slot) against `light_slots` ascending ones.  A light tile
    is parsed long before the heavy one in front of it, so its look-back finds that tile's word as an EARLIER call left
    it; only the epoch in the word tells it to wait."""
    from gigapaxos_amd import wire as W
    frames = []
    for t in range(ntiles):
        for _ in range(tile):
            g = int(rng.integers(0, len(names)))
            base = int(rng.integers(1, 1000))
            slots = list(range(base + 47, base - 1, -1)) if t % 2 == 0 else list(range(base, base + light_slots))
            frames.append(W.batched_accept_reply(names[g], g % 3, 101 + (g & 1), 0, 100, base - 1, slots))
    return frames
