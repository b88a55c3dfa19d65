"""The rules of the retransmission sweep (include/gpx_timers.h), restated in numpy over DENSE poke rows - the columns
gpx_poke_scan writes, which the tests take from the CPU oracle's orc_poke_scan - and `JavaWaitfor`, a reading of the
time half of the reference's WaitforUtility (paxosutil/WaitforUtility.java:39-40, 101-127) and of both
PaxosCoordinatorState.testAndSetWaitingTooLong (PCS:715-739) on an injected clock, with double arithmetic exactly as
the Java writes it."""
import math

import numpy as np

PEEK = 1
MAX_STEPS = 32
COUNT_MAX = 255
INT32_MAX = 2**31 - 1
POKE_NONE, POKE_ACCEPT, POKE_PREPARE = 0, 1, 2
S_NOGROUP = 1
ROW_COLS = ("poke", "slot", "bnum", "bcoord", "median_cp", "flags", "heard")   # the seven columns a hit carries over
OUT_COLS = ("gidx",) + ROW_COLS + ("count", "waited")                          # the call's ten output columns


# ---- the reference -----------------------------------------------------------------------------------------------------
class JavaWaitfor:
    """WaitforUtility's initTime and retransmissionCount, and the test PaxosCoordinatorState makes on them.  `clock()` is
    System.currentTimeMillis().  One object is one wait: the proposal's waitfor (ACCEPT_TIMEOUT,
    ACCEPT_RETRANSMISSION_BACKOFF_FACTOR) or waitforMyBallot (PREPARE_TIMEOUT, PREPARE_RETRANSMISSION_BACKOFF_FACTOR)."""

    def __init__(self, clock, timeout_ms, factor=1.5):
        self.clock, self.timeout, self.factor = clock, int(timeout_ms), float(factor)
        self.init_time = clock()            # private long initTime = System.currentTimeMillis();
        self.retransmission_count = 0       # private int retransmissionCount = 0;

    def total_wait_time(self):              # return System.currentTimeMillis() - this.initTime;
        return self.clock() - self.init_time

    wait_time = total_wait_time

    def incr_retransmisson_count(self, reset_init_time):
        self.retransmission_count += 1
        if reset_init_time:
            self.init_time = self.clock()

    def too_long(self, wait):
        """wait > TIMEOUT * Math.pow(FACTOR, count): a long against a double"""
        return float(wait) > self.timeout * math.pow(self.factor, self.retransmission_count)

    def test_and_set_waiting_too_long(self):
        if self.too_long(self.total_wait_time()):
            self.incr_retransmisson_count(True)
            return True
        return False


def backoff_table(timeout_ms, factor=1.5, n_steps=MAX_STEPS):
    """gpx_rtx_backoff_table, in Python's doubles (IEEE, as the C library's and Java's)"""
    out = []
    for c in range(n_steps):
        x = timeout_ms * math.pow(factor, c)
        out.append(INT32_MAX if x >= INT32_MAX else int(math.floor(x)))
    return out


# ---- the engine's rules --------------------------------------------------------------------------------------------------
def _u32(a):
    return np.asarray(a).astype(np.int64) & 0xFFFFFFFF


def key_of(poke, slot, bnum, bcoord):
    """the 32-bit identity of a wait (rtx_key, gpx_timers.hip.h): odd multipliers, the murmur3 finaliser, never 0"""
    M = 0xFFFFFFFF
    h = (_u32(slot) * 0x9e3779b1 & M) ^ (_u32(bnum) * 0x85ebca77 & M) ^ (_u32(bcoord) * 0xc2b2ae3d & M) ^ \
        (_u32(poke) * 0x27d4eb2f & M)
    h ^= h >> 16
    h = h * 0x85ebca6b & M
    h ^= h >> 13
    h = h * 0xc2b2ae35 & M
    h ^= h >> 16
    return np.where(h == 0, 1, h).astype(np.uint32)


def wrap32(x):
    """an integer as the int32 of the same residue modulo 2^32"""
    return ((int(x) + 2**31) & 0xFFFFFFFF) - 2**31


class Timers:
    """the three timer words of a table of n_groups, zeroed as the engine allocates them"""

    def __init__(self, n_groups):
        self.n = n_groups
        self.key = np.zeros(n_groups, np.uint32)
        self.since = np.zeros(n_groups, np.int32)
        self.count = np.zeros(n_groups, np.uint8)


def sweep(T, groups, rows, now_ms, accept_ms, prepare_ms, flags, cap):
    """One call over the distinct entries `groups` (group numbers, any int64; out of range allowed), whose dense poke
    rows are rows[col][i] for col in ROW_COLS + ("status",).  Changes the words of T as the call does.

    -> dict: hits (entry indices written, ascending), cols (the ten output columns of those, by name),
       counts (n_hits, n_nogroup, n_waiting, n_fired), due (all due entry indices, written or not),
       armed (entries whose wait was new to this call)"""
    groups = np.asarray(groups, np.int64)
    n = groups.size
    assert len(accept_ms) == len(prepare_ms) and 1 <= len(accept_ms) <= MAX_STEPS and cap >= 0 and not flags & ~PEEK
    assert min(accept_ms) >= 0 and min(prepare_ms) >= 0
    now = wrap32(now_ms)
    inr = (groups >= 0) & (groups < T.n)
    g = np.where(inr, groups, 0)
    k0 = np.where(inr, T.key[g], 0).astype(np.uint32)
    s0 = np.where(inr, T.since[g], 0).astype(np.int64)
    c0 = np.where(inr, T.count[g], 0).astype(np.int64)
    poke = np.asarray(rows["poke"]).astype(np.int64)
    nog = np.asarray(rows["status"]) == S_NOGROUP
    assert nog[~inr].all()
    waiting = ~nog & (poke != POKE_NONE)
    k = key_of(poke, rows["slot"], rows["bnum"], rows["bcoord"])
    new = waiting & (k != k0)
    same = waiting & (k == k0)
    waited = ((now - s0 + 2**31) & 0xFFFFFFFF) - 2**31            # (int32_t)((uint32_t)now - (uint32_t)since)
    steps = len(accept_ms)
    idx = np.minimum(c0, steps - 1)
    thr = np.where(poke == POKE_PREPARE, np.asarray(prepare_ms, np.int64)[idx], np.asarray(accept_ms, np.int64)[idx])
    due = same & (waited > thr)
    assert not (due & (waited < 0)).any()
    due_idx = np.nonzero(due)[0]
    written = due_idx[:min(due_idx.size, cap)]
    peek = bool(flags & PEEK)
    c_after = np.minimum(c0 + 1, COUNT_MAX)
    if not peek:
        k1 = np.where(waiting, k, 0).astype(np.uint32)
        s1 = np.where(nog, 0, np.where(new, now, s0))
        c1 = np.where(same, c0, 0)
        c1[written] = c_after[written]
        s1[written] = now
        T.key[g[inr]] = k1[inr]
        T.since[g[inr]] = s1[inr].astype(np.int32)
        T.count[g[inr]] = c1[inr].astype(np.uint8)
    cols = {"gidx": groups[written].astype(np.int32), "count": c_after[written].astype(np.uint8),
            "waited": waited[written].astype(np.int32)}
    for c in ROW_COLS:
        cols[c] = np.asarray(rows[c])[written]
    counts = (int(due_idx.size), int(nog.sum()), int(waiting.sum()), 0 if peek else int(written.size))
    return dict(hits=written, cols=cols, counts=counts, due=due_idx, armed=np.nonzero(new)[0])
