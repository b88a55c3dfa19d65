"""Checkpoint transfer read from the Java, statement by statement, on top of the acceptor reading of
tests/acc_enum_common.py (written from the reference's text, not from the engine's kernels):

  PISM.handleCheckpoint                                              PISM:1852-1879
  PaxosAcceptor.jumpSlot                                             PaxosAcceptor.java:564-578
  PaxosAcceptor.putAndRemoveNextExecutable, `decision == null`       PaxosAcceptor.java:329-338
  PISM.handlePaxosMessage's stopped test                             PISM:456-460

`CpAcceptor` is that reading; its slots are I32 (Java ints), so `statePacket.slotNumber >= getSlot()` stays the plain
signed comparison the Java writes while `i - slotNumber < 0` wraps.  The restore of the app state always succeeds here
(a host that sees it fail does not send the record: include/gpx_checkpoint.h, GPX_CP_PEEK).

The rest of the module is what the CPU and the GPU tests share: the coverage counters, the plans (enumeration, wrap,
differential) and `drive`, which runs op sequences - ACCEPTs, commits and checkpoint records, one group per sequence -
through the model and, when given one, an engine behind the C-ABI.
"""
import numpy as np

from gigapaxos_amd import S_OK, S_STOPPED, S_WINDOW, S_NOGROUP, A_STOP, C_HASVALUE, C_STOP
from tests.acc_enum_common import Acceptor, I32, PValue, COORD, ballot_cmp

CP_PEEK, CP_ADOPT, CP_MOVED = 1, 1, 2
INT_MAX, INT_MIN = 2**31 - 1, -2**31

CP_COVERAGE = {"jump_lt_W": 0, "jump_eq_W": 0, "jump_gt_W": 0, "cp_eq_slot_minus_1": 0, "cp_eq_slot": 0,
               "tail_valued": 0, "tail_rebuilt": 0, "tail_stopped": 0, "tail_blocked_after_gc": 0,
               "accepts_kept_flag_off": 0, "wrap_adopted_not_moved": 0, "wrap_not_adopted": 0}


def reset_coverage():
    for k in CP_COVERAGE:
        CP_COVERAGE[k] = 0


class CpAcceptor(Acceptor):
    """PaxosAcceptor + PISM.handleCheckpoint.  `window` only classifies jumps for the coverage counters."""

    def __init__(self, slot, ballot, gc_slot, from_disk=True, window=8):
        super().__init__(I32(slot), ballot, I32(gc_slot), from_disk)
        self.window = window

    # ---- PaxosAcceptor.java:564-578 (assertions are off) ---------------------------------------------------------
    def jumpSlot(self, slotNumber):
        i = self._slot
        if slotNumber - i > 1 << 20:
            # the loop below, for distances no test could walk: the same removals, the same count of executed()
            for s in [s for s in self.committed if 0 <= int(I32(s) - i) < int(slotNumber - i)]:
                del self.committed[s]
            if self.from_disk:
                for s in [s for s in self.accepted if 0 <= int(I32(s) - i) < int(slotNumber - i)]:
                    del self.accepted[s]
            self._slot = slotNumber
            return
        while i - slotNumber < 0:
            self.executed(i, False)
            self.committed.pop(i, None)
            if self.from_disk:
                self.accepted.pop(i, None)
            i = i + 1

    # ---- PaxosAcceptor.java:325-338: the entry with decision == null -----------------------------------------------
    def putAndRemoveNextExecutable(self, decision):
        if decision is None:
            if self.stopped:
                return None
            decision = self.committed.get(self._slot)
            if decision is None:
                return None
            n_acc = len(self.accepted)
            nx = super().putAndRemoveNextExecutable(decision)
            if nx is None and len(self.accepted) < n_acc:
                CP_COVERAGE["tail_blocked_after_gc"] += 1
            return nx
        return super().putAndRemoveNextExecutable(decision)

    def peekCheckpoint(self, cp):
        """-> (status, adopt, from, the slot jumpSlot would leave) without changing anything"""
        if self.stopped:
            return (S_STOPPED, False, 0, 0)
        adopt = int(cp) >= int(self._slot)
        to = self._slot
        if adopt and (I32(cp) + 1) - self._slot > 0:
            to = I32(cp) + 1
        return (S_OK, adopt, int(self._slot), int(to))

    # ---- PISM:1852-1879 ------------------------------------------------------------------------------------------------
    def handleCheckpoint(self, cp):
        """-> (status, adopt, from, to, run)"""
        if self.stopped:                                   # PISM:456-460
            return (S_STOPPED, False, 0, 0, None)
        frm = self._slot
        cp = I32(cp)
        adopt = int(cp) >= int(self._slot)                 # statePacket.slotNumber >= this.paxosState.getSlot()
        if adopt:
            kept = [s for s in self.accepted if 0 <= int(I32(s) - frm) < int((cp + 1) - frm)]
            self.jumpSlot(cp + 1)
            d = int(self._slot - frm)
            W = self.window
            if d > 0:
                CP_COVERAGE["jump_lt_W" if d < W else "jump_eq_W" if d == W else "jump_gt_W"] += 1
                CP_COVERAGE["cp_eq_slot"] += d == 1
                CP_COVERAGE["accepts_kept_flag_off"] += bool(kept) and not self.from_disk
            else:
                CP_COVERAGE["wrap_adopted_not_moved"] += 1
        else:
            CP_COVERAGE["cp_eq_slot_minus_1"] += int(cp) == int(frm) - 1
            CP_COVERAGE["wrap_not_adopted"] += int(cp - frm) >= 0
        before = (dict(self.committed), self.stopped)
        run = self.extractExecuteAndCheckpoint(None)
        if run is not None:
            first = before[0].get(run[0])
            CP_COVERAGE["tail_valued" if first is not None and first.has_value else "tail_rebuilt"] += 1
            CP_COVERAGE["tail_stopped"] += self.stopped
        return (S_OK, adopt, int(frm), int(self._slot), run)

    def apply(self, op):
        if op[0] == "J":
            return self.handleCheckpoint(op[1])
        # the op's slot and median as Java ints: the subtractions of the reading wrap whichever operand they come from
        return super().apply((op[0], I32(op[1]), op[2], I32(op[3]), op[4]))

    # ---- what gpx_group_dump shows of the acceptor ---------------------------------------------------------------------
    def dump_maps(self):
        key = lambda t: int(I32(t[0]) - self._slot)   # noqa: E731
        acc = sorted([(int(s), v.ballot[0], v.ballot[1], 1 if v.stop else 0) for s, v in self.accepted.items()], key=key)
        com = sorted([(int(s), v.ballot[0], v.ballot[1], int(v.median), 1 if v.has_value else 0,
                       1 if (v.stop and v.has_value) else 0) for s, v in self.committed.items()], key=key)
        return (tuple(int(x) for x in self.row()) + (1 if self.stopped else 0,), acc, com)


def parse_dump(d, slot):
    """gpx_group_dump's words (docs/HISTORY.md, state dump) -> the shape of CpAcceptor.dump_maps"""
    d = [int(x) for x in d]
    pos = 3 + d[2]
    head = tuple(d[pos:pos + 5])
    pos += 5
    na = d[pos]
    acc = [tuple(d[pos + 1 + 4 * i: pos + 5 + 4 * i]) for i in range(na)]
    pos += 1 + 4 * na
    nc = d[pos]
    com = [tuple(d[pos + 1 + 6 * i: pos + 7 + 6 * i]) for i in range(nc)]
    key = lambda t: int(I32(t[0]) - slot)   # noqa: E731
    return (head, sorted(acc, key=key), sorted(com, key=key))


# ---- the engine's window rules (include/gpx.h, GPX_S_WINDOW: "record not applied") -------------------------------------
def window_refuses(m, op, W):
    """The engine keeps each map in a ring of W entries indexed by slot & (W - 1).  An ACCEPT it would store is refused
    while another live accepted slot holds its ring entry; a commit W or more slots ahead of the next slot is refused.
    The Java has no such limit: a refused record is not shown to the model."""
    kind, slot = op[0], I32(op[1])
    if kind == "A":
        if ballot_cmp((op[2], COORD), m.ballot) >= 0 and slot - m.acceptedGCSlot > 0:
            return any(int(s) != int(slot) and (int(s) - int(slot)) % W == 0 for s in m.accepted)
        return False
    return int(slot - m._slot) >= W


# ---- plans -----------------------------------------------------------------------------------------------------------------
def _ops_near(rng, base, n, stops=True):
    """n random ACCEPT / commit ops on slots base .. base + 3"""
    out = []
    for _ in range(n):
        kind = "ADB"[int(rng.integers(0, 3))]
        s = int(I32(base) + int(rng.integers(0, 4)))
        bn = int(rng.integers(0, 3))
        md = int(I32(base) + int(rng.choice([-2, -1, 0, 1, 2])))
        st = int(stops and kind != "B" and rng.random() < 0.2)
        out.append((kind, s, bn, md, st))
    return out


def scenario_sequences(W):
    """hand-built sequences, one per coverage counter (the group starts at slot 1, gc -1, ballot 0)"""
    A, D, B, J = (lambda s, b=0, m=-1, st=0: ("A", s, b, m, st)), (lambda s, b=0, m=-1, st=0: ("D", s, b, m, st)), \
        (lambda s, b=0, m=-1: ("B", s, b, m, 0)), (lambda cp: ("J", cp, 0, 0, 0))
    return [
        (J(0), A(1)),                                        # cp == slot - 1: not adopted
        (J(1), A(2)),                                        # cp == slot: d = 1
        (A(1), A(2), D(3), J(2), A(4)),                      # jump over two accepts; tail executes the valued commit of 3
        (A(1), D(2), D(3), J(W - 1), D(W + 1)),              # d = W - 1, parked commits dropped
        (A(2), D(3), J(W), A(W + 1), D(W + 1)),              # d = W
        (A(2), D(3), J(W + 1), A(W + 2), D(W + 2)),          # d = W + 1
        (A(3), D(2), J(5000), A(5001), D(5001)),             # far
        (A(3, 1), B(3, 1), J(2), A(4)),                      # tail rebuilt from an accept
        (A(3, 1, -1, 1), B(3, 1), A(4), D(4), J(2), A(5)),   # tail stopped (the accepted stop), later commit cleared
        (D(3, 0, -1, 1), J(2), A(4)),                        # tail stopped by a valued stop
        (A(2, 1), A(3, 1), B(3, 1), B(2, 2, 1), J(1), A(3, 2), D(2)),  # placeholder at 2 (ballot 2 != 1): the tail is blocked
        # a placeholder parked at 5 with median 4, slot 2 executed and accepted again late: the jump to 5 leaves that
        # accept (it lies below the jumped range), the blocked tail's collection takes it
        (J(1), B(5, 1, 4), D(2), A(2), J(4), A(5, 1), D(6)),
        (A(2), B(3, 1, 3), J(2), A(3, 1)),                   # flag off: the tail's collection takes the accept jumped over
        (A(1), A(2), A(3), J(3), A(4), B(4)),                # accepts in the range: kept with the flag off
        (D(2, 0, -1, 1), J(0), D(1), A(2)),                  # not adopted, nothing parked at the slot: no tail
        (D(1, 0, -1, 1), J(5), A(6)),                        # stopped group: the record is dropped
        (D(2), D(3), J(0), D(1), J(-1), A(4)),               # not adopted twice
        (A(1), D(1), D(3), J(1), J(2), D(3), A(4)),          # behind the slot, then at it
    ]


def enum_sequences(W, n=3000, seed=11):
    """The enumeration plan of one table: n sequences over acc_enum_common's alphabet plus 'J' (cp in a small set around
    the slots), every J followed by at least one ACCEPT or commit.  Deterministic in (W, n, seed)."""
    rng = np.random.default_rng(seed + W)
    seqs = list(scenario_sequences(W))
    jumps = [-1, 0, 1, 2, 3, W - 1, W, W + 1, 2 * W, 5000]
    while len(seqs) < n:
        sq = _ops_near(rng, 1, int(rng.integers(0, 4)))
        nxt = 1                                               # an upper estimate of the group's next slot
        for _ in range(int(rng.integers(1, 3))):
            cp = int(rng.choice(jumps)) + (nxt - 1 if rng.random() < 0.5 else 0)
            sq.append(("J", cp, 0, 0, 0))
            nxt = max(nxt, cp + 1)
            sq += _ops_near(rng, nxt - 1, int(rng.integers(1, 4)))
        seqs.append(tuple(sq))
    return seqs[:n]


WRAP_STARTS = (INT_MAX - 3, INT_MIN + 3)


def wrap_sequences():
    """[(start slot, sequence)]: groups restored at Integer.MAX_VALUE - 3 and MIN_VALUE + 3"""
    hi, lo = WRAP_STARTS
    J = lambda cp: ("J", cp, 0, 0, 0)   # noqa: E731
    A = lambda s, m: ("A", int(I32(s)), 0, int(I32(m)), 0)   # noqa: E731
    D = lambda s, m: ("D", int(I32(s)), 0, int(I32(m)), 0)   # noqa: E731
    return [
        (hi, (A(hi + 1, hi - 1), D(hi + 2, hi - 1), J(INT_MAX), A(INT_MIN, hi - 1), D(INT_MIN, hi - 1))),  # target = MIN_VALUE
        (hi, (D(hi + 1, hi - 1), J(hi), A(hi + 2, hi - 1))),                 # the tail crosses MAX_VALUE
        (hi, (J(INT_MIN + 5), A(hi, hi - 1), D(hi, hi - 1))),                # cp past the wrap: not adopted
        (hi, (A(hi, hi - 1), J(INT_MIN), D(hi, hi - 1), A(hi + 1, hi - 1))),
        (lo, (J(5), A(lo, lo - 1), D(lo, lo - 1))),                          # positive cp, slot just past MIN_VALUE: adopted, not moved
        (lo, (D(lo + 1, lo - 1), J(INT_MAX - 1), D(lo, lo - 1))),            # the same with a commit parked ahead
        (lo, (A(lo + 1, lo - 1), J(lo + 2), A(lo + 3, lo - 1), D(lo + 3, lo - 1))),   # an ordinary jump near MIN_VALUE
        (lo, (J(lo - 1), A(lo, lo - 1))),                                    # cp == slot - 1
    ]


def segments(seq):
    """maximal runs of ops that go through the same call; a checkpoint record is a call of its own (records of one call
    name distinct groups)"""
    segs = []
    for op in seq:
        call = "A" if op[0] == "A" else "J" if op[0] == "J" else "C"
        if segs and segs[-1][0] == call and call != "J":
            segs[-1][1].append(op)
        else:
            segs.append((call, [op]))
    return segs


def expected(m, op, W):
    """the model's answer to one op in the engine's columns; the model advances unless the engine's window refuses"""
    if op[0] == "J":
        st, adopt, frm, to, run = m.handleCheckpoint(op[1])
        fl = (CP_ADOPT if adopt else 0) | (CP_MOVED if st == S_OK and to != frm else 0)
        return (st, frm, to, fl), run
    if not m.stopped and window_refuses(m, op, W):   # (a stopped group drops the record before the ring is looked at)
        return ((S_WINDOW, 0, 0, 0, 0) if op[0] == "A" else S_WINDOW), None
    r = m.apply(op)
    return (r[:5] if op[0] == "A" else r[0]), r[-1]


def drive(seqs, W, from_disk, starts=None, engine=None, checkpoint=None, dumps=200, models=None):
    """One group per sequence (group g starts at slot starts[g], default 1, with gc = slot - 2: a HotRestoreInfo row).
    Phase p of all groups goes out as one batch per call type.  With `engine` every reply, status, dense output, run,
    the counts, the final rows and `dumps` sampled dumps are compared with the model; `checkpoint(engine, gidx, cp)`
    -> ((from, to, flags, status), runs [k, 3], counts).  Returns (models, records checked)."""
    G = len(seqs)
    starts = [1] * G if starts is None else list(starts)
    if models is None:   # (given: the sequences continue the groups those models describe)
        models = [CpAcceptor(starts[g], (0, COORD), I32(starts[g]) - 2, from_disk, W) for g in range(G)]
    segs = [segments(s) for s in seqs]
    checked = 0
    for p in range(max(len(s) for s in segs)):
        for call in ("A", "C", "J"):
            recs = [(j, g, op) for g, sg in enumerate(segs) if p < len(sg) and sg[p][0] == call
                    for j, op in enumerate(sg[p][1])]
            if not recs:
                continue
            recs.sort(key=lambda r: (r[0], r[1]))
            want = [expected(models[g], op, W) for _, g, op in recs]
            checked += len(recs)
            if engine is None:
                continue
            by_group = {}
            for (j, g, op), (_, run) in zip(recs, want):
                if run is not None:
                    by_group.setdefault(g, []).append((g, int(run[0]), int(run[1])))
            n = len(recs)
            gi = np.array([r[1] for r in recs], np.int32)
            sl = np.array([int(r[2][1]) for r in recs], np.int64).astype(np.int32)
            where = lambda i: f"phase {p} call {call} record {i}: sequence {seqs[recs[i][1]]} op {recs[i][2]}"  # noqa: E731
            if call == "J":
                (frm, to, fl, st), runs, counts = checkpoint(engine, gi, sl)
                got = list(zip(st.tolist(), frm.tolist(), to.tolist(), fl.tolist()))
                exp = [w[0] for w in want]
                want_runs = [t for (j, g, op), (_, run) in zip(recs, want) if run is not None for t in by_group[g]]
                got_runs = [tuple(t) for t in runs.tolist()]
                want_counts = (sum(1 for w in exp if w[3] & CP_ADOPT), 0, sum(1 for w in exp if w[0] == S_STOPPED),
                               len(want_runs))
                got_counts = (counts.n_adopted, counts.n_nogroup, counts.n_stopped, counts.n_runs)
                assert got_counts == want_counts, (p, got_counts, want_counts)
            else:
                bn = np.array([r[2][2] for r in recs], np.int32)
                bc = np.full(n, COORD, np.int32)
                md = np.array([int(r[2][3]) for r in recs], np.int64).astype(np.int32)
                want_runs = [t for g in sorted(by_group) for t in by_group[g]]
                if call == "A":
                    fa = np.array([A_STOP if r[2][4] else 0 for r in recs], np.uint8)
                    (rb, rc, rm, rf, st), runs = engine.accept(gi, bn, bc, sl, md, fa)
                    got = list(zip(st.tolist(), rb.tolist(), rc.tolist(), rm.tolist(), rf.tolist()))
                    exp = [tuple(int(x) for x in w[0]) for w in want]
                else:
                    kd = np.array([(C_HASVALUE | (C_STOP if r[2][4] else 0)) if r[2][0] == "D" else 0 for r in recs],
                                  np.uint8)
                    st, runs = engine.commit(gi, bn, bc, sl, md, kd)
                    got = st.tolist()
                    exp = [w[0] for w in want]
                got_runs = [tuple(t) for t in runs.as_tuple_array().tolist()]
            if got != exp:
                i = next(i for i in range(n) if got[i] != exp[i])
                raise AssertionError(f"{where(i)}: got {got[i]}, the Java gives {exp[i]}")
            assert got_runs == want_runs, (p, call, [x for x in zip(got_runs, want_runs) if x[0] != x[1]][:3],
                                           len(got_runs), len(want_runs))
    if engine is not None:
        snap, st = engine.snapshot(np.arange(G))
        assert (st == S_OK).all()
        got_rows = list(zip(snap["acc_slot"].tolist(), snap["acc_bnum"].tolist(), snap["acc_bcoord"].tolist(),
                            snap["acc_gc_slot"].tolist()))
        exp_rows = [tuple(int(x) for x in m.row()) for m in models]
        for g in range(G):
            assert got_rows[g] == exp_rows[g], (seqs[g], got_rows[g], exp_rows[g])
        rng = np.random.default_rng(G)
        sample = set(range(min(G, 32))) | set(rng.choice(G, size=min(dumps, G), replace=False).tolist())
        for g in sorted(sample):
            assert parse_dump(engine.dump(g), models[g]._slot) == models[g].dump_maps(), (g, seqs[g])
    return models, checked


def create_at(engine, starts, kmax=3):
    """groups 0 .. len(starts) - 1 from HotRestoreInfo rows at the given slots (gc = slot - 2, ballot (0, COORD))"""
    from gigapaxos_amd import hri_create

    G = len(starts)
    rows = hri_create(G, 3, COORD)
    rows["acc_slot"] = np.array([int(I32(s)) for s in starts], np.int64).astype(np.int32)
    rows["acc_gc_slot"] = np.array([int(I32(s) - 2) for s in starts], np.int64).astype(np.int32)
    members = np.zeros((G, kmax), np.int32)
    members[:, :3] = [COORD, COORD + 1, COORD + 2]
    assert (engine.create_groups(np.arange(G), members, 3, rows) == S_OK).all()


# ---- the differential plan: a checkpoint record against one valued decision per skipped slot -----------------------------
def diff_plan(G, W, from_disk, ds, seed=5, every=1):
    """-> (history, cps): history[g] = the ops of group g before the checkpoint, cps = [(g, cp)] for every `every`-th
    group, its distance cycling through `ds`.  Built against the model so that - a rule of construction, not a filter -
    no valued stop is parked in [slot, cp] and every commit parked at or after the slot carries a median at most the
    group's accepted-GC slot: then jumpSlot(cp + 1) + extractExecuteAndCheckpoint(null) and one valued decision per slot
    of [slot, cp] with median = that GC slot leave the same acceptor."""
    rng = np.random.default_rng(seed + 131 * W + from_disk)
    history, cps = [], []
    for g in range(G):
        m = CpAcceptor(1, (0, COORD), -1, from_disk, W)
        ops = []

        def do(op):
            assert not window_refuses(m, op, W)
            m.apply(op)
            ops.append(op)
        for s in range(1, 1 + int(rng.integers(0, 4))):        # a few slots executed; the GC slot follows them
            do(("D", s, 0, s - 1, 0))
        slot, gc = int(m._slot), int(m.acceptedGCSlot)
        d = ds[(g // every) % len(ds)]
        cp = slot + d - 1
        chosen = g % every == 0
        for _ in range(int(rng.integers(0, 6))):
            kind = "ADB"[int(rng.integers(0, 3))]
            s = slot + int(rng.integers(0 if kind == "A" else 1, W))   # no commit at the slot itself: nothing executes
            stop = int(kind != "B" and rng.random() < 0.25)
            if stop and (not chosen or s <= cp):
                stop = 0   # no stop inside the jumped range (an accepted one turns into a valued one when a batched
                           # commit of its ballot meets it) and none on a neighbour
            op = (kind, s, int(rng.integers(0, 3)), gc - int(rng.integers(0, 2)), stop)
            if window_refuses(m, op, W) or m.stopped:
                continue
            do(op)
        assert int(m.acceptedGCSlot) == gc and int(m._slot) == slot and not m.stopped
        assert all(v.median <= gc and not (v.has_value and v.stop and s <= cp) for s, v in m.committed.items())
        history.append(tuple(ops))
        if chosen:
            cps.append((g, cp))
    return history, cps


def decisions_for(models, cps):
    """the oracle's side of the equivalence: for each (g, cp) one GPX_C_HASVALUE decision per slot of [slot, cp] with
    median = the group's accepted-GC slot, a group's records in slot order -> (gidx, slot, median) columns"""
    gi, sl, md = [], [], []
    for g, cp in cps:
        m = models[g]
        d = cp + 1 - int(m._slot)
        assert d > 0
        gi.append(np.full(d, g, np.int32))
        sl.append(np.arange(int(m._slot), cp + 1, dtype=np.int64).astype(np.int32))
        md.append(np.full(d, int(m.acceptedGCSlot), np.int32))
    return np.concatenate(gi), np.concatenate(sl), np.concatenate(md)


# ---- states no handler sequence reaches from empty maps: a placeholder next to the ACCEPT that matches it ----------------
# (handleAccept and handleBatchedCommit both turn such a pair into a valued decision on arrival; a group image - or a
# future recovery path - can still hold it, and reconstructDecision's second branch is what the tail then takes.)
# (slot, gc, accepted {slot: (bnum, stop)}, committed {slot: (bnum, median, has_value, stop)}, cp)
STATE_CASES = [
    (5, 3, {5: (1, 0), 6: (1, 1), 7: (1, 0)}, {5: (1, 3, 0, 0), 6: (1, 3, 0, 0), 7: (1, 3, 0, 0)}, 2),   # not adopted; rebuilt 5, 6 (stop)
    (1, -1, {4: (2, 0)}, {4: (2, -1, 0, 0)}, 3),                                                          # jump to 4, rebuilt 4
    (1, -1, {2: (2, 0), 3: (1, 0)}, {2: (2, -1, 0, 0), 3: (2, -1, 0, 0)}, 0),                            # cp 0 < slot 1, nothing parked at 1: no tail
    (2, 0, {2: (2, 0), 3: (1, 0), 4: (1, 0)}, {2: (2, 0, 0, 0), 3: (2, 0, 0, 0), 4: (1, 0, 1, 0)}, 1),   # rebuilt 2, blocked at 3 (ballots differ)
]


def state_model(case, W, from_disk):
    slot, gc, acc, com, _ = case
    m = CpAcceptor(slot, (2, COORD), gc, from_disk, W)
    m.accepted = {I32(s): PValue((b, COORD), I32(s), -1, True, bool(st)) for s, (b, st) in acc.items()}
    m.committed = {I32(s): PValue((b, COORD), I32(s), md, bool(hv), bool(st)) for s, (b, md, hv, st) in com.items()}
    return m


def state_image_rows(rows, cases, W, kmax=3):
    """the exported main rows of len(cases) fresh groups (uint8 [n, stride]) with the acceptor of each case written in"""
    from gigapaxos_amd import image as IM

    L = IM.layout(kmax, W)
    w = np.ascontiguousarray(rows).view("<i4").reshape(len(cases), -1).copy()
    for r, (slot, gc, acc, com, _) in zip(w, cases):
        r[7], r[8], r[9], r[10] = slot, 2, COORD, gc
        for s in set(acc) | set(com):
            i = s & (W - 1)
            fl = 0
            if s in acc:
                r[L["acc"] + 4 * i: L["acc"] + 4 * i + 3] = (s, acc[s][0], COORD)
                fl |= IM.R_PRESENT | (IM.R_STOP if acc[s][1] else 0)
            if s in com:
                b, md, hv, st = com[s]
                r[L["com"] + 4 * i: L["com"] + 4 * i + 4] = (s, b, COORD, md)
                fl |= (IM.R_PRESENT | (IM.R_HASVALUE if hv else 0) | (IM.R_STOP if st else 0)) << 8
            r[L["acc"] + 4 * i + 3] = fl
    return w.view(np.uint8).reshape(len(cases), -1)


# ---- a model as the engine's rings: the table format of tests/checkpoint_emulation.cpp ----------------------------------
def ring_words(m, W):
    """[(ring index, accepted entry {slot, bnum, bcoord, flags}, committed entry {slot, bnum, bcoord, median})] of the ring
    indices that hold something; the flag word carries the accepted entry's flags in bits 0-7 and the committed entry's in
    bits 8-15 (gpx_kernels.hip.h, AccView)"""
    out = {}
    for s, v in m.accepted.items():
        w = int(s) & (W - 1)
        assert w not in out, "two accepted slots on one ring entry"
        out[w] = [[int(s), v.ballot[0], v.ballot[1], 1 | (2 if v.stop else 0)], [0, 0, 0, 0]]
    seen = set()
    for s, v in m.committed.items():
        w = int(s) & (W - 1)
        assert w not in seen, "two committed slots on one ring entry"
        seen.add(w)
        e = out.setdefault(w, [[0, 0, 0, 0], [0, 0, 0, 0]])
        e[0][3] |= (1 | (4 if v.has_value else 0) | (2 if v.stop and v.has_value else 0)) << 8
        e[1] = [int(s), v.ballot[0], v.ballot[1], int(v.median)]
    return [(w, a, c) for w, (a, c) in sorted(out.items())]


def table_words(models, live, W):
    """the integers of one table: per group flags (0 = dead), slot, gc, then its live ring entries"""
    out = []
    for m, alive in zip(models, live):
        if not alive:
            out += [0, 0, 0, 0]
            continue
        rw = ring_words(m, W)
        out += [1 | (2 if m.stopped else 0) | (3 << 8), int(m._slot), int(m.acceptedGCSlot), len(rw)]
        for w, a, c in rw:
            out += [w] + a + c
    return out
