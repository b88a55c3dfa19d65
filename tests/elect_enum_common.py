"""The prepare-reply phase (gpx_election_begin / gpx_prepare_reply_batch and their *_dev twins) enumerated against the
Java reading tests/round_model.Candidate: drivers of tests/test_elect_enum_gpu.py (the HIP engine) and
tests/test_elect_enum_model.py (the same drivers over the oracle, on the CPU).

One group per case, all cases in one engine.  A case is a pre-active SHAPE (0-3 proposals made while the election runs,
with or without a stop last) and a sequence of L LETTERS: the PREPARE replies that reach the candidate, in that order.
The candidate is ME with ballot (BNUM, ME) among non-contiguous member ids; its acceptor stands at slot S0.

  letters   every member x a menu of six pvalue sets (empty; S0 in the low ballot; S0 in the higher ballot; S0+1 and a
            stop at S0+3; S0-1, below first_slot; S0+2 carrying the handle of the pre-active at S0: isDuplicate drops that
            pre-active) + a non-member in my ballot, a higher ballot from a member and from a non-member, a lower ballot
            number, a lower coordinator id; extended: S0+3 flagged GPX_PV_NOOP, in the low ballot again but another
            request (the first of the two to arrive stays), from a reply whose first_slot is S0-1, the pre-active's handle at S0+2 from a reply whose first_slot is S0+1 (the pre-active at S0
            is then BELOW the carried range, where isDuplicate is not asked: it is proposed again), an empty reply with
            first_slot S0-1
  forms     per-step: one host call per arrival position; one-call: ONE call, half of the groups (seeded) with their
            records a few entries apart, the other half with theirs a third of the batch apart (other scatter tiles),
            every group's own order kept - `flip` swaps the halves; dev: the one-call batch through the *_dev calls
  checked   every reply: v_kind, status, e_median when elected, the entry list when elected or preempted; after the
            last reply: snapshot, poke_scan and the drop counter

The reading knows no window.  The engine's limits are restated in engine_refusal from include/gpx.h's words (carried
pvalues live in a ring of `window` entries; the carried range and the re-proposed pre-actives must fit `window` slots) -
not from the kernel: where it predicts a refusal the engine must refuse, and nowhere else."""
import copy
import ctypes as C

import numpy as np

from gigapaxos_amd import Engine, S_OK
from tests.acc_enum_common import I32
from tests.election_common import (plain_rows, S_PREACTIVE, S_WINDOW, EB_PREPARING, V_IGNORED, V_RECORDED, V_ELECTED,
                                   V_PREEMPTED, E_CARRY, E_NOOP, E_PREACTIVE, E_NEWSTOP, PV_STOP, PV_NOOP)
from tests.lifetime_common import DevEngine
from tests.round_model import Candidate, wraparound_max

S_NOGROUP = 1                                   # include/gpx.h
POKE_NONE, POKE_ACCEPT, POKE_PREPARE = 0, 1, 2
ME, BNUM, NON_MEMBER = 101, 2, 77
MEMBERS = {1: [101], 2: [7, 101], 3: [7, 101, 5000], 5: [7, 101, 5000, (1 << 20) + 3, (1 << 30) + 1]}
# S0; wrap: S0 + 2 = Integer.MAX_VALUE, S0 + 3 = MIN_VALUE; wrap+1: one further, so that three PRE-ACTIVE proposals
# (S0 .. S0 + 2) straddle the wrap as well - their TreeMap order is then not their slot order
BASES = {"plain": 5, "wrap": 2 ** 31 - 3, "wrap+1": 2 ** 31 - 2}
SHAPES = [(0, False), (1, False), (2, False), (3, False), (1, True), (3, True)]   # (pre-active proposals, the last a stop)
PRE_HANDLE = [9001, 9002, 9003]
NEAR = 5                                        # one-call: records of a `near` group are NEAR entries apart
LAYOUT_SEED = 20231
KMAP = {"carry": E_CARRY, "noop": E_NOOP, "preactive": E_PREACTIVE, "newstop": E_NEWSTOP}
VMAP = {"ignored": V_IGNORED, "recorded": V_RECORDED, "elected": V_ELECTED, "preempted": V_PREEMPTED}
VNAME = {v: k for k, v in VMAP.items()}


def pv_handle(off, b):
    """The caller's key of the request accepted at S0 + off in ballot b (one request per slot and ballot)."""
    return 50_000 + (off + 1) * 100 + b[0]


def alphabet(K, extended=True, members=None, me=ME, sixth=False):
    """[(acceptor, reply bnum, reply bcoord, first_slot - S0, ((slot - S0, bnum, bcoord, handle, flags), ...))]"""
    mem = members or MEMBERS[K]
    lo, hi = (0, mem[0]), (1, mem[-1])

    def pv(off, b, flags=0, h=None):
        return (off, b[0], b[1], pv_handle(off, b) if h is None else h, flags)
    menu = [(), (pv(0, lo),), (pv(0, hi),), (pv(1, lo), pv(3, lo, PV_STOP)), (pv(-1, lo),), (pv(2, lo, h=PRE_HANDLE[0]),)]
    letters = [(m, BNUM, me, 0, p) for m in mem for p in menu]
    letters += [(NON_MEMBER, BNUM, me, 0, menu[1]),          # a non-member in my ballot
                (mem[0], BNUM + 1, mem[0], 0, ()),           # a higher ballot from a member
                (NON_MEMBER, BNUM + 1, NON_MEMBER, 0, ()),   # ... and from a non-member
                (mem[-1], BNUM - 1, me, 0, menu[1]),         # a lower ballot number
                (mem[-1], BNUM, me - 1, 0, menu[1])]         # a lower coordinator id
    if extended:
        # (slot S0 + 3 in the LOW ballot again, as another request: between two pvalues of one slot and one ballot the
        # first to arrive stays - `>` in the pmax update, PCS:345-368 - so its order with the stop at S0 + 3 shows)
        letters += [(mem[-1], BNUM, me, -1, (pv(3, lo, PV_NOOP, h=pv_handle(3, lo) + 50),)),
                    (mem[-1], BNUM, me, 1, (pv(2, hi, h=PRE_HANDLE[0]),)),
                    (mem[0], BNUM, me, -1, ())]
    if sixth:
        letters += [(mem[0], BNUM, me, 0, (pv(4, lo),))]     # a sixth slot: S0 + 4 meets S0 in a ring of four
    return letters


# ---- the engine's limits, from include/gpx.h ----------------------------------------------------------------------------
def clone(c):
    d = Candidate(c.K, c.my, c.next)
    d.node_slots, d.carry, d.heard, d.proposals = list(c.node_slots), dict(c.carry), list(c.heard), dict(c.proposals)
    d.active, d.exists = c.active, c.exists
    return d


def recorded_slots(c, j, first, pvs):
    """nodeSlotNumbers after recordSlotNumber(preply) of member j (PrepareReplyPacket.getMinSlot; PCS:786-803)"""
    ns = list(c.node_slots)
    min_slot = first
    for s_, _, _, _ in pvs:
        if s_ - min_slot < 0:
            min_slot = s_
    if ns[j] - min_slot < 0:
        ns[j] = min_slot
    return ns


def engine_refusal(c, reply, W):
    """What the engine cannot do with a reply the reading would count (candidate c BEFORE the reply; reply = (member
    index, first slot, [(slot, ballot, handle, stop)]), slots as I32) -> None | 'clash' | 'span' | 'length'.

      clash   carried pvalues live at ring index slot mod W: two slots of the reply, or one of the reply and one already
              carried, that differ and share an index.  The reply is dropped whole: V_IGNORED + GPX_S_WINDOW
      span    with this reply a majority has answered, and the carried range max(nodeSlotNumbers) .. highest carried slot
              is longer than W slots - or the two are exactly 2^31 apart, where the reference's loop would never end
      length  the range fits, but with the pre-actives proposed again behind it (and processStop's new stop) the
              proposal list spans more than W slots
    span and length: the reply counts (V_RECORDED + GPX_S_WINDOW: heard-from mask, nodeSlotNumbers and carried pvalues
    keep it) but the coordinator does not become active."""
    j, first, pvs = reply
    ring = {}
    for s_ in list(c.carry) + [p[0] for p in pvs]:
        if ring.setdefault(int(s_) & (W - 1), int(s_)) != int(s_):
            return "clash"
    if sum(c.heard) + 1 <= c.K // 2:
        return None
    keys = set(c.carry) | {p[0] for p in pvs}
    if not keys:
        return None
    max_carry = wraparound_max(sorted(keys))
    max_min = wraparound_max(recorded_slots(c, j, first, pvs))
    R = I32(max_carry) - max_min
    if R >= W or int(R) == -2 ** 31:
        return "span"
    d = clone(c)
    kind, _, _ = d.prepare_reply(j, c.my, first - 1, pvs)
    assert kind == "elected"
    lo = max_min if R >= 0 else max_carry + 1
    return "length" if d.next - lo > W else None


def record_only(c, j, first, pvs):
    """What a reply refused for span or length leaves: isPrepareAcceptedByMajority's bookkeeping, nothing else."""
    c.node_slots = recorded_slots(c, j, first, pvs)
    for s_, b, h, stop in pvs:
        if s_ not in c.carry or b > c.carry[s_][0]:
            c.carry[s_] = (b, h, stop)
    c.heard[j] = True


# ---- one group against the reading --------------------------------------------------------------------------------------
class Stats:
    def __init__(self, L):
        self.kinds = [dict.fromkeys(VMAP, 0) for _ in range(L)]     # per arrival position
        self.entries = dict.fromkeys(KMAP, 0)
        self.refused = dict(clash=0, span=0, length=0)
        self.groups = self.groups_refused = self.after_refusal = 0
        self.elected = self.preempted = self.dup_dropped = self.dup_kept = self.replaced = self.both_sides = self.pre_both_sides = 0
        self.records = self.kernels = self.driver = None
        self.outcome = None

    def summary(self):
        return dict(groups=self.groups, elected=self.elected, preempted=self.preempted, refused=dict(self.refused),
                    groups_refused=self.groups_refused)


def walk(K, W, S0, mem, shape, replies, st, me=ME):
    """The reading (and engine_refusal) over one group's replies -> (candidate at the end, per reply the expected
    (v_kind, status, median, entry list | None)).  replies: (acceptor id, (bnum, bcoord), first slot, pvalues as the
    engine takes them)."""
    c = Candidate(K, (BNUM, me), I32(S0))
    for i in range(shape[0]):
        assert c.propose(PRE_HANDLE[i], shape[1] and i == shape[0] - 1) is not None
    idx = {m: j for j, m in enumerate(mem)}
    want, was_refused, after = [], False, False
    for pos, (acc, rb, first, pvs) in enumerate(replies):
        first = I32(first)
        rp = [(I32(s_), (b0, b1), h, bool(fl & PV_STOP)) for s_, b0, b1, h, fl in pvs]
        j = idx.get(acc)
        status, refusal = S_OK, None
        if j is None:
            # a non-member: isPreemptable looks at the ballot only; otherwise canIgnorePrepareReply
            out = c.prepare_reply(0, rb, first - 1, rp) if rb > c.my else ("ignored", 0, [])
        else:
            if c.exists and not c.active and rb == c.my and not c.heard[j]:
                refusal = engine_refusal(c, (j, first, rp), W)
                st.replaced += any(s_ in c.carry and b > c.carry[s_][0] for s_, b, _, _ in rp)
            if refusal == "clash":
                out, status = ("ignored", 0, []), S_WINDOW
            elif refusal:
                record_only(c, j, first, rp)
                out, status = ("recorded", 0, []), S_WINDOW
            else:
                pre = dict(c.proposals)
                out = c.prepare_reply(j, rb, first - 1, rp)
                if out[0] == "elected" and c.carry:
                    carried = {h for _, h, _ in c.carry.values()}
                    kept = {h for _, k_, h, _ in out[2] if k_ == "preactive"}
                    for s_, (_, h, _) in pre.items():
                        if h in carried and s_ not in c.carry:
                            st.dup_kept += h in kept
                            st.dup_dropped += h not in kept
        if refusal:
            st.refused[refusal] += 1
            was_refused = True
        elif was_refused and out[0] in ("elected", "preempted"):
            after = True
        kind, med, lst = out
        st.kinds[pos][kind] += 1
        if kind in ("elected", "preempted"):
            for _, k_, _, _ in lst:
                st.entries[k_] += 1
            pre_slots = [s_ for s_, k_, _, _ in lst if k_ == "preactive"]
            st.pre_both_sides += bool(pre_slots) and min(pre_slots) < 0 <= max(pre_slots)
            if kind == "elected":
                st.elected += 1
                st.both_sides += bool(lst) and min(s_ for s_, _, _, _ in lst) < 0 <= max(s_ for s_, _, _, _ in lst)
            else:
                st.preempted += 1
        want.append((VMAP[kind], status, int(med), [(int(s_), KMAP[k_], h, stop) for s_, k_, h, stop in lst]))
    st.groups += 1
    st.groups_refused += was_refused
    st.after_refusal += after
    return c, want


# ---- the batches ----------------------------------------------------------------------------------------------------------
def layout(G, L, form, flip=False):
    """The calls of a form: [(group of each record, arrival position of each record)]."""
    g = np.arange(G, dtype=np.int32)
    if form == "per-step":
        return [(g, np.full(G, p, np.int32)) for p in range(L)]
    far = np.random.default_rng(LAYOUT_SEED).random(G) < 0.5
    if flip:
        far = ~far
    gf, gn = g[far], g[~far]
    parts = [(gf, np.zeros(gf.shape[0], np.int32))]
    full = gn.shape[0] // NEAR * NEAR
    for blk in (gn[:full].reshape(-1, NEAR), gn[full:].reshape(1, -1)):
        nb, B = blk.shape
        parts.append((np.repeat(blk[:, None, :], L, axis=1).reshape(-1),
                      np.broadcast_to(np.arange(L, dtype=np.int32)[None, :, None], (nb, L, B)).reshape(-1)))
    parts += [(gf, np.full(gf.shape[0], p, np.int32)) for p in range(1, L)]
    return [(np.concatenate([p[0] for p in parts]).astype(np.int32), np.concatenate([p[1] for p in parts]).astype(np.int32))]


def check_layout(calls, G, L):
    """Every (group, position) once, every group's positions in order; -> the smallest and largest distance between
    two consecutive records of one group inside a call."""
    seen = np.zeros((G, L), np.int64) - 1
    k = 0
    for g, p in calls:
        assert (seen[g, p] == -1).all()
        seen[g, p] = k + np.arange(g.shape[0])
        k += g.shape[0]
    assert (seen >= 0).all() and (np.diff(seen, axis=1) > 0).all()
    d = np.diff(seen, axis=1)
    return int(d.min()), int(d.max())


# ---- the device-pointer form ----------------------------------------------------------------------------------------------
OUT_SENTINEL = 0x5A


class ElectDevEngine(DevEngine):
    """DevEngine with the view change's two *_dev calls; they answer like Engine.election_begin / prepare_reply."""

    def election_begin(self, gidx, bnum):
        g = np.ascontiguousarray(gidx, np.int32)
        n = g.shape[0]
        gd, bd, st = self._dev(g), self._dev(np.array(np.broadcast_to(np.asarray(bnum, np.int32), (n,)))), self._z(n, True)
        self._begin()
        self.e.call_dev("election_begin", n, gd.data_ptr(), bd.data_ptr(), st.data_ptr())
        self._finish(None)
        return st.cpu().numpy()[:n]

    def prepare_reply_raw(self, cols, off, pv_total, pv, poison=None, guard=16):
        """gpx_prepare_reply_batch_dev on the five record columns `cols`, the offsets as given (not validated: that is
        the kernel's business) and the pvalue columns pv = (slot, bnum, bcoord, handle | None, flags | None), each
        allocated with exactly pv_total entries between two bands of `guard` entries holding `poison` (one pvalue).
        The eight outputs are filled with OUT_SENTINEL before the call.  -> {name: array}."""
        t = self.t
        n = cols[0].shape[0]
        W = int(self.e.cfg.window)
        dc = [self._dev(c, np.int32) for c in cols] + [self._dev(off, np.int32)]
        dts = (np.int32, np.int32, np.int32, np.int64, np.uint8)
        dp, ptrs = [], []
        for i, (a, dt) in enumerate(zip(pv, dts)):
            if a is None:
                dp.append(None), ptrs.append(0)
                continue
            a = np.ascontiguousarray(a, dt)[:pv_total]
            band = np.full(guard, 0 if poison is None else poison[i], dt)
            x = self._dev(np.concatenate([band, a, band]))
            dp.append(x), ptrs.append(x.data_ptr() + guard * np.dtype(dt).itemsize)
        q = max(n, 1)
        shapes = dict(v_kind=(q, t.uint8), e_count=(q, t.int32), e_median=(q, t.int32), e_slot=(q * W, t.int32),
                      e_kind=(q * W, t.uint8), e_handle=(q * W, t.int64), e_flags=(q * W, t.uint8), status=(q, t.uint8))
        out = {}
        for nm, (m, dt) in shapes.items():
            out[nm] = t.empty(m, dtype=dt, device="cuda")
            out[nm].view(t.uint8).fill_(OUT_SENTINEL)
        self._begin()
        vp = lambda p: C.c_void_p(int(p)) if p else None   # noqa: E731  (call_dev takes pointers only: pv_total is an int)
        self.e.lib.check(self.e.lib.fn["prepare_reply_batch_dev"](
            self.e.h, n, *[vp(c.data_ptr()) for c in dc], int(pv_total), *[vp(p) for p in ptrs],
            *[vp(out[nm].data_ptr()) for nm in shapes]), "prepare_reply_batch_dev")
        self._finish(None)
        for x, (a, dt) in zip(dp, zip(pv, dts)):   # the columns and their bands are inputs: untouched
            if x is not None:
                h = x.cpu().numpy()
                assert (h[guard:guard + pv_total] == np.ascontiguousarray(a, dt)[:pv_total]).all()
                assert (h[:guard] == h[0]).all() and (h[guard + pv_total:] == h[0]).all()
        return {nm: x.cpu().numpy() for nm, x in out.items()}

    def prepare_reply(self, gidx, acceptor, r_bnum, r_bcoord, first_slot, pvalues=None):
        g = np.ascontiguousarray(gidx, np.int32)
        n = g.shape[0]
        off, pv = flatten(pvalues if pvalues is not None else [[] for _ in range(n)])
        cols = [g] + [np.array(np.broadcast_to(np.asarray(x, np.int32), (n,))) for x in (acceptor, r_bnum, r_bcoord, first_slot)]
        r = self.prepare_reply_raw(cols, off, int(off[-1]), pv)
        return answer(r, n)


def flatten(pvalues):
    """(pv_off, (slot, bnum, bcoord, handle, flags)) of per-record lists of pvalue tuples."""
    off = np.zeros(len(pvalues) + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p in pvalues])
    flat = np.array([t_ for p in pvalues for t_ in p], np.int64).reshape(-1, 5)
    return off, (flat[:, 0].astype(np.int32), flat[:, 1].astype(np.int32), flat[:, 2].astype(np.int32), flat[:, 3].copy(),
                 flat[:, 4].astype(np.uint8))


def answer(r, n):
    """Engine.prepare_reply's answer from the eight output columns."""
    es, ek, eh, ef, ec = r["e_slot"], r["e_kind"], r["e_handle"], r["e_flags"], r["e_count"]
    lists = [[(int(es[j * n + i]), int(ek[j * n + i]), int(eh[j * n + i]), int(ef[j * n + i])) for j in range(int(ec[i]))]
             for i in range(n)]
    return (r["v_kind"][:n], r["e_median"][:n], r["status"][:n]), lists


class HostAsElectDev:
    """A library's host calls behind prepare_reply_raw (the CPU model's stand-in for the device form): include/gpx.h's
    sentence about the _dev twin - a record whose slice falls outside [0, pv_total] is refused with GPX_S_WINDOW -
    applied before the host call, which takes the remaining records with the pvalues their slices name."""

    def __init__(self, e):
        self.e, self.kernels, self.launches, self.refused = e, [], {}, 0

    def __getattr__(self, name):
        return getattr(self.e, name)

    def counters(self):
        c = self.e.counters()
        return c[:2] + (c[2] + self.refused,) + c[3:]

    def prepare_reply_raw(self, cols, off, pv_total, pv, poison=None, guard=16):
        n = cols[0].shape[0]
        W = int(self.e.cfg.window)
        r = dict(v_kind=np.zeros(n, np.uint8), e_count=np.zeros(n, np.int32), e_median=np.zeros(n, np.int32),
                 e_slot=np.full(n * W, 0x5A5A5A5A, np.int32), e_kind=np.full(n * W, OUT_SENTINEL, np.uint8),
                 e_handle=np.full(n * W, 0x5A5A5A5A5A5A5A5A, np.int64), e_flags=np.full(n * W, OUT_SENTINEL, np.uint8),
                 status=np.zeros(n, np.uint8))
        good, pvs = slices(off, pv_total, pv)
        r["status"][~good] = S_WINDOW
        self.refused += int((~good).sum())
        gi = np.nonzero(good)[0]
        if gi.shape[0]:
            (vk, em, st), lists = self.e.prepare_reply(*[c[gi] for c in cols], [pvs[i] for i in gi.tolist()])
            r["v_kind"][gi], r["e_median"][gi], r["status"][gi] = vk, em, st
            for q, i in enumerate(gi.tolist()):
                r["e_count"][i] = len(lists[q])
                for j, (s_, k_, h, fl) in enumerate(lists[q]):
                    r["e_slot"][j * n + i], r["e_kind"][j * n + i], r["e_handle"][j * n + i], r["e_flags"][j * n + i] = s_, k_, h, fl
        return r


def slices(off, pv_total, pv):
    """Per record: is its slice inside [0, pv_total], and the pvalue tuples it names (NULL handle / flags columns: 0)."""
    off = np.asarray(off, np.int64)
    o, m = off[:-1], off[1:] - off[:-1]
    good = (o >= 0) & (m >= 0) & (o + m <= pv_total)
    ps, pb, pc, ph, pf = pv
    pvs = [[(int(ps[x]), int(pb[x]), int(pc[x]), int(ph[x]) if ph is not None else 0, int(pf[x]) if pf is not None else 0)
            for x in range(int(o[i]), int(o[i] + m[i]))] if good[i] else None for i in range(o.shape[0])]
    return good, pvs


REFERENCE = {}   # key of a leg -> (Stats, per group (expected answers, the candidate at the end)): the reading, walked once


# ---- A.1: the enumeration ---------------------------------------------------------------------------------------------------
def cases(K, L, extended=True, sample=None, sixth=False):
    """(letters, shape index of each group, letter indices of each group [G][L]); sample = (groups, seed)"""
    letters = alphabet(K, extended, sixth=sixth)
    A = len(letters)
    total = len(SHAPES) * A ** L
    ids = np.arange(total, dtype=np.int64)
    if sample is not None and sample[0] < total:
        ids = np.sort(np.random.default_rng(sample[1]).choice(total, sample[0], replace=False))
    seq = np.stack([(ids // A ** (L - 1 - p)) % A for p in range(L)], axis=1).astype(np.int32)
    return letters, (ids // A ** L).astype(np.int32), seq


def make_engine(lib, K, W, G, S0, max_batch, members=None, kmax=None, me=ME):
    mem = members or MEMBERS[K]
    e = Engine(lib, me, G, kmax=kmax or K, window=W, max_batch=max_batch)
    s0, gc = int(I32(S0)), int(I32(S0) - 2)
    kk = kmax or K
    marr = np.zeros((G, kk), np.int32)
    marr[:, :K] = np.array(mem, np.int32)
    assert (e.create_groups(np.arange(G), marr, K, plain_rows(G, s0, 0, mem[0], gc=gc)) == S_OK).all()
    return e


def run_scripts(lib, K, W, S0, mem, shapes, scripts, calls, dev=False, kmax=None, engine=None, groups=None, me=ME, key=None,
                driver=None):
    """Group x has pre-active shape shapes[x] and gets scripts(x, pos) = (acceptor, (bnum, bcoord), first slot, pvalues)
    as its reply number pos; `calls` (layout) says which records go into which call.  Everything the engine answers is
    held against walk().  engine / groups: a living engine and the (fresh) group indices to use in it; driver(engine):
    what answers election_begin and prepare_reply in the engine's place (dev: ElectDevEngine)."""
    G = len(shapes)
    L = max(int(p.max()) for _, p in calls) + 1
    e = engine or make_engine(lib, K, W, G, S0, max(n_.shape[0] for n_, _ in calls) + 64, mem, kmax, me)
    gmap = np.arange(G, dtype=np.int32) if groups is None else np.asarray(groups, np.int32)
    drv = driver(e) if driver else (ElectDevEngine(e) if dev else e)
    drops0 = e.counters()[2]
    try:
        assert (drv.election_begin(gmap, np.full(G, BNUM, np.int32)) == EB_PREPARING).all()
        for i in range(3):
            sel = np.array([x for x in range(G) if shapes[x][0] > i], np.int32)
            if sel.shape[0] == 0:
                continue
            stop = np.array([shapes[x][1] and i == shapes[x][0] - 1 for x in sel.tolist()], np.uint8)
            sl, bn, bc, _, ps = e.propose(gmap[sel], stop, handle=np.full(sel.shape[0], PRE_HANDLE[i], np.int64))
            assert (ps == S_PREACTIVE).all() and (sl == int(I32(S0) + i)).all() and (bn == BNUM).all() and (bc == me).all()
        got = {}
        for g, p in calls:
            recs = [scripts(int(x), int(q)) for x, q in zip(g.tolist(), p.tolist())]
            (vk, em, rs), lists = drv.prepare_reply(gmap[g], [r[0] for r in recs], [r[1][0] for r in recs], [r[1][1] for r in recs],
                                                    [int(I32(r[2])) for r in recs], [r[3] for r in recs])
            vk, em, rs = vk.tolist(), em.tolist(), rs.tolist()
            for i, (x, q) in enumerate(zip(g.tolist(), p.tolist())):
                got[(x, q)] = (vk[i], rs[i], em[i], lists[i])
        # ---- every reply against the reading (computed once per `key`, shared by the forms of a leg) ----
        ref = REFERENCE.get(key)
        if ref is None:
            st0, s0, exp = Stats(L), int(I32(S0)), []
            for x in range(G):
                c, want = walk(K, W, S0, mem, shapes[x], [scripts(x, q) for q in range(L)], st0, me)
                exp.append((want, (c.exists, c.active, int(c.next), [int(v) for v in c.node_slots],
                                   sum(1 << j for j, h in enumerate(c.heard) if h), s0 in c.proposals,
                                   bool(c.proposals[s0][2]) if s0 in c.proposals else False, int(c.median()))))
            ref = (st0, exp)
            if key is not None:
                REFERENCE[key] = ref
        st = copy.copy(ref[0])
        outcome = []
        for x, (want, _) in enumerate(ref[1]):
            res = None
            for q in range(L):
                vk, rs, em, lst = got[(x, q)]
                wk, ws, wm, wl = want[q]
                if (vk, rs) != (wk, ws) or em != (wm if wk == V_ELECTED else 0):
                    raise AssertionError(f"group {x} (shape {shapes[x]}) reply {q} of {[scripts(x, i) for i in range(L)]}: the reading "
                                         f"says {VNAME[wk]}, status {ws}, median {wm}; the engine {VNAME.get(vk, vk)}, status {rs}, median {em}")
                lst = [(s_, k_, h if k_ in (E_CARRY, E_PREACTIVE) else 0, bool(fl & PV_STOP)) for s_, k_, h, fl in lst]
                assert lst == wl, f"group {x} (shape {shapes[x]}) reply {q} of {[scripts(x, i) for i in range(L)]}: the reading lists {wl}; the engine {lst}"
                if wk in (V_ELECTED, V_PREEMPTED):
                    res = (wk, wm, tuple(wl))
            outcome.append(res)
        st.outcome = outcome
        # ---- the rows and the pokes after the last reply ----
        snap, sst = e.snapshot(gmap)
        pk, sl, bn, bc, md, fl, hd, pst = e.poke_scan(gmap)
        assert (sst == S_OK).all() and (pst == S_OK).all()
        s0 = int(I32(S0))
        rows = zip(snap["has_coord"].tolist(), snap["coord_bnum"].tolist(), snap["coord_bcoord"].tolist(),
                   snap["next_proposal_slot"].tolist(), snap["node_slots"][:, :K].tolist())
        pokes = zip(pk.tolist(), sl.tolist(), bn.tolist(), bc.tolist(), md.tolist(), fl.tolist(), hd.tolist())
        none = (POKE_NONE, 0, 0, 0, 0, 0, 0)
        for x, (row, poke, (_, fin)) in enumerate(zip(rows, pokes, ref[1])):
            exists, active, nxt, ns, heard, head, head_stop, median = fin
            what = f"group {x} after its last reply"
            if not exists:                                     # PISM.handlePrepareReply: this.coordinator = null
                assert row[0] == 0 and poke == none, (what + " (preempted)", row, poke)
            elif not active:
                # the row is a HotRestoreInfo: getBallotIfActive & co. (PISM:2015-2018) show an ACTIVE coordinator only;
                # the heard-from mask of the one that is still preparing comes with the poke
                assert row[0] == 0 and row[3] == -1, (what, row)
                assert poke == (POKE_PREPARE, s0, BNUM, me, 0, 0, heard), (what, poke)
            else:
                assert row == (1, BNUM, me, nxt, ns), (what, row, nxt, ns)
                # isCommandering(the acceptor's slot): its ACCEPT again, with the median as it is now
                assert poke == ((POKE_ACCEPT, s0, BNUM, me, median, PV_STOP if head_stop else 0, 0) if head else none), (what, poke)
        assert e.counters()[2] - drops0 == sum(st.refused.values()), "counters()[2]: one per refused reply"
        if drv is not e:
            st.kernels, st.driver = dict(getattr(drv, "launches", {})), drv
        st.records = sum(g.shape[0] for g, _ in calls)
    finally:
        if engine is None:
            e.close()
    return st


def run_enum(lib, K, W, L, base, form, extended=True, sample=None, flip=False, engine=None, groups=None, profile=False,
             driver=None):
    """One engine, one group per (pre-active shape, letter sequence); -> Stats."""
    S0 = BASES[base]
    letters, shape_of, seq = cases(K, L, extended, sample, sixth=W < 8)   # (the W = 4 leg: see alphabet)
    G = seq.shape[0]
    table = [(a, (rb, rc), S0 + fo, [(int(I32(S0) + off), b0, b1, h, fl) for off, b0, b1, h, fl in pvs])
             for a, rb, rc, fo, pvs in letters]
    shapes = [SHAPES[s] for s in shape_of.tolist()]
    seq_l = seq.tolist()
    calls = layout(G, L, "one-call" if form == "dev" else form, flip)
    prof = None
    if profile and engine is None and form != "dev":
        engine = make_engine(lib, K, W, G, S0, max(g.shape[0] for g, _ in calls) + 64)
        engine.profile(2)
        prof = engine
    try:
        st = run_scripts(lib, K, W, S0, MEMBERS[K], shapes, lambda x, q: table[seq_l[x][q]], calls, dev=form == "dev",
                         engine=engine, groups=groups, key=(K, W, L, base, extended, sample), driver=driver)
        if prof is not None:
            st.kernels = {k: v[0] for k, v in prof.profile_read().items()}
    finally:
        if prof is not None:
            prof.close()
    st.seq, st.alphabet = seq, len(letters)
    return st


def reversal_share(st, L):
    """Full enumerations only: the share of groups whose outcome (elected or preempted, median, entry list) differs from
    that of the group with the same shape and the letters in reverse order."""
    seq, A = st.seq, st.alphabet
    G = seq.shape[0]
    assert G == len(SHAPES) * A ** L
    ids = np.arange(G, dtype=np.int64)
    rev = (ids // A ** L) * A ** L + sum(seq[:, p].astype(np.int64) * A ** p for p in range(L))
    return sum(st.outcome[x] != st.outcome[int(r)] for x, r in enumerate(rev.tolist())) / G


# ---- A.3: sixteen members ---------------------------------------------------------------------------------------------------
MEMBERS16 = [3 + (i << 20) for i in range(16)]
SEED16 = 1609


def run_sixteen(lib, W=8, base="plain", G=48, dev=False):
    """kmax = 16, sixteen members with ids 2^20 apart, the candidate among them: per group a seeded order of nine
    distinct members - index 15 among the first eight, a second reply of index 15 before the ninth - so that the
    majority (more than k / 2 = 8) is reached exactly at the ninth distinct member, the tenth reply of the script; an
    eleventh, of a tenth member, comes too late."""
    rng = np.random.default_rng(SEED16)
    S0, me = BASES[base], MEMBERS16[4]
    menu = alphabet(16, False, MEMBERS16, me)[:6]
    scripts = []
    for x in range(G):
        others = [int(j) for j in rng.permutation(15)]     # indices 0 .. 14
        order = others[:8]
        at = int(rng.integers(0, 8))
        order.insert(at, 15)                               # index 15 among the first eight distinct members
        order.insert(int(rng.integers(at + 1, 9)), 15)     # ... and again, before the ninth distinct one
        order.append(others[8])
        assert len(order) == 11 and len(set(order[:9])) == 8 and len(set(order[:10])) == 9 and order[9] != 15
        rs = []
        for j in order:
            pvs = menu[int(rng.integers(0, 6))][4]
            rs.append((MEMBERS16[j], (BNUM, me), S0, [(int(I32(S0) + off), b0, b1, h, fl) for off, b0, b1, h, fl in pvs]))
        scripts.append(rs)
    shapes = [SHAPES[x % len(SHAPES)] for x in range(G)]
    st = run_scripts(lib, 16, W, S0, MEMBERS16, shapes, lambda x, q: scripts[x][q], layout(G, 11, "one-call"), dev=dev, kmax=16,
                     me=me)
    assert st.kinds[9]["elected"] == G and st.kinds[10]["ignored"] == G and st.elected == G
    return st


# ---- B.2: what only a device-pointer caller can hand over -------------------------------------------------------------------
DB_TABLE = 16384                      # max_groups of the engine; groups with index % 97 == 13 are never created
DB_SEED = 4177
POISON = (5, 1, 5000, 777, PV_STOP)   # the bands around the pvalue columns: slot S0 in the higher ballot, a stop
PLANES = ("e_slot", "e_kind", "e_handle", "e_flags")


def scatter_tile():
    """Records of one workgroup of the bucket front end's scatter: the smallest tile geometry_common knows."""
    from tests.geometry_common import TILE_CANDIDATES
    return min(T for (T, _), _ in TILE_CANDIDATES)


def db_engines(lib_a, lib_o, dev):
    """(driver a, oracle o): the same table in both, every existing group's candidate preparing, a pre-active in every third."""
    S0, mem = BASES["plain"], MEMBERS[3]
    gone = np.arange(13, DB_TABLE, 97, dtype=np.int32)
    rest = np.setdiff1d(np.arange(DB_TABLE, dtype=np.int32), gone).astype(np.int32)
    ea, eo = (Engine(lib, ME, DB_TABLE, kmax=3, window=8, max_batch=3 * DB_TABLE) for lib in (lib_a, lib_o))
    for e in (ea, eo):
        m = rest.shape[0]
        assert (e.create_groups(rest, np.tile(np.array(mem, np.int32), (m, 1)), 3, plain_rows(m, S0, 0, mem[0], gc=S0 - 2)) == S_OK).all()
        assert (e.election_begin(rest, np.full(rest.shape[0], BNUM, np.int32)) == EB_PREPARING).all()
        sl, _, _, _, ps = e.propose(rest[::3], np.zeros(rest[::3].shape[0], np.uint8),
                                    handle=np.full(rest[::3].shape[0], PRE_HANDLE[0], np.int64))
        assert (ps == S_PREACTIVE).all()
    return (ElectDevEngine(ea) if dev else HostAsElectDev(ea)), eo, rest


def db_check(a, eo, cols, off, pv_total, pv, what, expect_bad=None):
    """One raw call on a, the oracle's host call on the records whose slices lie inside [0, pv_total] (with the pvalues
    those slices name): every record's answer, the untouched planes, the state of every group named, the drop counter.
    -> (answer of a, bad records)."""
    n = cols[0].shape[0]
    W = int(eo.cfg.window)
    ca, co = a.counters()[2], eo.counters()[2]
    r = a.prepare_reply_raw(cols, off, pv_total, pv, poison=POISON)
    good, pvs = slices(off, pv_total, pv)
    bad = np.nonzero(~good)[0]
    if expect_bad is not None:
        assert bad.tolist() == sorted(expect_bad), (what, bad.tolist(), sorted(expect_bad))
    gi = np.nonzero(good)[0]
    (vk, em, st), lists = eo.prepare_reply(*[c[gi] for c in cols], [pvs[i] for i in gi.tolist()])
    (avk, aem, ast), alists = answer(r, n)
    assert avk[gi].tolist() == vk.tolist() and aem[gi].tolist() == em.tolist() and ast[gi].tolist() == st.tolist(), what
    assert [alists[i] for i in gi.tolist()] == lists, what + ": entry lists"
    # a refused slice: V_IGNORED + GPX_S_WINDOW, nothing listed, counted
    assert (avk[bad] == V_IGNORED).all() and (ast[bad] == S_WINDOW).all(), (what, avk[bad].tolist(), ast[bad].tolist())
    assert (r["e_count"][bad] == 0).all() and (r["e_median"][bad] == 0).all(), what
    assert a.counters()[2] - ca == eo.counters()[2] - co + bad.shape[0], what + ": counters()[2]"
    # records of groups outside the table, or of no group: the dense outputs are written as 0, not left alone
    out = np.nonzero(st != S_OK)[0]
    out = gi[out[st[out] == S_NOGROUP]]
    assert (r["v_kind"][out] == 0).all() and (r["e_count"][out] == 0).all() and (r["e_median"][out] == 0).all(), what
    # the kernel writes what it lists and nothing else: planes j >= e_count[i] are as they were before the call
    cnt = r["e_count"][:n].astype(np.int64)
    assert (cnt >= 0).all() and (cnt <= W).all(), what
    untouched = np.arange(W)[:, None] >= cnt[None, :]
    for nm in PLANES:
        plane = r[nm][:W * n].reshape(W, n)
        fill = np.frombuffer(bytes([OUT_SENTINEL]) * plane.dtype.itemsize, plane.dtype)[0]
        assert (plane[untouched] == fill).all(), f"{what}: {nm} written beyond e_count"
    named = np.unique(cols[0])
    if named.shape[0] > 600:   # (the tile-sized calls: the groups of the first and last records and every 16th between)
        named = np.unique(np.concatenate([named[:8], named[::16], named[-8:]]))
    for g in named.tolist():
        if 0 <= g < DB_TABLE and g % 97 != 13:
            assert a.dump(g).tolist() == eo.dump(g).tolist(), f"{what}: state of group {g}"
    return r, bad


def db_batch(groups, rng, with_strangers=False):
    """Three replies per group (its members in a seeded order, a seeded menu entry each), blocks of NEAR groups, arrival
    position by position inside a block.  -> (cols, per-record pvalues, index of record (group k of block b, position p))"""
    S0, mem = BASES["plain"], MEMBERS[3]
    menu = [[(S0 + off, b0, b1, h, fl) for off, b0, b1, h, fl in l[4]] for l in alphabet(3)[:6]]
    assert groups.shape[0] % NEAR == 0
    blk = groups.reshape(-1, NEAR)
    g = np.repeat(blk[:, None, :], 3, axis=1).reshape(-1).astype(np.int32)
    n = g.shape[0]
    order = np.stack([rng.permutation(3) for _ in range(groups.shape[0])]).reshape(-1, NEAR, 3).transpose(0, 2, 1).reshape(-1)
    acc = np.array(mem, np.int32)[order]
    pvalues = [menu[int(x)] for x in rng.integers(1, 6, n)]
    if with_strangers:      # a group beyond the table, a negative index, a group that does not exist: in every fourth
        at0 = np.arange(1, blk.shape[0], 4) * 3 * NEAR   # block, in place of the first reply of its first group
        g[at0] = np.resize(np.array([DB_TABLE + 5, -1, 13 + 97, 2 ** 31 - 1, -2 ** 31, 13, DB_TABLE], np.int32), at0.shape[0])
    cols = [g, acc, np.full(n, BNUM, np.int32), np.full(n, ME, np.int32), np.full(n, S0, np.int32)]
    return cols, pvalues, lambda b, k, p: b * 3 * NEAR + p * NEAR + k


def run_device_branches(lib_a, lib_o, dev, legs=None):
    """-> {leg: bad records}"""
    a, eo, rest = db_engines(lib_a, lib_o, dev)
    rng = np.random.default_rng(DB_SEED)
    seen = {}
    cursor = 0

    def fresh(m):
        nonlocal cursor
        out = rest[cursor:cursor + m]
        cursor += m
        assert out.shape[0] == m
        return out
    try:
        # ---- slices the host twin would refuse ----
        for leg in ("last slice ends at pv_total", "last slice ends at pv_total + 1"):
            cols, pvalues, at = db_batch(fresh(300), rng, with_strangers=True)
            n = cols[0].shape[0]
            off, pv = flatten(pvalues)
            total = int(off[-1])
            expect = set()
            nb = n // (3 * NEAR)
            for b in range(nb):
                # the middle reply of group 2 of the block (of group 4 in the last block: the call's last record, that
                # group's third reply, must still meet a preparing candidate); the record in front ends where it starts
                i = at(b, 4 if b == nb - 1 else 2, 1)
                kind = b % 3
                if kind == 0:
                    off[i] = -1 - (b % 5)                       # a negative offset (record i), a descending pair (i - 1)
                elif kind == 1 and off[i - 1] >= 1:
                    off[i] = off[i - 1] - 1                     # a descending pair; record i: a longer slice, inside
                    expect.add(i - 1)
                    continue
                else:
                    off[i] = total + 1 + (b % 2)                # past the end (record i - 1), descending from there (i)
                expect |= {i - 1, i}
            if leg.endswith("+ 1"):
                off[n] = total + 1
                expect.add(n - 1)
            assert len(pvalues[n - 1]) > 0 and cols[0][n - 1] >= 0
            _, bad = db_check(a, eo, cols, off, total, pv, leg, expect)
            seen[leg] = bad.shape[0]
        # ---- pvalues without handles, without flags, without both ----
        for leg, (nh, nf) in (("pv_handle NULL", (True, False)), ("pv_flags NULL", (False, True)), ("both NULL", (True, True))):
            cols, pvalues, _ = db_batch(fresh(100), rng)
            off, pv = flatten(pvalues)
            assert pv[3].any() and pv[4].any()
            pv = (pv[0], pv[1], pv[2], None if nh else pv[3], None if nf else pv[4])
            db_check(a, eo, cols, off, int(off[-1]), pv, leg, set())
            seen[leg] = 0
        # ---- one record; one below, at and one above the scatter's tile ----
        T = scatter_tile()
        S0 = BASES["plain"]
        for n in (1, T - 1, T, T + 1):
            g = fresh(n)
            pvalues = [[(S0 + 1, 0, 7, 60_000 + i, 0), (S0 + 3, 1, 5000, 70_000 + i, PV_STOP)] for i in range(n)]
            off, pv = flatten(pvalues)
            cols = [g.astype(np.int32), np.full(n, 7, np.int32), np.full(n, BNUM, np.int32), np.full(n, ME, np.int32),
                    np.full(n, S0, np.int32)]
            r, _ = db_check(a, eo, cols, off, int(off[-1]), pv, f"n = {n}", set())
            assert (r["v_kind"][:n] == V_RECORDED).all()
            # ... and the second member's reply elects every one of them, the last record's list included
            cols[1] = np.full(n, 5000, np.int32)
            r, _ = db_check(a, eo, cols, off, int(off[-1]), pv, f"n = {n}, second replies", set())
            assert (r["v_kind"][:n] == V_ELECTED).all() and (r["e_count"][:n] >= 3).all()
            seen[f"n = {n}"] = 0
        return seen, getattr(a, "launches", {})
    finally:
        a.e.close(), eo.close()
