"""Streams for the regular round of the tiled accept-reply kernels (the `if constexpr (TW)` block of bucket16_body,
gigapaxos_amd/csrc/gpx_ar16.hip.h), and what keeps them honest.

The two-word staging rebuilds the arrival order of a group's votes from a key (tile, offset in the tile), a rank that an
LDS atomic returns and a sorting network in registers.  The order shows in the result in ONE place: getMedianMinus is
taken at the vote that completes the majority, over nodeSlotNumbers as they stand at that moment (PCS:597-640, 809-825,
859-875), so which vote falls BEHIND the decision changes median_cp - unless every vote carries max_cp = slot - 1, as
streams.vote_round's do.  order_round gives every vote its own checkpoint; reorder_within_groups permutes a group's
votes among its own positions; regular() restates, bucket by bucket, the kernel's conditions for the short path;
CASES are the calls of tests/test_staging_order_gpu.py, which tests/test_staging_order_model.py replays oracle against
oracle on the CPU to show that none of them is vacuous.  Test infrastructure only."""
import zlib

import numpy as np

from gigapaxos_amd import D_DECISION, S_OK
from tests.geometry_common import ar_route, geometry
from tests.parity_common import wrap32

INT32_MAX = (1 << 31) - 1
INT32_MIN = -(1 << 31)
GUEST = 7777  # a node that is no member of any group; below 2^16: its votes travel without an escape
KS_ROWS = 4   # rows per group of the two-word staging


def order_round(groups, ks, members, newest, me, rng, back=0, d_range=(-3, 9), edges=None, edge_groups=None, nvotes=None,
                extra=None, extra_rank=0, extra_groups=None):
    """One round of votes as six int32 columns (gidx, bnum, bcoord, slot, acceptor, max_cp): the votes of a group sit at
    shuffled positions of the call, its members answer in a random order of their own, and every vote carries its own
    checkpoint max_cp = slot - 1 - d, d uniform in d_range (d < 0: an acceptor ahead of the coordinator's slot).

    groups: the table rows; ks: their sizes; members: the node ids (a group of K has the first K); newest: every group's
    newest outstanding slot (int64, not wrapped: the columns are); back: the slot answered is newest - back (scalar or per
    group); edges = (values, share): that share of the votes (of the groups edge_groups marks, default all) takes d from
    `values`; nvotes: distinct members that answer per group (default all); extra = "dup" (a second vote of one of the
    group's voters, with a checkpoint of its own as a retransmission after a checkpoint carries) or "guest" (a vote of
    GUEST) at arrival rank extra_rank among the group's votes, for the groups extra_groups marks (default all)."""
    groups = np.asarray(groups, np.int32)
    ng = groups.shape[0]
    ks = np.broadcast_to(np.asarray(ks, np.int64), (ng,))
    kmax = int(ks.max())
    mem = np.asarray(members, np.int32)
    nv = ks.copy() if nvotes is None else np.broadcast_to(np.asarray(nvotes, np.int64), (ng,)).copy()
    assert (nv >= 1).all() and (nv <= ks).all()
    has_extra = np.zeros(ng, bool)
    if extra is not None:
        has_extra = np.ones(ng, bool) if extra_groups is None else np.asarray(extra_groups, bool)
    keys = rng.random((ng, kmax))
    keys[np.arange(kmax)[None, :] >= ks[:, None]] = 2.0  # columns beyond the group's size order last
    perm = np.argsort(keys, axis=1)
    c = nv + has_extra
    n = int(c.sum())
    start = np.cumsum(c) - c
    gi = np.repeat(np.arange(ng), c)
    rank = np.arange(n) - np.repeat(start, c)
    r_ins = np.where(has_extra, np.minimum(extra_rank, nv), 1 << 20)[gi]
    is_extra = rank == r_ins
    src = rank - (rank > r_ins)
    dup_of = rng.integers(0, 1 << 30, ng) % nv
    src = np.where(is_extra, dup_of[gi], src)
    acc = mem[perm[gi, src]]
    if extra == "guest":
        acc = np.where(is_extra, GUEST, acc).astype(np.int32)
    d = rng.integers(d_range[0], d_range[1], n)
    if edges is not None:
        values, share = edges
        pick = rng.random(n) < share
        if edge_groups is not None:
            pick &= np.asarray(edge_groups, bool)[gi]
        d = np.where(pick, rng.choice(np.asarray(values, np.int64), size=n), d)
    slot = (np.asarray(newest, np.int64) - np.broadcast_to(np.asarray(back, np.int64), (ng,)))[gi]
    flat = [groups[gi], np.zeros(n, np.int32), np.full(n, me, np.int32), wrap32(slot), acc.astype(np.int32),
            wrap32(slot - 1 - d)]
    pos = rng.permutation(n)
    at = pos[np.lexsort((pos, gi))]  # the group's own positions, ascending: rank r of the group arrives r-th
    cols = []
    for f in flat:
        col = np.empty(n, np.int32)
        col[at] = f
        cols.append(col)
    return cols


def reorder_within_groups(cols, how):
    """The same columns with every group's votes permuted among that group's own positions.  "reversed": the last arrival
    first, ...; "last_first": the last arrival first, the others behind it in their order."""
    g = cols[0]
    n = g.shape[0]
    order = np.argsort(g, kind="stable")
    gs = g[order]
    start = np.concatenate([[0], np.nonzero(np.diff(gs))[0] + 1]) if n else np.zeros(0, np.int64)
    cnt = np.diff(np.concatenate([start, [n]]))
    st, c = np.repeat(start, cnt), np.repeat(cnt, cnt)
    i = np.arange(n) - st
    if how == "reversed":
        src = st + (c - 1 - i)
    elif how == "last_first":
        src = st + (i - 1) % c
    else:
        raise ValueError(how)
    out = []
    for col in cols:
        new = np.empty_like(col)
        new[order] = col[order[src]]
        out.append(new)
    assert (out[0] == g).all()
    return out


def tiles_of(cols, T):
    """Every vote's (tile, offset in the tile) of a call scattered in tiles of T votes."""
    i = np.arange(cols[0].shape[0])
    return i // T, i % T


def _majority2(x, y):
    """wave_majority2 (gpx_tiles.hip.h): what more than half of the first <= 64 entries hold, looking at four candidates
    at most; entry 0's otherwise."""
    m = min(x.shape[0], 64)
    x, y = x[:m], y[:m]
    tried = np.zeros(m, bool)
    cx, cy = x[0], y[0]
    for _ in range(4):
        same = (x == cx) & (y == cy)
        if 2 * int(same.sum()) > m:
            return int(cx), int(cy)
        tried |= same
        rest = np.nonzero(~tried)[0]
        if rest.shape[0] == 0:
            break
        cx, cy = x[rest[0]], y[rest[0]]
    return int(x[0]), int(y[0])


def _u32(x):
    return np.asarray(x, np.int64) & 0xFFFFFFFF


def _jsub(a, b):
    return wrap32(np.asarray(a, np.int64) - np.asarray(b, np.int64)).astype(np.int64)


def regular(cols, pair, T, pre=None, dec=None):
    """Which buckets of this call the K <= 4 kernel does NOT take down its two-word path, and why: {bucket: reason}, the
    reason being the first of the kernel's own tests that fails (bucket16_body's `if constexpr (TW)` block, in its order;
    the escapes are k_scatter_tiles', gpx_tiles.hip.h scatter_tile: dslot, dcp, es, eb against the batch's reference vote).
    pair: .G, .shift, .W, optionally .stopped (rows the test stopped); pre: (rows, status) of a snapshot of every table
    row taken BEFORE the call; dec: the oracle's decisions of the call.  (A preparing coordinator cannot be told from a
    snapshot: no stream here has one.  The staging rows fit whenever the call has a quarter of a vote per lane.)"""
    gidx, bnum, bcoord, slot, acc, maxcp = (np.asarray(c, np.int64) for c in cols)
    G, sh, W = pair.G, pair.shift, pair.W
    gb = 1 << sh
    nbk = (G + gb - 1) >> sh
    n = gidx.shape[0]
    rows, st = pre
    in_table = (gidx >= 0) & (gidx < G)
    slot0, _ = _majority2(slot, np.zeros_like(slot))
    ref_bn, ref_bc = _majority2(bnum, bcoord)
    es = (_u32(slot - slot0 + 128) > 255) | (_u32(slot - 1 - maxcp + 128) > 255)
    eb = (bnum != ref_bn) | (bcoord != ref_bc) | (_u32(acc) > 0xFFFF)
    tile, _ = tiles_of(cols, T)
    ntiles = (n + T - 1) // T
    wide = np.bincount(tile[in_table & es], minlength=ntiles) * 32 > T
    gsafe = np.where(in_table, gidx, 0)
    cnt = np.bincount(gsafe[in_table], minlength=G)
    nxt = rows["next_proposal_slot"].astype(np.int64)
    ndec = np.bincount(np.asarray(dec.gidx, np.int64)[np.asarray(dec.kind) == D_DECISION], minlength=G)
    nout = np.bincount(np.asarray(dec.gidx, np.int64), minlength=G)
    stopped = np.zeros(G, bool)
    stopped[list(getattr(pair, "stopped", ()))] = True
    out = {}
    for b in range(nbk):
        lo, hi = b << sh, min((b + 1) << sh, G)
        mine = in_table & (gidx >= lo) & (gidx < hi)
        nb = int(mine.sum())
        if nb == 0:
            out[b] = "empty"
            continue
        c = cnt[lo:hi]
        if ((b + 1) << sh) > G:
            why = "partial bucket"
        elif not gb <= nb <= KS_ROWS * gb:
            why = "sparse or over-full"
        elif wide[tile[mine]].any():
            why = "wide tile"
        elif (c > KS_ROWS).any():
            why = "more votes than rows"
        elif es[mine].any():
            why = "escaped slot or checkpoint"
        elif (c < 1).any():
            why = "group without a vote"
        elif not ((st[lo:hi] == S_OK) & (rows["has_coord"][lo:hi] == 1) & ~stopped[lo:hi]).all():
            why = "group missing, idle or stopped"
        elif not ((rows["coord_bnum"][lo:hi] == ref_bn) & (rows["coord_bcoord"][lo:hi] == ref_bc)).all():
            why = "not the reference ballot"
        elif eb[mine].any():
            why = "escaped ballot or acceptor"
        else:
            first = np.full(G, np.iinfo(np.int64).min)
            first[gidx[mine][::-1]] = slot[mine][::-1]  # (any of the group's votes: they must all agree)
            d = _jsub(nxt[lo:hi], first[lo:hi])
            if (slot[mine] != first[gidx[mine]]).any():
                why = "two slots in a group"
            elif not ((d >= 1) & (d <= W)).all():
                why = "slot outside the window"
            elif not ((ndec[lo:hi] == 1) & (nout[lo:hi] == 1)).all():
                why = "not one decision per group"
            else:
                continue
        out[b] = why
    return out


def every_bucket(pair, why):
    return {b: why for b in range((pair.G + (1 << pair.shift) - 1) >> pair.shift)}


def retarget(cols, i, slot, d):
    """Vote i answers `slot` (not wrapped) with checkpoint slot - 1 - d instead."""
    cols[3][i] = wrap32(slot)
    cols[5][i] = wrap32(slot - 1 - d)


class Driver:
    """What a case's script drives: the pair's proposals and order_round's calls.  reply() is the test's: the HIP engine
    against the oracle on the GPU, the oracle against itself - with everything that keeps the case honest - on the CPU."""

    def __init__(self, pair, case):
        self.p, self.case = pair, case
        self.rng = np.random.default_rng(zlib.crc32(case["name"].encode()))
        self.nprop = 0

    @property
    def newest(self):
        return self.p.base[self.p.g] + self.nprop - 1

    def propose(self, times=1):
        for _ in range(times):
            self.p.propose()
            self.nprop += 1

    def cols(self, **opts):
        return order_round(self.p.g, self.p.ks, self.p.members, self.newest, self.p.me, self.rng, **opts)

    def round(self, what, irregular=None, **opts):
        return self.reply(self.cols(**opts), what, irregular or {})

    def route(self, n):
        """The front end geometry_common predicts for a call of n votes: the tiled one, with this many tiles."""
        T, NT = self.p.tile
        r = ar_route(geometry(self.p.G, self.p.kmax, self.p.shift), n, sar_max_n=0, force_T=T, force_NT=NT)
        assert r == ("tiles", T, NT), r
        return (n + T - 1) // T

    def reply(self, cols, what, irregular):
        raise NotImplementedError


# ---- the cases: what Pair is built with, and a script over a Driver --------------------------------------------------
# sens: "k3" / "k4" - reversing every group's arrival order must change at least one decision in ten, pooled over the
# case's regular rounds (measured on the oracle for uniform d in [-3, 9): 24 % for K = 3, 17 % for K = 4); "zero": it
# must change none, by construction; None: not claimed.  tiles: the tile counts of the case's calls.  spread: a
# multi-tile case, the tile part of the key matters.

def _rounds(n, irregular=None, **opts):
    def script(D):
        irr = irregular(D.p) if callable(irregular) else irregular
        for r in range(n):
            D.propose()
            D.round("round %d" % r, irr, **opts)
    return script


def _older_slot(D):
    p = D.p
    D.propose(2)
    cols = D.cols(back=1)
    D.reply(cols, "newest - 1", {})
    D.round("newest", {})
    D.propose(8)
    # group 900's second arrival answers another outstanding slot than its first: two slots, bucket 1 falls back
    cols = D.cols(back=7)
    i = np.nonzero(cols[0] == 900)[0][1]
    retarget(cols, i, int(D.newest[0]) - 3, 2)
    D.reply(cols, "oldest (d = W), two slots in group 900", {1: "two slots in a group"})
    D.round("retransmitted votes of a decided slot", every_bucket(p, "not one decision per group"), back=7)
    D.round("the oldest now (d = W - 1)", {}, back=6)
    # nine behind: its ring entry is the newest slot's (slot & 7), which must stay as it is
    D.round("more than W behind", every_bucket(p, "slot outside the window"), back=8)
    D.round("the newest", {})


def _guest(extra, rank):
    def script(D):
        for r in range(2):
            D.propose()
            D.round("%s at rank %d" % (extra, rank), {}, extra=extra, extra_rank=rank)
    return script


def _two_votes(D):
    for r in range(3):
        D.propose()
        D.round("two of three answer", {}, nvotes=2)


def _single_vote(D):
    nv = np.full(D.p.g.shape[0], 3)
    nv[700] = 1
    D.propose()
    D.round("one vote in group 700", {1: "not one decision per group"}, nvotes=nv)
    D.propose()
    nv[700] = 3
    D.round("all answer, group 700 its older slot", {}, back=(np.arange(D.p.g.shape[0]) == 700).astype(np.int64))


def _cp_edges(values, fallback):
    def script(D):
        p = D.p
        in1 = (p.g >> p.shift) == 1
        for r in range(4):
            D.propose()
            if fallback:  # a few votes of bucket 1 only
                D.round("checkpoint byte past its edges", {1: "escaped slot or checkpoint"}, edges=(values, 0.02),
                        edge_groups=in1)
            else:
                D.round("checkpoint byte at its edges", {}, edges=(values, 0.1))
    return script


def _lower_ballot(D):
    p = D.p
    nbk = p.G >> p.shift
    for r in range(4):
        D.propose()
        cols = D.cols()
        for b in range(nbk):  # a vote of a lower ballot in front of one group's own votes, in every bucket
            g = (b << p.shift) + 37 * (r + 1)
            i = int(np.nonzero(cols[0] == g)[0][0])
            v = [c[i] for c in cols]
            v[2] = p.me - 1
            cols = [np.ascontiguousarray(np.insert(c, max(i - 3, 0), x)) for c, x in zip(cols, v)]
        D.reply(cols, "a lower ballot in every bucket", every_bucket(p, "escaped ballot or acceptor"))


def _slot_base(G, far_lo, far_hi, only_bucket=None, gb=512):
    """A tenth of the groups `far_lo` slots below the others and a tenth `far_hi` above (only_bucket: three groups each,
    in that bucket alone)."""
    base = np.full(G, 1000, np.int64)
    if only_bucket is None:
        base[3::10] += far_lo
        base[7::10] += far_hi
    else:
        base[only_bucket * gb + np.array([5, 200, 411])] += far_lo
        base[only_bucket * gb + np.array([9, 300, 500])] += far_hi
    return base


def _slot_edges(D):
    D.propose(3)
    D.round("slot byte at its edges, newest - 2", {}, back=2)
    D.round("newest - 1", {}, back=1)
    D.round("newest", {})


def _slot_edges_fallback(D):
    D.propose(3)
    for back in (2, 1, 0):
        D.round("slot byte past its edges", {2: "escaped slot or checkpoint"}, back=back)


def _half_far(G):
    base = np.full(G, INT32_MAX - 4, np.int64)
    base[1::2] = INT32_MIN + 2
    return base


def _partial(p):
    return {p.G >> p.shift: "partial bucket"}


_T4 = (4096, 512)
CASES = [
    # 1. order, one and two tiles
    dict(name="order-2048", sens="k3", tiles={2}, spread=True, script=_rounds(6),
         pair=dict(G=2048, k=3, node_slots=[0, 2, 5], tile=_T4)),
    dict(name="order-2000-partial-bucket", sens="k3", tiles={2}, spread=True, script=_rounds(6, _partial),
         pair=dict(G=2000, k=3, node_slots=[0, 2, 5], tile=_T4)),
    # 2. four tiles (tile_adv), K = 4: majority 3, all four rows used
    dict(name="four-tiles-k4", sens="k4", tiles={4}, spread=True, script=_rounds(4),
         pair=dict(G=4096, k=4, node_slots=[0, 1, 3, 6], tile=_T4)),
    # 3. bit 13 of the offset: tiles of 16,384 votes, the first one full
    dict(name="offset-bit-13", sens="k3", tiles={2}, spread=True, script=_rounds(3),
         pair=dict(G=8192, k=3, node_slots=[0, 2, 5], tile=(16384, 1024))),
    # 4. 256 and 1,024 lanes per bucket (the 10-bit local group field full), on the smallest tables of four buckets
    dict(name="lanes-256", sens="k3", tiles={1}, script=_rounds(4),
         pair=dict(G=1024, k=3, node_slots=[0, 2, 5], tile=_T4, shift=8)),
    dict(name="lanes-1024", sens="k3", tiles={3}, spread=True, script=_rounds(4),
         pair=dict(G=4096, k=3, node_slots=[0, 2, 5], tile=_T4, shift=10)),
    # 5. the checkpoint byte and the slot byte at and past their edges
    dict(name="checkpoint-byte-edges", sens="k3", tiles={2}, cp_bytes=(0, 255), script=_cp_edges((-128, 127), False),
         pair=dict(G=2048, k=3, node_slots=[0, 2, 5], tile=_T4)),
    dict(name="checkpoint-byte-escapes", sens=None, tiles={2}, cp_bytes=(-1, 256), script=_cp_edges((-129, 128), True),
         pair=dict(G=2048, k=3, node_slots=[0, 2, 5], tile=_T4)),
    dict(name="slot-byte-edges", sens="k3", tiles={2}, slot_bytes=(0, 255), script=_slot_edges,
         pair=dict(G=2048, k=3, node_slots=[0, 2, 5], tile=_T4, window=64, base=_slot_base(2048, -128, 127))),
    dict(name="slot-byte-escapes", sens=None, tiles={2}, slot_bytes=(-1, 256), script=_slot_edges_fallback,
         pair=dict(G=2048, k=3, node_slots=[0, 2, 5], tile=_T4, window=64, base=_slot_base(2048, -129, 128, 2))),
    # 6. older outstanding slots, retransmissions, slots behind the window
    dict(name="older-slot", sens="k3", tiles={2}, script=_older_slot,
         pair=dict(G=2048, k=3, node_slots=[0, 2, 5], tile=_T4)),
    # 7. four rows with a guest, two votes, one vote
    dict(name="duplicate-first", sens="k3", tiles={2}, script=_guest("dup", 0), pair=dict(G=2048, k=3, node_slots=[0, 2, 5], tile=_T4)),
    dict(name="duplicate-third", sens="k3", tiles={2}, script=_guest("dup", 2), pair=dict(G=2048, k=3, node_slots=[0, 2, 5], tile=_T4)),
    dict(name="duplicate-last", sens="k3", tiles={2}, script=_guest("dup", 3), pair=dict(G=2048, k=3, node_slots=[0, 2, 5], tile=_T4)),
    dict(name="stranger-first", sens="k3", tiles={2}, script=_guest("guest", 0), pair=dict(G=2048, k=3, node_slots=[0, 2, 5], tile=_T4)),
    dict(name="stranger-third", sens="k3", tiles={2}, script=_guest("guest", 2), pair=dict(G=2048, k=3, node_slots=[0, 2, 5], tile=_T4)),
    dict(name="stranger-last", sens="k3", tiles={2}, script=_guest("guest", 3), pair=dict(G=2048, k=3, node_slots=[0, 2, 5], tile=_T4)),
    dict(name="two-votes-of-three", sens="zero", tiles={1}, script=_two_votes,
         why_zero="both votes are needed for the majority of three: the median is taken after both, whichever comes first",
         pair=dict(G=2048, k=3, node_slots=[0, 2, 5], tile=_T4)),
    dict(name="single-vote", sens=None, tiles={2}, script=_single_vote, pair=dict(G=2048, k=3, node_slots=[0, 2, 5], tile=_T4)),
    dict(name="groups-of-one-and-two", sens="zero", tiles={1}, script=_rounds(4),
         why_zero="K = 1 and K = 2 need every vote for the majority: nothing falls behind the decision",
         pair=dict(G=2048, k=2, kmax=4, ks=1 + (np.arange(2048) % 2), node_slots=[0, 3, 0, 0], tile=_T4)),
    # 8. across Integer.MAX_VALUE
    dict(name="across-max-value", sens="k3", tiles={2}, script=_rounds(10),
         pair=dict(G=2048, k=3, node_slots=[0, 2, 5], tile=_T4, base=np.full(2048, INT32_MAX - 4, np.int64))),
    # (MIN_VALUE + 2 is seven slots past MAX_VALUE - 4: the slot byte spans the wrap, every bucket stays regular)
    dict(name="half-at-min-value", sens="k3", tiles={2}, script=_rounds(10),
         pair=dict(G=2048, k=3, node_slots=[0, 2, 5], tile=_T4, base=_half_far(2048))),
    # 9. the other layouts on the same stream
    dict(name="five-replicas", sens=None, tiles={3}, script=_rounds(4), kernel="k_bucket_ar16_tiles_k5", two_word=False,
         pair=dict(G=2048, k=5, node_slots=[0, 1, 2, 4, 7], tile=_T4)),
    dict(name="four-word-lower-ballot", sens="k3", tiles={2}, script=_lower_ballot,
         pair=dict(G=2048, k=3, node_slots=[0, 2, 5], tile=_T4)),
]
CASE = {c["name"]: c for c in CASES}
