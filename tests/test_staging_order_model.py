"""tests/test_staging_order_gpu.py's cases cannot be vacuous: every one of them replayed on the CPU, the oracle against
the oracle (tests/staging_common.py).  Per case: reversing every group's arrival order changes at least one decision in
ten where the case claims to see the order (none where it cannot, by construction); regular() - the restatement of the
two-word path's conditions - names exactly the buckets the case says fall back, and why; the multi-tile cases spread
their groups over tiles so that a key without its tile bits mis-orders them; the byte-edge cases reach bytes 0 and 255
in regular buckets (-1 and 256, the escapes, in their twins); and a second reading of handleAcceptReplyMyBallot
(pcs_enum_common.model_stream, written independently of the oracle) gives the same order-dependent medians on 200
groups of every stream."""
import numpy as np
import pytest

from tests.parity_common import wrap32
from tests.pcs_enum_common import model_stream
from tests.staging_common import CASE, CASES, GUEST, Driver, _jsub, _majority2, order_round, regular, reorder_within_groups, tiles_of
from tests.test_two_word_staging_gpu import Pair

SENS_FLOOR = 0.10  # one decision in ten (measured for uniform d in [-3, 9): 24 % at K = 3, 17 % at K = 4)


class ModelDriver(Driver):
    """p.eo takes the case's calls, p.eh (an oracle as well) the same calls with every group's arrival order reversed."""

    def __init__(self, pair, case):
        super().__init__(pair, case)
        self.calls, self.changed, self.total = [], 0, 0

    def reply(self, cols, what, irregular):
        p, case = self.p, self.case
        ntiles = self.route(cols[0].shape[0])
        assert ntiles in case["tiles"], (what, ntiles)
        pre = p.eo.snapshot(np.arange(p.G, dtype=np.int32))
        do = p.eo.accept_reply(*cols)
        dr = p.eh.accept_reply(*reorder_within_groups(cols, "reversed"))
        if case.get("two_word", True):
            assert regular(cols, p, p.tile[0], pre, do) == irregular, what
        a, b = do.as_tuple_array(), dr.as_tuple_array()
        a, b = a[np.lexsort((a[:, 1], a[:, 0]))], b[np.lexsort((b[:, 1], b[:, 0]))]
        # the same groups decide the same slots in either order; only the median can differ
        assert a.shape == b.shape and (a[:, [0, 1, 2, 3, 5]] == b[:, [0, 1, 2, 3, 5]]).all(), what
        self.changed += int((a[:, 4] != b[:, 4]).sum())
        self.total += a.shape[0]
        self.calls.append((cols, do, irregular))
        p.round += 1
        return do


def _run(monkeypatch, oracle_lib, name):
    case = CASE[name]
    D = ModelDriver(Pair(monkeypatch, oracle_lib, oracle_lib, **case["pair"]), case)
    case["script"](D)
    return D


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_case_says_what_it_claims(monkeypatch, oracle_lib, name):
    """The predicate held at every call (ModelDriver.reply); here the case's own floors."""
    case = CASE[name]
    D = _run(monkeypatch, oracle_lib, name)
    p = D.p
    assert D.total > 0
    share = D.changed / D.total
    print("%s: reversing the arrival order changes %d of %d decisions (%.1f %%)" % (name, D.changed, D.total, 100 * share))
    if case["sens"] in ("k3", "k4"):
        assert share >= SENS_FLOOR, (name, share)
    elif case["sens"] == "zero":
        assert D.changed == 0 and case["why_zero"], name
    # whatever the order, the state afterwards is the same: every vote reaches recordSlotNumber, decided or not
    allg = np.arange(p.G, dtype=np.int32)
    assert p.eh.snapshot(allg)[0].tobytes() == p.eo.snapshot(allg)[0].tobytes()
    T = p.tile[0]
    gb = 1 << p.shift
    if case.get("spread"):
        for cols, _, _ in D.calls:
            tile, off = tiles_of(cols, T)
            g = cols[0]
            order = np.argsort(g, kind="stable")
            gs, ts, os_ = g[order], tile[order], off[order]
            multi = np.zeros(p.G, bool)
            inverted = np.zeros(p.G, bool)
            # consecutive arrivals of one group: a later tile, and there a smaller offset than the arrival before
            nxt = (gs[1:] == gs[:-1]) & (ts[1:] > ts[:-1])
            multi[gs[1:][nxt]] = True
            inverted[gs[1:][nxt & (os_[1:] < os_[:-1])]] = True
            ng = np.unique(g).shape[0]
            assert 2 * int(multi.sum()) >= ng, (name, int(multi.sum()), ng)
            assert 10 * int(inverted.sum()) >= ng, (name, int(inverted.sum()), ng)
    for key, col in (("cp_bytes", 5), ("slot_bytes", 3)):
        if key not in case:
            continue
        seen_regular, seen_any = set(), set()
        for cols, _, irregular in D.calls:
            slot = cols[3].astype(np.int64)
            if col == 5:
                byte = _jsub(slot - 1, cols[5]) + 128
            else:
                byte = _jsub(slot, _majority2(slot, np.zeros_like(slot))[0]) + 128
            reg = ~np.isin(cols[0] >> p.shift, list(irregular))
            seen_any |= set(np.unique(byte).tolist())
            seen_regular |= set(np.unique(byte[reg]).tolist())
        lo, hi = case[key]
        if (lo, hi) == (0, 255):
            assert {0, 255} <= seen_regular and min(seen_any) == 0 and max(seen_any) == 255, (name, key)
        else:
            assert {lo, hi} <= seen_any and min(seen_regular) >= 0 and max(seen_regular) <= 255, (name, key)
    # the second reading, on 200 groups spread over the table
    behind = np.zeros(p.kmax, np.int64) if case["pair"].get("node_slots") is None else np.asarray(case["pair"]["node_slots"], np.int64)
    final = p.eo.snapshot(allg)[0]
    for g in np.linspace(0, p.G - 1, 200).astype(np.int64):
        K = int(p.ks[g])
        mem = [int(m) for m in p.members[:K]]
        b = int(p.base[g])
        votes, want = [], []
        for cols, do, _ in D.calls:
            for i in np.nonzero(cols[0] == g)[0]:
                a = int(cols[4][i])
                ballot = (int(cols[1][i]), int(cols[2][i]))
                kind = 0 if ballot == (0, p.me) else (1 if ballot > (0, p.me) else -1)
                votes.append((int(cols[3][i]), mem.index(a) if a in mem else -1, kind, int(cols[5][i])))
            t = do.as_tuple_array()
            want += [tuple(int(x) for x in r[1:]) for r in t[t[:, 0] == g]]
        init = [int(wrap32(b - 1 - behind[j])) for j in range(K)]
        out, _, coord, ns = model_stream(mem, p.me, D.nprop, votes, init, base=b - 1)
        assert [o[1:] for o in out] == want, (name, int(g))
        assert coord and ns == final["node_slots"][g][:K].tolist(), (name, int(g))
    p.eh.close()
    p.eo.close()


def test_every_path_of_the_issue_has_a_case():
    names = set(CASE)
    assert len(names) == len(CASES)
    assert {c["sens"] for c in CASES} == {"k3", "k4", "zero", None}
    assert sum(1 for c in CASES if c.get("spread")) >= 4
    assert any(int(np.max(c["pair"]["base"])) == (1 << 31) - 5 for c in CASES if c["pair"].get("base") is not None)


@pytest.mark.parametrize("how", ["reversed", "last_first"])
def test_reorder_keeps_every_group_on_its_own_positions(how):
    rng = np.random.default_rng(7)
    G = 300
    ks = 1 + np.arange(G) % 4
    cols = order_round(np.arange(G), ks, [100, 101, 102, 103], np.full(G, 50), 100, rng, extra="guest", extra_rank=1,
                       extra_groups=np.arange(G) % 5 == 0)
    tag = np.arange(cols[0].shape[0], dtype=np.int32)  # a seventh column: which vote went where
    new = reorder_within_groups(cols + [tag], how)
    assert (new[0] == cols[0]).all()
    for g in range(G):
        at = np.nonzero(cols[0] == g)[0]
        was, now = tag[at].tolist(), new[6][at].tolist()
        assert now == (was[::-1] if how == "reversed" else was[-1:] + was[:-1])
        assert at.shape[0] == ks[g] + (g % 5 == 0)
    back = reorder_within_groups(new, how)
    if how == "reversed":
        assert all((x == y).all() for x, y in zip(back, cols + [tag]))
    # one vote per member, the stranger's second among its group's, checkpoints all over [-3, 9) slots behind slot - 1
    d = 50 - 1 - cols[5].astype(np.int64)
    assert set(np.unique(d).tolist()) == set(range(-3, 9)) and (cols[3] == 50).all()
    for g in range(0, G, 5):
        at = np.nonzero(cols[0] == g)[0]
        assert cols[4][at[min(1, ks[g])]] == GUEST and sorted(cols[4][np.delete(at, min(1, ks[g]))]) == list(range(100, 100 + ks[g]))


def test_default_vote_round_is_left_alone():
    """bench.py is filled from streams.vote_round: its default output keeps every vote at max_cp = slot - 1."""
    from gigapaxos_amd import streams
    cols = streams.vote_round(64, [100, 101, 102], 4, 100)
    assert (cols[3] == 5).all() and (cols[5] == 4).all() and cols[0].shape[0] == 192
