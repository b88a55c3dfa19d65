"""tests/viewchange_lists_model.py (planes -> lists, both sides, both cuts, from_hit) over the ORACLE's dense calls, on the
CPU: the enumerations of tests/elect_enum_common.py at K = 3 and 5 and W = 4, 8 and 64, the constructed batches of
tests/viewchange_lists_common.py, and acceptor states with accepted slots on both sides of Integer.MAX_VALUE - and what
keeps the GPU legs of tests/test_viewchange_lists_gpu.py from being vacuous."""
import numpy as np
import pytest

from tests import elect_enum_common as EC
from tests import viewchange_lists_common as VC
from tests import viewchange_lists_model as M

SAMPLE = (3_000, 2607)     # (groups, seed) of an enumeration leg


def cap_set(W, total):
    return sorted({0, 1, W - 1, W, W + 1, total})


def check_caps(model, W, what):
    """Every pair of caps from {0, 1, W - 1, W, W + 1, all}: the rounds concatenated are the uncut lists - all of them
    where the caps guarantee progress, else the prefix up to a hit that the caps can never admit."""
    full_h, full_e, _ = model.more()
    for ch in cap_set(W, model.n_hits):
        for ce in cap_set(W, model.n_entries):
            hits, entries, done, _ = model.rounds(ch, ce)
            if ch >= 1 and ce >= W:
                assert done == model.n_hits, (what, ch, ce)
            elif done < model.n_hits:
                assert ch == 0 or int(model.cnt[done]) > ce, (what, ch, ce, done)
            ne = int(model.pre[done])
            M.same(hits, {c: a[:done] for c, a in full_h.items()}, f"{what} caps ({ch}, {ce}) hits")
            M.same(entries, {c: a[:ne] for c, a in full_e.items()}, f"{what} caps ({ch}, {ce}) entries")


class ModelDriver:
    """Answers run_scripts' prepare_reply from the MODEL's lists over the oracle's dense call (what the GPU driver does
    with the HIP list call), and keeps every call's dense answer."""

    def __init__(self, e):
        self.e, self.calls = e, []

    def __getattr__(self, name):
        return getattr(self.e, name)

    def prepare_reply(self, gidx, acceptor, r_bnum, r_bcoord, first_slot, pvalues=None):
        W = int(self.e.cfg.window)
        d = M.dense_from_answer(gidx, self.e.prepare_reply(gidx, acceptor, r_bnum, r_bcoord, first_slot, pvalues), W)
        self.calls.append(d)
        hits, entries, counts = M.ReplyModel(d, W).more()
        return M.answer_from_lists(d["n"], d["v_kind"], d["status"], hits, entries)


@pytest.mark.parametrize("K,W,base", [(3, 4, "plain"), (3, 8, "wrap"), (3, 64, "plain"), (5, 8, "plain")])
def test_model_on_the_enumerations(oracle_lib, K, W, base):
    drivers = []

    def driver(e):
        drivers.append(ModelDriver(e))
        return drivers[-1]
    st = EC.run_enum(oracle_lib, K, W, 3, base, "one-call", sample=SAMPLE, driver=driver)
    assert st.groups == SAMPLE[0] and st.elected > 0 and st.preempted > 0
    d = max(drivers[0].calls, key=lambda c: c["n"])
    model = M.ReplyModel(d, W)
    hits, entries, counts = model.more()
    assert counts["n_hits"] == counts["hits_done"] > 100 and counts["n_entries"] == counts["entries_done"] > 100
    M.same(M.lists_to_planes(hits, entries, d["n"], W), M.dense_on_hits(d, W), "lists_to_planes(model(dense))")
    # ascending record index; a hit's rows begin where the last hit's end
    assert (np.diff(hits["rec"]) > 0).all() and (hits["off"][1:] == (hits["off"] + hits["count"])[:-1]).all()
    sub = M.take(d, np.arange(min(d["n"], 700)))
    check_caps(M.ReplyModel(sub, W), W, f"K {K} W {W}")
    # from_hit on its own: every start of a short call, caps that cut inside
    small = M.ReplyModel(M.take(d, np.arange(60)), W)
    fh, fe, _ = small.more()
    for f in range(small.n_hits + 2):
        h, e, c = small.more(f, 3, W + 1)
        k = c["hits_done"]
        assert c["from_hit"] == f and (k > 0 or f >= small.n_hits)
        M.same({x: a for x, a in h.items() if x != "off"}, {x: a[f:f + k] for x, a in fh.items() if x != "off"}, f"from {f}")
        lo = int(small.pre[min(f, small.n_hits)])
        M.same(e, {x: a[lo:lo + c["entries_done"]] for x, a in fe.items()}, f"from {f} entries")
        assert (h["off"] == (small.pre[f:f + k] - lo)).all()


@pytest.mark.parametrize("W", [4, 8, 64])
def test_constructed_batches_are_not_vacuous(oracle_lib, W):
    """The batch kinds of tests/viewchange_lists_common.py do on the oracle what they claim: every e_kind occurs, a
    GPX_S_WINDOW hit of either sort, a PREEMPTED hit with entries, hits with 0, 1 and W entries."""
    e = VC.coordinator_engine(oracle_lib, W)
    try:
        kinds = VC.pattern(600, seed=W)
        assert set(kinds) >= set(VC.HIT_KINDS + ".i")
        b = VC.coordinator_batch([e], W, kinds)
        d = M.dense_from_answer(b[0], e.prepare_reply(*b), W)
        model = M.ReplyModel(d, W)
        hits, entries, counts = model.more()
        want_hit = np.array([k in VC.HIT_KINDS for k in kinds])
        assert hits["rec"].tolist() == np.nonzero(want_hit)[0].tolist()
        assert hits["count"].tolist() == [VC.expected_entries(kinds[r], W) for r in hits["rec"].tolist()]
        by = {k: hits["rec"][[kinds[r] == k for r in hits["rec"].tolist()]] for k in VC.HIT_KINDS}
        assert all(len(v) for v in by.values())
        assert (d["v_kind"][np.concatenate([by[k] for k in VC.ELECT_KINDS])] == M.V_ELECTED).all()
        assert (d["v_kind"][by["X"]] == M.V_PREEMPTED).all() and (d["e_count"][by["X"]] == 2).all()
        assert (d["status"][by["C"]] == M.S_WINDOW).all() and (d["v_kind"][by["C"]] == M.V_IGNORED).all()
        assert (d["status"][by["N"]] == M.S_WINDOW).all() and (d["v_kind"][by["N"]] == M.V_RECORDED).all()
        assert (d["status"][by["G"]] == 1).all()
        assert set(entries["kind"].tolist()) == {1, 2, 3, 4}, "every e_kind: carry, no-op, pre-active, new stop"
        assert {0, 1, W} <= set(hits["count"].tolist())
        assert counts["n_elected"] == sum(kinds.count(k) for k in VC.ELECT_KINDS) and counts["n_preempted"] == kinds.count("X")
        assert counts["n_dropped"] == sum(kinds.count(k) for k in "CNG")
        M.same(M.lists_to_planes(hits, entries, d["n"], W), M.dense_on_hits(d, W), "constructed batch")
        check_caps(model, W, f"constructed W {W}")
    finally:
        e.close()


@pytest.mark.parametrize("s0", [VC.WRAP_S0, VC.PLAIN_S0], ids=["wrap", "plain"])
@pytest.mark.parametrize("W", [4, 8, 64])
def test_acceptor_lists_on_both_sides_of_the_wrap(oracle_lib, W, s0):
    e = VC.acceptor_engine(oracle_lib, W, groups=400, s0=s0)
    f = VC.acceptor_engine(oracle_lib, W, groups=400, s0=s0)
    try:
        g, bn, bc, fs = VC.acceptor_batch(257, groups=400, s0=s0)
        d = M.dense_prepare(e, g, bn, bc, fs)
        (rb, rc, rg, rf, st), rows = f.prepare(g, bn, bc, fs)
        off, ps, pb, pc, counts = M.prepare_lists(d, W)
        got = [(i, int(ps[x]), int(pb[x]), int(pc[x])) for i in range(257) for x in range(off[i], off[i + 1])]
        assert got == M.rows_by_signed_slot(rows) and counts["recs_done"] == 257 and counts["entries_done"] == len(rows)
        # the order is the TreeMap's - signed - and every list ascends in it
        assert all((np.diff(ps[off[i]:off[i + 1]].astype(np.int64)) > 0).all() for i in range(257))
        if s0 == VC.WRAP_S0:
            # lists on both sides of Integer.MAX_VALUE: the signed order is not the order the slots were numbered in
            both = [i for i in range(257) if off[i + 1] - off[i] > 1 and ps[off[i]] < 0 <= ps[off[i + 1] - 1]]
            assert len(both) > 20
            assert all(VC.i32(int(ps[off[i]]) - s0) > VC.i32(int(ps[off[i + 1] - 1]) - s0) for i in both)
        else:
            # ... and away from the wrap it is not the ring's either (2^31 is a multiple of every window: at the wrap
            # itself ring-index order and signed order coincide)
            many = [i for i in range(257) if off[i + 1] - off[i] > 1]
            ring = [[int(d["p_slot"][w * 257 + i]) for w in range(W) if (int(d["p_mask"][i]) >> w) & 1] for i in many]
            assert any(r != sorted(r) for r in ring) or W == 64, "ring-index order never differed from slot order"
        assert counts["n_nack"] > 10 and counts["n_tolog"] > 100 and counts["n_dropped"] == (st != 0).sum() > 0
        nack = np.nonzero(rf & M.P_NACK)[0]
        assert (np.diff(off)[nack] == 0).all() and (np.diff(off)[st != 0] == 0).all()
        dup = [i for i in nack.tolist() if bn[i] == 2]
        assert dup, "no NACK after an adopt inside the call"
        # the cut: leading complete records
        total = counts["n_entries"]
        for cap in sorted({0, 1, W - 1, W, W + 1, total // 2, total - 1, total}):
            o2, s2, b2, c2, k2 = M.prepare_lists(d, W, cap)
            r = k2["recs_done"]
            assert o2.tolist() == off[:r + 1].tolist() and k2["entries_done"] == off[r] <= cap
            assert r == 257 or off[r + 1] > cap
            assert s2.tolist() == ps[:off[r]].tolist() and b2.tolist() == pb[:off[r]].tolist() and c2.tolist() == pc[:off[r]].tolist()
        # repeating the PREPAREs of cut records changes nothing and returns the same pvalues
        d2 = M.dense_prepare(e, g[100:], np.maximum(bn[100:], 0), bc[100:], fs[100:])
        o3, s3, _, _, _ = M.prepare_lists(d2, W)
        same_ballot = np.nonzero((d2["r_flags"][:157] & M.P_NACK) == 0)[0]
        for i in same_ballot.tolist():
            if not (rf[100 + i] & M.P_NACK):
                assert s3[o3[i]:o3[i + 1]].tolist() == ps[off[100 + i]:off[101 + i]].tolist()
    finally:
        e.close(), f.close()
