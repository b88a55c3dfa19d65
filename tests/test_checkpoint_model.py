"""Checkpoint transfer without a GPU: the Java reading (tests/checkpoint_model.py) against hand-written answers, the
coverage of the plans the GPU tests use, and the equivalence the unchanged oracle can execute - a checkpoint record
equals one valued decision per skipped slot - shown on the oracle alone."""
import numpy as np
import pytest

from gigapaxos_amd import Engine, S_OK, S_STOPPED, S_WINDOW, C_HASVALUE
from tests import checkpoint_model as M
from tests.acc_enum_common import COORD

OK, STOPPED, AD, MV = S_OK, S_STOPPED, M.CP_ADOPT, M.CP_MOVED
INT_MAX, INT_MIN = M.INT_MAX, M.INT_MIN


def answers(seq, W=8, from_disk=True, start=1):
    """what every checkpoint record of the sequence answers, and the acceptor afterwards"""
    m = M.CpAcceptor(start, (0, COORD), start - 2 if start == 1 else M.I32(start) - 2, from_disk, W)
    out = [M.expected(m, op, W) for op in seq]
    return [o for op, o in zip(seq, out) if op[0] == "J"], out, m


def test_model_against_hand_written_answers():
    """Worked by hand from the Java text, scenario by scenario (tests/checkpoint_model.py, scenario_sequences); W = 8, the
    group starts at slot 1 with gc -1 and ballot (0, COORD).  One scenario per coverage counter."""
    S = M.scenario_sequences(8)
    M.reset_coverage()
    want_j = {
        0: [((OK, 1, 1, 0), None)],                               # cp == slot - 1: not adopted, nothing moves
        1: [((OK, 1, 2, AD | MV), None)],                         # cp == slot: one slot
        2: [((OK, 1, 4, AD | MV), (3, 1))],                       # jump to 3, the valued commit of 3 executes
        3: [((OK, 1, 8, AD | MV), None)],                         # d = 7 = W - 1
        4: [((OK, 1, 9, AD | MV), None)],                         # d = W
        5: [((OK, 1, 10, AD | MV), None)],                        # d = W + 1
        6: [((OK, 1, 5001, AD | MV), None)],
        7: [((OK, 1, 4, AD | MV), (3, 1))],
        8: [((OK, 1, 4, AD | MV), (3, 1))],                       # ... a stop: the group is stopped afterwards
        9: [((OK, 1, 4, AD | MV), (3, 1))],
        10: [((OK, 1, 2, AD | MV), None)],                        # blocked by a placeholder of another ballot
        11: [((OK, 1, 2, AD | MV), None), ((OK, 3, 5, AD | MV), None)],
        12: [((OK, 1, 3, AD | MV), None)],
        13: [((OK, 1, 4, AD | MV), None)],
        14: [((OK, 1, 1, 0), None)],
        15: [((STOPPED, 0, 0, 0), None)],
        16: [((OK, 1, 1, 0), None), ((OK, 4, 4, 0), None)],
        17: [((OK, 2, 2, 0), None), ((OK, 2, 4, AD | MV), (3, 1))],
    }
    assert len(S) == len(want_j)
    finals = {}
    for i, seq in enumerate(S):
        got_j, out, m = answers(seq)
        assert got_j == want_j[i], (i, got_j)
        finals[i] = (out, m)
    # what the jump left in the maps, seen by the records after it
    assert finals[3][1].dump_maps() == ((8, 0, COORD, -1, 0), [], [(9, 0, COORD, -1, 1, 0)])   # commits of 2, 3 gone
    assert finals[4][0][-1] == (OK, (9, 1)) and finals[5][0][-1] == (OK, (10, 1)) and finals[6][0][-1] == (OK, (5001, 1))
    assert finals[8][0][-1] == ((STOPPED, 0, 0, 0, 0), None) and finals[8][1].committed == {}  # the stop cleared commit 4
    assert finals[10][1].row() == (4, 2, COORD, 1) and finals[10][0][-1] == (OK, (2, 2))      # median 1 collected at the block
    assert finals[11][1].row() == (7, 1, COORD, 4) and finals[11][0][-2][1] == (5, 1)
    assert finals[14][0][2] == (OK, (1, 2)) and finals[14][1].stopped
    c = dict(M.CP_COVERAGE)
    assert c["jump_lt_W"] >= 1 and c["jump_eq_W"] == 1 and c["jump_gt_W"] == 2 and c["cp_eq_slot_minus_1"] == 4   # scenarios 0, 14, 16, 17
    assert c["cp_eq_slot"] == 4 and c["tail_valued"] == 5 and c["tail_stopped"] == 2 and c["tail_blocked_after_gc"] == 1
    assert c["accepts_kept_flag_off"] == 0 and c["tail_rebuilt"] == 0
    # the accepts flag: the same records, the accepts of the jumped range stay (and an ACCEPT behind one of them meets the
    # engine's ring limit)
    M.reset_coverage()
    _, out, m = answers(S[13], from_disk=False)
    assert [a[0] for a in m.dump_maps()[1]] == [1, 2, 3, 4] and M.CP_COVERAGE["accepts_kept_flag_off"] == 1
    _, out, m = answers(S[5], from_disk=False)
    assert out[3] == ((S_WINDOW, 0, 0, 0, 0), None) and [a[0] for a in m.dump_maps()[1]] == [2]
    _, out, m = answers(S[12], from_disk=False)                   # the blocked tail's collection takes accept 2
    assert m.row() == (3 + 1, 1, COORD, 3) and M.CP_COVERAGE["tail_blocked_after_gc"] == 1
    # the tail rebuilt from an accept: states with a placeholder next to its matching ACCEPT
    M.reset_coverage()
    want = [(OK, False, 5, 7, (5, 2)), (OK, True, 1, 5, (4, 1)), (OK, False, 1, 1, None), (OK, False, 2, 3, (2, 1))]
    for case, w in zip(M.STATE_CASES, want):
        m = M.state_model(case, 8, True)
        assert m.handleCheckpoint(case[4]) == w
    assert M.CP_COVERAGE["tail_rebuilt"] == 3 and M.CP_COVERAGE["tail_stopped"] == 1
    # the two wrap oddities, and the jump whose target is MIN_VALUE
    M.reset_coverage()
    hi, lo = M.WRAP_STARTS
    m = M.CpAcceptor(hi, (0, COORD), hi - 2)
    assert m.handleCheckpoint(INT_MAX) == (OK, True, hi, INT_MIN, None)
    m = M.CpAcceptor(hi, (0, COORD), hi - 2)
    assert m.handleCheckpoint(INT_MIN + 5) == (OK, False, hi, hi, None) and m.peekCheckpoint(INT_MIN + 5)[1:] == (False, hi, hi)
    m = M.CpAcceptor(lo, (0, COORD), lo - 2)
    assert m.peekCheckpoint(5) == (OK, True, lo, lo)
    assert m.handleCheckpoint(5) == (OK, True, lo, lo, None)      # adopted (5 >= MIN + 3), not moved (6 - slot wraps negative)
    assert M.CP_COVERAGE["wrap_adopted_not_moved"] == 1 and M.CP_COVERAGE["wrap_not_adopted"] == 1


def test_peek_is_step_one_and_two_of_the_record():
    for W in (4, 8):
        for seq in M.enum_sequences(W, n=400):
            m = M.CpAcceptor(1, (0, COORD), -1, True, W)
            for op in seq:
                if op[0] == "J":
                    st, adopt, frm, to = m.peekCheckpoint(op[1])
                    before = m.dump_maps()
                    full = m.handleCheckpoint(op[1])
                    assert (st, adopt, frm) == full[:3]
                    if st == OK:
                        assert to == (full[4][0] if full[4] else full[3])     # the tail starts where step 2 ends
                    assert st == OK or m.dump_maps() == before
                else:
                    M.expected(m, op, W)


def test_plans_of_the_gpu_tests_cover_every_counter():
    """The plans tests/test_checkpoint_gpu.py runs: the enumeration of every table, the wrap groups and the states built by
    import together leave no coverage counter at zero - and each table's enumeration alone covers what is not a wrap or
    an imported state."""
    M.reset_coverage()
    for W in (4, 8, 64):
        for fd in (True, False):
            before = dict(M.CP_COVERAGE)
            _, n = M.drive(M.enum_sequences(W), W, fd)
            assert n > 15000
            grew = {k for k in M.CP_COVERAGE if M.CP_COVERAGE[k] > before[k]}
            assert grew >= {"jump_lt_W", "jump_eq_W", "jump_gt_W", "cp_eq_slot_minus_1", "cp_eq_slot", "tail_valued",
                            "tail_stopped", "tail_blocked_after_gc"}, (W, fd, grew)
            assert ("accepts_kept_flag_off" in grew) == (not fd)
    ws = M.wrap_sequences()
    for fd in (True, False):
        M.drive([s for _, s in ws], 8, fd, starts=[a for a, _ in ws])
        for case in M.STATE_CASES:
            M.state_model(case, 8, fd).handleCheckpoint(case[4])
    zero = [k for k, v in M.CP_COVERAGE.items() if v == 0]
    assert not zero, zero


def oracle_engine(oracle_lib, G, W, from_disk):
    e = Engine(oracle_lib, COORD + 1, G, kmax=3, window=W, max_batch=1 << 17, flags=1 if from_disk else 0)
    M.create_at(e, [1] * G)
    return e


def merged_runs(runs):
    """{group: (first, total)} of runs that continue one another (a call reports one run per record that executed)"""
    out = {}
    for g, first, count in runs:
        if g in out:
            assert int(M.I32(out[g][0]) + out[g][1]) == first, (g, out[g], first)
            out[g] = (out[g][0], out[g][1] + count)
        else:
            out[g] = (first, count)
    return out


@pytest.mark.parametrize("W", [4, 8, 64])
@pytest.mark.parametrize("from_disk", [True, False])
def test_a_checkpoint_record_equals_one_valued_decision_per_skipped_slot(oracle_lib, W, from_disk):
    """For a live group with no stop parked in [slot, cp] and no parked median above its accepted-GC slot (how diff_plan
    builds its histories: a rule of construction, every generated case is compared), handleCheckpoint(cp) on the model
    and gpx_commit_batch of one GPX_C_HASVALUE decision per slot of [slot, cp] on the oracle leave the same
    HotRestoreInfo row, the same dump and the same answers to ACCEPTs and commits afterwards; the oracle's run
    (slot, d + t) is the call's (cp + 1, t)."""
    G = 240
    ds = (1, W - 1, W, W + 1, 2, 3, 2 * W + 1) * 5 + (5000,)     # 5,000 for a handful: one decision per slot on the oracle
    history, cps = M.diff_plan(G, W, from_disk, ds)
    assert len(cps) == G == len(history)                          # no case was left out
    eo = oracle_engine(oracle_lib, G, W, from_disk)
    M.reset_coverage()
    models, _ = M.drive(history, W, from_disk, engine=eo, dumps=G)      # the oracle follows the model up to the checkpoint
    gi, sl, md = M.decisions_for(models, cps)
    assert gi.size <= 1 << 17                                     # one call
    slot0 = {g: int(models[g]._slot) for g, _ in cps}
    st, runs = eo.commit(gi, np.zeros(gi.size, np.int32), np.full(gi.size, COORD, np.int32), sl, md,
                         np.full(gi.size, C_HASVALUE, np.uint8))
    refused = {int(g) for g in gi[st != S_OK]}                    # (checked below: only groups the tail stops)
    assert set(st.tolist()) <= {S_OK, S_STOPPED}
    got = merged_runs(runs.as_tuple_array().tolist())
    compared = 0
    for g, cp in cps:
        status, adopt, frm, to, run = models[g].handleCheckpoint(cp)
        t = run[1] if run else 0
        assert (status, adopt, frm) == (S_OK, True, slot0[g]) and to == cp + 1 + t
        assert run is None or run[0] == cp + 1
        assert got[g] == (slot0[g], cp + 1 - slot0[g] + t), (g, got[g], run)
        # a valued commit parked inside the range executes on the oracle as soon as the decisions reach it, and the stop
        # behind it with it: the decisions still to come for those slots then meet a stopped group
        assert g not in refused or models[g].stopped
        compared += 1
    assert compared == G and set(got) == {g for g, _ in cps}
    assert M.CP_COVERAGE["jump_lt_W"] and M.CP_COVERAGE["jump_eq_W"] and M.CP_COVERAGE["jump_gt_W"]
    assert M.CP_COVERAGE["tail_valued"] and (from_disk or M.CP_COVERAGE["accepts_kept_flag_off"])
    # the same row, the same dump, and the same answers to a probe afterwards (drive compares all three)
    rng = np.random.default_rng(W)
    probe = [tuple(M._ops_near(rng, int(models[g]._slot), 4, stops=False)) for g in range(G)]
    M.drive([()] * G, W, from_disk, engine=eo, dumps=G, models=models)
    M.drive(probe, W, from_disk, engine=eo, dumps=G, models=models)
    eo.close()
