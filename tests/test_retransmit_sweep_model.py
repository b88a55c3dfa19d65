"""The retransmission sweep (include/gpx_timers.h), the part that is arithmetic: the numpy model (tests/timers_model.py)
against hand-written answers; gpx_rtx_backoff_table against the reference's double comparison; the model's firing
instants against `JavaWaitfor` on the same clock; and the proof, on the CPU oracle alone, that none of the histories of
tests/test_retransmit_sweep_gpu.py is vacuous."""
import numpy as np
import pytest

from tests import timers_common as TC
from tests import timers_model as M

A, P, NONE = M.POKE_ACCEPT, M.POKE_PREPARE, M.POKE_NONE
ACC, PRE = [100, 150, 225], [40, 60, 90]


def rows_of(entries):
    """entries: (poke, slot, bnum, bcoord, heard) or None for a dead group"""
    cols = {c: [] for c in M.ROW_COLS + ("status",)}
    for e in entries:
        poke, slot, bnum, bcoord, heard = e if e is not None else (NONE, 0, 0, 0, 0)
        live = e is not None and poke != NONE
        for c, v in zip(M.ROW_COLS, (poke, slot if live else 0, bnum if live else 0, bcoord if live else 0,
                                     slot - 1 if live else 0, 0, heard if live else 0)):
            cols[c].append(v)
        cols["status"].append(M.S_NOGROUP if e is None else 0)
    return {c: np.array(v, np.int64) for c, v in cols.items()}


def one(T, entries, now, flags=0, cap=None, acc=ACC, pre=PRE):
    n = len(entries)
    return M.sweep(T, np.arange(n), rows_of(entries), now, acc, pre, flags, n if cap is None else cap)


def words(T):
    return list(zip((T.key != 0).tolist(), T.since.tolist(), T.count.tolist()))


def test_model_against_hand_written_answers():
    T = M.Timers(4)
    w = [(A, 7, 0, 100, 0), (P, 3, 1, 100, 0), (NONE, 0, 0, 0, 0), None]
    # arm
    r = one(T, w, 1000)
    assert r["counts"] == (0, 1, 2, 0) and r["armed"].tolist() == [0, 1]
    assert words(T) == [(True, 1000, 0), (True, 1000, 0), (False, 0, 0), (False, 0, 0)]
    # not yet due: the comparison is strict, for both kinds
    assert one(T, w, 1040)["counts"] == (0, 1, 2, 0)
    # the PREPARE is due after 41 ms, the ACCEPT not before 101
    r = one(T, w, 1041)
    assert r["counts"] == (1, 1, 2, 1) and r["cols"]["gidx"].tolist() == [1] and r["cols"]["poke"].tolist() == [P]
    assert r["cols"]["count"].tolist() == [1] and r["cols"]["waited"].tolist() == [41]
    assert words(T)[:2] == [(True, 1000, 0), (True, 1041, 1)]
    assert one(T, w, 1100)["counts"][0] == 0                      # 100 is not longer than 100; 59 not than 60
    # both due; re-armed with the next threshold
    r = one(T, w, 1102)
    assert r["cols"]["gidx"].tolist() == [0, 1] and r["cols"]["count"].tolist() == [1, 2]
    assert r["cols"]["waited"].tolist() == [102, 61] and r["cols"]["slot"].tolist() == [7, 3]
    assert words(T)[:2] == [(True, 1102, 1), (True, 1102, 2)]
    # a reply changes heard, not the timer
    k_before = T.key.copy()
    w[0] = (A, 7, 0, 100, 0b10)
    r = one(T, w, 1252)
    assert r["counts"][0] == 1 and r["cols"]["gidx"].tolist() == [1]      # 150 is not longer than 150; 150 > 90
    assert (T.key == k_before).all() and words(T)[0] == (True, 1102, 1)
    r = one(T, w, 1253)
    assert r["cols"]["gidx"].tolist() == [0] and r["cols"]["heard"].tolist() == [2] and r["cols"]["count"].tolist() == [2]
    # a decision moves the head of line: a new key, armed again, count 0
    w[0] = (A, 8, 0, 100, 0)
    r = one(T, w, 5000)
    assert r["armed"].tolist() == [0] and 0 not in r["cols"]["gidx"].tolist() and words(T)[0] == (True, 5000, 0)
    # a higher ballot likewise
    w[0] = (A, 8, 2, 100, 0)
    assert one(T, w, 6000)["armed"].tolist() == [0] and words(T)[0] == (True, 6000, 0)
    # PREPARE turning into ACCEPT on election: same slot, same ballot, another kind
    w[1] = (A, 3, 1, 100, 0)
    r = one(T, w, 6001)
    assert r["armed"].tolist() == [1] and words(T)[1] == (True, 6001, 0)
    # the wait ends: key and count go, since stays; the group dies: all three go
    w[0] = (NONE, 0, 0, 0, 0)
    one(T, w, 6002)
    assert words(T)[0] == (False, 6000, 0)
    w[1] = None
    one(T, w, 6003)
    assert words(T)[1] == (False, 0, 0)


def test_count_saturates_and_the_threshold_index_stops():
    T = M.Timers(1)
    w = [(A, 1, 0, 100, 0)]
    one(T, w, 0, acc=[10, 20], pre=[10, 20])
    now, fired = 0, []
    for c in range(300):
        now += 20 if c else 10
        assert one(T, w, now, acc=[10, 20], pre=[10, 20])["counts"][0] == 0       # 10 / 20 ms: not longer
        now += 1
        r = one(T, w, now, acc=[10, 20], pre=[10, 20])
        fired.append(r["cols"]["count"].tolist())
    assert fired == [[min(c + 1, 255)] for c in range(300)] and T.count[0] == 255


def test_cap_cut_continues_on_the_next_call_and_peek_changes_nothing():
    T = M.Timers(6)
    w = [(A, g + 1, 0, 100, 0) for g in range(6)]
    one(T, w, 0)
    before = words(T)
    r = one(T, w, 500, cap=0)
    assert r["counts"] == (6, 0, 6, 0) and words(T) == before                     # counts only
    r = one(T, w, 500, flags=M.PEEK)
    assert r["counts"] == (6, 0, 6, 0) and r["cols"]["gidx"].tolist() == list(range(6)) and words(T) == before
    r = one(T, w, 500, cap=4)
    assert r["counts"] == (6, 0, 6, 4) and r["cols"]["gidx"].tolist() == [0, 1, 2, 3]
    r = one(T, w, 500, cap=4)
    assert r["counts"] == (2, 0, 6, 2) and r["cols"]["gidx"].tolist() == [4, 5]
    assert [c for _, _, c in words(T)] == [1] * 6
    # a peek over a table it has never seen arms nothing
    T2 = M.Timers(6)
    assert one(T2, w, 0, flags=M.PEEK)["counts"] == (0, 0, 6, 0) and not T2.key.any()


def test_clock_wrap_and_a_clock_that_steps_back():
    for base in (2**31, 2**32, 3 * 2**31):
        T = M.Timers(1)
        w = [(A, 1, 0, 100, 0)]
        one(T, w, base - 50)
        assert T.since[0] == M.wrap32(base - 50)
        assert one(T, w, base - 1)["counts"][0] == 0
        assert one(T, w, base + 50)["counts"][0] == 0                              # 100 ms across the wrap
        r = one(T, w, base + 51)
        assert r["cols"]["waited"].tolist() == [101] and T.since[0] == M.wrap32(base + 51)
        assert one(T, w, base - 10**6)["counts"][0] == 0                           # the clock stepped back
        assert one(T, w, base + 51 - 2**31 + 1)["counts"][0] == 0                  # as far back as it can look
        assert words(T)[0] == (True, M.wrap32(base + 51), 1)                       # and nothing else happened


@pytest.mark.parametrize("timeout", [1, 7, 6000, 60000])
def test_backoff_table_against_the_java_comparison(timeout):
    import __graft_entry__ as ge

    ge.build()
    from gigapaxos_amd import load_hip, timers

    lib = load_hip()
    tab = timers.backoff_table(timeout, 1.5, 32, lib=lib).tolist()
    assert tab == M.backoff_table(timeout, 1.5, 32) and len(tab) == 32
    clock = [0]
    for c in range(32):
        j = M.JavaWaitfor(lambda: clock[0], timeout, 1.5)
        j.retransmission_count = c
        for wait in range(max(tab[c] - 2, 0), min(tab[c] + 3, 2**31)):
            assert (wait > tab[c]) == j.too_long(wait), (timeout, c, wait)
    # saturation: beyond INT32_MAX the entry is INT32_MAX, and no int32 wait is longer
    big = timers.backoff_table(60000, 1.5, 32, lib=lib).tolist()
    assert big[31] == M.INT32_MAX == M.backoff_table(60000, 1.5, 32)[31] and big[0] == 60000 and big[1] == 90000
    assert timers.backoff_table(2**31 - 1, 1.0, 3, lib=lib).tolist() == [2**31 - 1] * 3
    assert timers.backoff_table(7, 1.5, 4, lib=lib).tolist() == [7, 10, 15, 23]
    for bad in ((-1, 1.5, 4), (7, 0.5, 4), (7, float("nan"), 4), (7, float("inf"), 4), (7, 1.5, 0), (7, 1.5, 33)):
        with pytest.raises(timers.GpxError):
            timers.backoff_table(*bad, lib=lib)


def model_firings(ticks, kind, timeout, created_seen):
    """the ticks at which the model hands the wait back; created_seen: a sweep runs at the instant of creation"""
    T = M.Timers(1)
    w = [(kind, 5, 2, 100, 0)]
    tab = M.backoff_table(timeout, 1.5, 32)
    fired = []
    for t in ([0] if created_seen else []) + list(ticks):
        r = M.sweep(T, [0], rows_of(w), t, tab, tab, 0, 1)
        if r["counts"][0]:
            fired.append(t)
            assert r["cols"]["count"].tolist() == [len(fired)]
    return fired


def java_firings(ticks, timeout):
    clock = [0]
    j = M.JavaWaitfor(lambda: clock[0], timeout, 1.5)       # created at instant 0
    fired = []
    for t in ticks:
        clock[0] = t
        if j.test_and_set_waiting_too_long():
            fired.append(t)
    return fired


@pytest.mark.parametrize("kind", [A, P])
def test_firing_instants_equal_the_references(kind):
    timeout, period = 100, 37
    ticks = list(range(period, 8000, period))
    java = java_firings(ticks, timeout)
    assert len(java) >= 6
    assert model_firings(ticks, kind, timeout, created_seen=True) == java
    # the documented deviation and nothing else: the first sweep comes late, so the wait is stamped up to one period
    # after its creation - every firing is late by at most one period, none comes at a shorter interval than the threshold
    late = model_firings(ticks, kind, timeout, created_seen=False)
    assert len(late) >= 6 and late != java
    assert all(0 <= m - j <= period for m, j in zip(late, java))
    tab = M.backoff_table(timeout, 1.5, 32)
    stamps = [ticks[0]] + late
    for c, (a, b) in enumerate(zip(stamps, stamps[1:])):
        assert b - a > tab[c]
    # against a Java object created when the first sweep saw the wait, the instants are the reference's again
    clock = [ticks[0]]
    j = M.JavaWaitfor(lambda: clock[0], timeout, 1.5)
    shifted = []
    for t in ticks[1:]:
        clock[0] = t
        if j.test_and_set_waiting_too_long():
            shifted.append(t)
    assert shifted == late
    # and each firing is at most one sweep period behind the firing the reference would make from the same state
    for c, (a, b) in enumerate(zip(stamps, stamps[1:])):
        assert b - a <= tab[c] + period


SCENARIOS = [
    ("edges", lambda o: TC.hits_by_construction(None, o, "edges"), False),
    ("hole", lambda o: TC.hits_by_construction(None, o, "hole"), False),
    ("all", lambda o: TC.hits_by_construction(None, o, "all"), False),
    ("six sweeps", lambda o: TC.six_sweeps_of_backoff(None, o), False),
    ("prepare", lambda o: TC.prepare_kind(None, o), True),
    ("saturation", lambda o: TC.saturation(None, o), False),
    ("clock", lambda o: TC.clock_wrap(None, o), False),
    ("cap", lambda o: TC.cap_cuts(None, o), False),
    ("peek", lambda o: TC.peek_twice(None, o), False),
    ("listed", lambda o: TC.listed_sweep(None, o), False),
    ("shapes", lambda o: TC.shapes(None, o, 3, 3, 4), False),
    ("shapes 16", lambda o: TC.shapes(None, o, 16, 16, 8), False),
    ("shapes 1", lambda o: TC.shapes(None, o, 3, 1, 8), False),
    ("host twin", lambda o: TC.host_twin(None, o), False),
    ("end to end", lambda o: TC.end_to_end(None, o), False),
    ("many tiles", lambda o: TC.many_tiles(None, o, 130561), False),
]


@pytest.mark.parametrize("name,run,rekeys", SCENARIOS, ids=[s[0] for s in SCENARIOS])
def test_histories_of_the_gpu_file_are_not_vacuous(oracle_lib, name, run, rekeys):
    """Driven by orc_poke_scan alone: every history has due entries and waiting entries that are not due; one that claims
    a key change between two sweeps has one."""
    stats = run(oracle_lib)
    print(name, stats)
    assert stats["hits"] > 0 and stats["waiting_not_due"] > 0 and stats["sweeps"] >= 2
    if rekeys:
        assert stats["rekeyed"] > 0


def test_the_none_history_waits_for_nothing(oracle_lib):
    stats = TC.hits_by_construction(None, oracle_lib, "none")
    assert stats["hits"] == 0 and stats["waiting_not_due"] == 0
