"""The two readings of the log index (tests/logindex_model.py) against each other, without a GPU: the flat table with
the calls' exact outputs and the per-group restatement of paxosutil/LogIndex.java, over seeded random operation
sequences and over every directed case the GPU file runs - and what keeps those from being vacuous."""
import numpy as np
import pytest

from tests import logindex_common as LC
from tests import logindex_model as LM

G, CAP = 128, 1024


def random_sequence(seed, B):
    """adds of a few files, GC slots that move both ways, lookups with ranges that cross the wrap, compactions of a file
    (file_rows -> relocate), table compactions, resets; slots walk across Integer.MAX_VALUE"""
    rng = np.random.default_rng(seed)
    groups = 12
    head = np.full(groups, LM.INT_MAX - 30, np.int64) + rng.integers(0, 20, groups)   # the next slot of each group
    file, ballot = 0, 0                                                    # ballots never repeat: no (slot, ballot) twice
    for step in range(60):
        op = 8 if step in (25, 45) else rng.integers(0, 10)
        if step % 3 == 2:                                                  # a range across the wrap, for every group
            B.lookup(np.arange(groups), [LM.INT_MAX - 100] * groups, [LM.INT_MIN + 100] * groups, [1] * groups, cap=CAP)
        if op < 4:
            n = int(rng.integers(1, 40))
            g = rng.integers(0, groups, n)
            back = rng.integers(-6, 4, n)                                  # some at or below what was logged, some new
            s = head[g] + back
            head[g] = np.maximum(head[g], s + 1)
            file += int(rng.integers(0, 2))
            LM.add_of(B, LM.recs(g, s, bnum=ballot + np.arange(n), bcoord=100 + rng.integers(0, 2, n)), file)
            ballot += n
        elif op < 6:
            g = rng.integers(0, groups + 1, int(rng.integers(1, 6)))       # group `groups`: never written; repeats happen
            B.set_gc(g, head[g % groups] - rng.integers(-2, 30, g.shape[0]))
        elif op < 8:
            g = rng.permutation(groups)[:5]
            lo = head[g] - rng.integers(0, 40, 5)
            B.lookup(g, lo, lo + rng.integers(-2, 30, 5), rng.integers(0, 2, 5), cap=CAP)
        elif op == 8:                                  # compact a file that is some group's min file
            _, groups_of, _, _ = B.files(0, file + 1)
            if not groups_of.any():
                continue
            f = int(np.nonzero(groups_of)[0][0])
            rows, c = B.file_rows(f, CAP)
            file += 1
            B.relocate(c["generation"], rows["row"], None, file, rows["off"] // 2, rows["len"])
            B.files(0, file + 1)
        else:
            if rng.integers(0, 2):
                B.compact()
            else:
                B.set_gc(rng.integers(0, groups, 1), None, LM.RESET)
    B.files(0, file + 1)
    B.lookup(np.arange(groups), [LM.INT_MAX - 200] * groups, cap=CAP)


@pytest.mark.parametrize("seed", range(8))
def test_flat_table_and_java_lists_agree_on_random_sequences(seed):
    B = LC.JavaChecked(G, CAP)
    random_sequence(seed, B)
    # not vacuous: an entry refused as stale; a GC slot that moved backwards over an entry that did not come back; a min
    # file that relocate left behind its group's first entry; a range across Integer.MAX_VALUE that found something
    assert all(v > 0 for v in B.seen.values()), B.seen
    assert B.m.n_rows > 0 and B.deviations == 0


@pytest.mark.parametrize("name", sorted(LM.CASES))
def test_directed_cases_on_both_readings(name):
    B = LC.JavaChecked(G, CAP)
    LM.CASES[name](B)
    # relocate goes by row, the reference by the first entry with equal (slot, ballot): the two part exactly in the case
    # that logs one slot at one ballot twice, and only in those two entries
    assert B.deviations == (1 if name == "relocate" else 0)


def test_the_directed_cases_reach_what_they_are_for():
    seen = dict(stale=0, backwards_gone=0, min_file_moved=0, wrap_range=0)
    for name in sorted(LM.CASES):
        B = LC.JavaChecked(G, CAP)
        LM.CASES[name](B)
        for k, v in B.seen.items():
            seen[k] += v
    assert all(v > 0 for v in seen.values()), seen


def test_java_arithmetic():
    assert LM.diff(LM.INT_MIN, LM.INT_MAX) == 1 and LM.diff(LM.INT_MAX, LM.INT_MIN) == -1
    assert LM.vdiff([LM.INT_MIN, 5], [LM.INT_MAX, 7]).tolist() == [1, -2]
    x = LM.LogIndex()
    assert x.get_min_logfile() is None and not x.add(-1, 0, 0, 3, 0, 0) and x.add(0, 0, 0, 3, 0, 0) and x.get_min_logfile() == 3
    x.set_gc_slot(0)
    assert x.get_min_logfile() is None and x.log == [] and not x.is_log_msg_needed(0) and x.is_log_msg_needed(1)
