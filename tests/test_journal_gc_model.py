"""tests/journal_gc_model.py - the specification of include/gpx_journal_gc.h - against a literal restatement of
compactLogfile's loop (SQLPaxosLogger.java:3375-3408): walk the file entry by entry, look the entry's group threshold
up, append or skip.  And the non-vacuity of the seeded cases that tests/test_journal_gc_gpu.py runs on the GPU."""
import numpy as np
import pytest

from tests import journal_gc_common as C
from tests import journal_gc_model as GM
from tests import journal_model as M


def compact_logfile(data, base, index, gc_slot):
    """compactLogfile's loop.  index: {file offset: (group, slot)} - what parsing the entry back into a packet gives the
    Java; gc_slot: {group: LogIndex.gcSlot}.  -> (tmp file bytes, [(group, slot, new offset, length)], compacted,
    neededAtAll)"""
    raf, tmp, entries = M.JournalFile(data, base), bytearray(), []
    compacted = needed_at_all = False
    while raf.pos < len(raf.data):                   # raf.getFilePointer() < raf.length()
        at = base + raf.pos
        offset = len(tmp)                            # rafTmp.getFilePointer()
        length = raf.read_int()
        msg = raf.read_fully(length)
        g, slot = index[at]
        if GM.i32(slot - gc_slot[g]) > 0:            # isLogMsgNeeded: !(slot - gcSlot <= 0)
            tmp += length.to_bytes(4, "big") + msg
            needed_at_all = True
            entries.append((g, slot, offset, length))
        else:
            compacted = True
    return bytes(tmp), entries, compacted, needed_at_all


def java_outcome(compacted, needed_at_all):
    return "replace" if compacted and needed_at_all else "delete" if not needed_at_all else "leave"


def against_the_loop(c, a_gc, cp=None):
    """a case whose rows name every entry of the file, in file order, of groups that exist"""
    want = GM.compact(c["data"], c["in_bytes"], c["in_base"], c["e_gidx"], c["e_slot"], c["e_off"], c["e_len"], a_gc,
                      np.ones(len(a_gc), bool), c["e_bnum"], c["e_bcoord"], cp, out_base=c["in_base"])
    index = {int(o): (int(g), int(s)) for o, g, s in zip(c["e_off"], c["e_gidx"], c["e_slot"])}
    gcs = {}
    for i, g in enumerate(c["e_gidx"].tolist()):
        th = GM.gc_of(a_gc[g], None if cp is None else cp[i])
        assert gcs.setdefault(g, th) == th            # the threshold is per group
    tmp, entries, compacted, needed = compact_logfile(bytes(c["data"]), c["in_base"], index, gcs)
    assert want.bytes == tmp
    rows = want.rows
    assert [(int(a), int(b), int(o) - c["in_base"], int(ln)) for a, b, o, ln in zip(rows["gidx"], rows["slot"], rows["off"], rows["len"])] == entries
    assert GM.outcome(want.counts) == java_outcome(compacted, needed)
    assert want.counts["n_bad"] == 0 and want.counts["named_bytes"] == c["in_bytes"]
    # the survivors through the journal pack (the parent commit's detour) are the same bytes
    assert C.survivors_through_pack(c, want) == want.bytes
    # and every kept entry reads back at its new offset as getJournaledMessage reads it
    for s, o, ln in zip(rows["src"], rows["off"], rows["len"]):
        old = int(c["e_off"][s])
        assert M.read_entry(tmp, int(o), int(ln), c["in_base"]) == M.read_entry(bytes(c["data"]), old, int(ln), c["in_base"])
    return want


def test_the_three_outcomes():
    gc = C.table_gc()
    for case, outcome in ((C.runs_case(), "replace"), (C.uniform_case(True), "leave"), (C.uniform_case(False), "delete")):
        assert GM.outcome(against_the_loop(case, gc).counts) == outcome
    u = against_the_loop(C.uniform_case(True), gc)
    assert u.counts["unchanged"] == 1 and u.counts["n_runs_done"] == 1 and u.bytes == bytes(C.uniform_case(True)["data"])
    s = C.model(C.uniform_case(True), flags=GM.SKIP_UNCHANGED)
    assert s.counts["unchanged"] == 1 and s.counts["n_done"] == 0 and s.bytes == b"" and s.counts["n_keep"] == 700
    # all kept, but not the input: unnamed bytes, rows out of order
    for case, runs in ((C.gaps_case(), 12), (C.swapped_case(), 4)):
        w = C.model(case, flags=GM.SKIP_UNCHANGED)
        assert w.counts["unchanged"] == 0 and w.counts["n_keep"] == len(case["e_len"]) == w.counts["n_done"] and w.counts["n_runs_done"] == runs


def test_wraparound_slots_and_thresholds():
    """gc at Integer.MAX_VALUE - 1: slots on both sides of the wrap; Java's int arithmetic throughout"""
    assert GM.i32(2 ** 31) == -2 ** 31 and GM.i32(-2 ** 31 - 1) == 2 ** 31 - 1
    gc = C.MAX_V - 1
    assert [GM.needed(s, gc) for s in (gc - 1, gc, C.MAX_V, C.MIN_V, C.MIN_V + 5, int(C.wrap(gc + 2 ** 31 - 1)), int(C.wrap(gc + 2 ** 31)))] == \
        [False, False, True, True, True, True, False]
    # cp_slot above, equal to, below and wrapped against a_gc: the smaller on the ring, SQLPaxosLogger.java:1482
    for acc in C.SPECIAL_GC:
        w = lambda d: int(C.wrap(acc + d))   # noqa: E731
        assert GM.gc_of(acc) == acc and GM.gc_of(acc, w(3)) == acc and GM.gc_of(acc, acc) == acc
        assert GM.gc_of(acc, w(-3)) == w(-3) and GM.gc_of(acc, w(2 ** 31)) == w(2 ** 31)
    for mode in C.CP_MODES:
        c = C.verdict_case(mode)
        keep = c["e_gidx"] == np.clip(c["e_gidx"], 0, 4)            # the rows of the five judged groups
        sub = {k: (v[keep] if isinstance(v, np.ndarray) and k.startswith(("e_", "cp_")) else v) for k, v in c.items()}
        sub["in_bytes"] = int(sub["e_off"][-1] + 4 + sub["e_len"][-1] - sub["in_base"])
        sub["data"] = c["data"][:sub["in_bytes"]]
        want = against_the_loop(sub, C.table_gc(), sub["cp_slot"])
        v = want.verdicts.reshape(5, 8)
        if mode in ("none", "above", "equal"):                      # d = -1, 0, 1, 2^31 - 1, 2^31, -4, -3, -2 against gc itself
            assert (v == [0, 0, 1, 1, 0, 0, 0, 0]).all()
        elif mode == "below":                                       # the threshold is gc - 3: -3 goes, -2 .. 1 stay
            assert (v == [1, 1, 1, 0, 0, 0, 0, 1]).all()
        else:                                                       # gc + 2^31 is "below" on the ring: what lies behind gc stays
            assert (v == [1, 0, 0, 0, 0, 1, 1, 1]).all()
        full = C.model(c)
        assert full.verdicts[-5:].tolist() == [GM.KEEP_UNJUDGED] * 5 and full.counts["n_unjudged"] == 5


def test_a_merge_of_two_files():
    """mergeLogfiles: two files laid end to end are one input, the output one file"""
    gc = C.table_gc()
    a, b = C.runs_case(), C.uniform_case(True, n=300, seed=31, in_base=0)
    both = {k: np.concatenate([a[k], b[k]]) for k in ("data", "e_gidx", "e_slot", "e_len")}
    both.update(in_bytes=a["in_bytes"] + b["in_bytes"], in_base=0, e_off=np.concatenate([a["e_off"], b["e_off"] + a["in_bytes"]]),
                e_bnum=None, e_bcoord=None, cp_slot=None)
    m = against_the_loop(both, gc)
    wa, wb = against_the_loop(a, gc), against_the_loop(b, gc)
    assert m.bytes == wa.bytes + wb.bytes and m.counts["n_keep"] == wa.counts["n_keep"] + 300
    assert m.rows["off"].tolist() == wa.rows["off"].tolist() + (wb.rows["off"] + len(wa.bytes)).tolist()


def test_refusals_caps_and_counts_only():
    c, by_prefix = C.refusal_case()
    w = C.model(c)
    assert w.counts["n_bad"] == 9 and w.counts["n_usable"] == 31 and w.counts["unchanged"] == 0
    bad = np.nonzero(w.verdicts == GM.BAD)[0].tolist()
    assert bad == [5, 6, 7, 8, 20, 22, 23, 24, 39] and not set(bad) & set(w.rows["src"].tolist())
    wo = C.model(c, data=False, flags=GM.COUNT_ONLY)
    assert np.nonzero(wo.verdicts == GM.BAD)[0].tolist() == [r for r in bad if r not in by_prefix] and wo.rows is None
    case, ends = C.caps_case()
    whole = C.model(case)
    assert whole.counts["keep_bytes"] == ends[-1] and whole.counts["n_keep"] == len(ends) - 1
    for cb, k in ((0, 0), (24, 0), (25, 1), (ends[300], 300), (ends[300] + 3, 300), (ends[300] - 1, 299)):
        p = C.model(case, cap_bytes=cb)
        assert (p.counts["n_done"], p.counts["bytes_done"]) == (k, ends[k]) and p.bytes == whole.bytes[:ends[k]]
        assert p.counts["n_keep"] == whole.counts["n_keep"] and p.counts["keep_bytes"] == ends[-1]
    p = C.model(case, cap_entries=128)
    assert p.counts["n_done"] == 128 and p.rows["src"].tolist() == whole.rows["src"][:128].tolist()


@pytest.mark.parametrize("name", ["runs", "phases", "tiny", "big", "round"])
def test_the_gpu_cases_are_not_vacuous(name):
    """what tests/test_journal_gc_gpu.py relies on, from the model alone on the same seeds: in the run cases at least a
    third of the entries are dropped and at least a third kept; the phase case reaches all 256 pairs of phases; the tile
    cases have the sizes they claim"""
    if name == "runs":
        c = C.runs_case()
        w = C.model(c)
        n = len(c["e_len"])
        assert 3 * w.counts["n_keep"] >= n and 3 * (n - w.counts["n_keep"]) >= n and w.counts["n_bad"] == 0
        assert w.counts["n_runs_done"] == len(C.RUN_LENGTHS)
        heads = np.nonzero(np.diff(np.concatenate([[-2], w.rows["src"]])) != 1)[0]
        assert np.diff(np.concatenate([heads, [w.counts["n_keep"]]])).tolist() == list(C.RUN_LENGTHS)
        assert any(int(w.rows["src"][h]) // 256 != int(w.rows["src"][h] + r - 1) // 256 for h, r in zip(heads, C.RUN_LENGTHS))
    elif name == "phases":
        c = C.phase_case()
        w = C.model(c)
        assert len(C.phase_pairs(c, w)) == 256 and set(c["e_len"].tolist()) == set(range(41))
    elif name == "tiny":
        w = C.model(C.tiny_case())
        assert w.counts["n_runs_done"] == 5000 and w.counts["keep_bytes"] < 2 * 16384      # > 256 runs in a 16 KB tile
        for k in (1, 2, 3):
            for d in (-5, 0, 5):
                case, total = C.tile_edge_case(k, d)
                assert C.model(case).counts["keep_bytes"] == total
        h = C.model(C.huge_case())
        assert (1 << 20) + 13 in h.rows["len"].tolist() and 0 < h.counts["n_keep"] < 2001
    elif name == "round":
        from tests import journal_common as JC
        g, s = JC.round_records()
        assert JC.GROUPS == 300 and JC.WINDOW == 8
        log = C.round_logged(g, s)
        assert int(log.sum()) == JC.ROUND_LOGGED[0] and set(s[log].tolist()) == set(range(1, 13))
        keep = np.array([GM.needed(b, C.round_commits()[a]) for a, b in zip(g[log], s[log])])
        assert 3 * int(keep.sum()) >= keep.size and 3 * int((~keep).sum()) >= keep.size
    else:
        c = C.big_case()
        w = C.model(c)
        assert w.counts["n_keep"] == 35_000 and len(c["e_len"]) > 256 * 256
        cut = C.model(c, cap_entries=32_800)
        assert int(cut.rows["src"][-1]) // 256 >= 256                                        # the cut falls into the second round
