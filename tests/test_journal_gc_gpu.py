"""The journal compaction (include/gpx_journal_gc.h) on the GPU, bit for bit against tests/journal_gc_model.py.  The
engine has a hundred groups created with chosen acceptor GC slots, read back with gpx_group_snapshot for the model.
Every buffer of a _dev call sits inside 4 KiB guard bands (tests/journal_common.Guarded): the outputs carry a sentinel
that is checked unchanged from bytes_done / row n_done to the end of the band, `in` lies between bands of live,
plausible bytes.  The cases are the smallest that reach each mechanism; tests/journal_gc_emulation.cpp runs the same
list on the CPU under AddressSanitizer, tests/test_journal_gc_model.py asserts their non-vacuity."""
import numpy as np
import pytest

from gigapaxos_amd import Engine, hri_create, S_OK, S_NOGROUP, S_STOPPED, C_HASVALUE, C_STOP
from tests import journal_common as JC
from tests import journal_gc_common as C
from tests import journal_gc_model as GM
from tests import journal_model as M

pytestmark = pytest.mark.gpu


def make_engine(lib, max_batch=1 << 14):
    """the table of tests/journal_gc_common.py: group g with acc_gc_slot table_gc()[g] and acc_slot one above it, group
    NEVER never created, group STOPPED stopped by a stop executed at its next slot"""
    e = Engine(lib, C.ME, C.G, kmax=C.K, window=8, max_batch=max_batch)
    g = np.array([q for q in range(C.G) if q != C.NEVER], np.int32)
    rows = hri_create(g.size, C.K, C.CREATOR)
    rows["acc_gc_slot"] = C.wrap(C.table_gc()[g])
    rows["acc_slot"] = C.wrap(C.table_gc()[g] + 1)                 # acc_slot - acc_gc_slot >= 1
    rows["next_proposal_slot"] = rows["acc_slot"]
    mem = np.tile(np.arange(C.CREATOR, C.CREATOR + C.K, dtype=np.int32), (g.size, 1))
    assert (e.create_groups(g, mem, C.K, rows) == S_OK).all()
    s = np.array([C.STOPPED], np.int32)
    nxt = C.wrap(C.table_gc()[s] + 1)
    st, _ = e.commit(s, [0], [C.CREATOR], nxt, [-1], np.array([C_HASVALUE | C_STOP], np.uint8))
    assert (st == S_OK).all()
    (_, _, _, _, st), _ = e.accept(s, [0], [C.CREATOR], C.wrap(nxt + 1), [-1])
    assert st.tolist() == [S_STOPPED]
    return e


def state(e):
    """a_gc and the exists flags as the model takes them, from gpx_group_snapshot"""
    rows, st = e.snapshot(np.arange(C.G))
    exists = st != S_NOGROUP
    return np.where(exists, rows["acc_gc_slot"], 0).astype(np.int64), exists


@pytest.fixture(scope="module")
def eng(hip_lib):
    e = make_engine(hip_lib)
    a_gc, exists = state(e)
    assert exists.tolist() == C.table_exists().tolist() and a_gc[exists].tolist() == C.table_gc()[exists].tolist()
    yield e, a_gc, exists
    e.close()


def through_pack_dev(e, c, want):
    """the differential: gpx_journal_pack_dev fed the survivors as frames gives the same bytes"""
    s = want.rows["src"].astype(np.int64)
    k = s.shape[0]
    i = np.zeros(k, np.int32)
    cols = dict(gidx=i, slot=i, bnum=i, bcoord=i, r_flags=np.full(k, M.R_TOLOG, np.uint8), status=np.zeros(k, np.uint8))
    p = JC.pack_dev(e, c["data"], c["e_off"][s] - c["in_base"] + 4, cols, frame_len=c["e_len"][s])
    assert p.bytes == want.bytes and k > 0


# 1 ---- verdicts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", C.CP_MODES)
def test_verdicts(eng, mode):
    e, a_gc, exists = eng
    c = C.verdict_case(mode)
    w = C.gc_dev(e, c, a_gc, exists, out_base=7, what="verdicts, cp_slot " + mode)
    assert w.counts["n_unjudged"] == 5 and w.verdicts[-5:].tolist() == [GM.KEEP_UNJUDGED] * 5
    v = w.verdicts[:40].reshape(5, 8)
    assert (v == v[0]).all() and 0 < v[0].sum() < 8                # the stopped group is judged like the others


# 2 ---- phases -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu_fast
def test_every_source_phase_against_every_output_phase(eng):
    e, a_gc, exists = eng
    c = C.phase_case()
    w = C.gc_dev(e, c, a_gc, exists, what="phases")
    assert len(C.phase_pairs(c, w)) == 256
    through_pack_dev(e, c, w)
    moved = dict(c, in_base=1 << 40, e_off=c["e_off"] + (1 << 40))
    C.gc_dev(e, moved, a_gc, exists, out_base=1 << 41, what="phases, a file offset as base")


# 3 ---- runs of kept rows --------------------------------------------------------------------------------------------------
def test_runs_of_kept_rows(eng):
    e, a_gc, exists = eng
    c = C.runs_case()
    w = C.gc_dev(e, c, a_gc, exists, what="runs")
    n = len(c["e_len"])
    assert w.counts["n_runs_done"] == len(C.RUN_LENGTHS) and 3 * w.counts["n_keep"] >= n and 3 * (n - w.counts["n_keep"]) >= n
    through_pack_dev(e, c, w)


def test_everything_kept_nothing_kept_and_broken_adjacency(eng):
    e, a_gc, exists = eng
    c = C.uniform_case(True)
    w = C.gc_dev(e, c, a_gc, exists, out_base=64, what="everything kept")
    assert w.counts["unchanged"] == 1 and w.counts["n_runs_done"] == 1 and w.bytes == c["data"].tobytes()
    w = C.gc_dev(e, c, a_gc, exists, flags=GM.SKIP_UNCHANGED, what="everything kept, skip unchanged")
    assert w.counts["unchanged"] == 1 and w.counts["n_done"] == 0 and w.counts["n_keep"] == 700      # and `out` kept its sentinel
    c = C.uniform_case(False)
    w = C.gc_dev(e, c, a_gc, exists, cap_bytes=c["in_bytes"], flags=GM.SKIP_UNCHANGED, what="nothing kept")
    assert w.counts["n_keep"] == 0 and w.counts["unchanged"] == 0 and GM.outcome(w.counts) == "delete"
    for c, runs, what in ((C.gaps_case(), 12, "unnamed bytes between rows"), (C.swapped_case(), 4, "rows out of offset order")):
        w = C.gc_dev(e, c, a_gc, exists, flags=GM.SKIP_UNCHANGED, what=what)
        assert w.counts["unchanged"] == 0 and w.counts["n_runs_done"] == runs and w.counts["n_done"] == len(c["e_len"])


# 4 ---- copy tiles ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
def test_tile_edges(eng, k):
    e, a_gc, exists = eng
    for d in range(-5, 6):
        c, total = C.tile_edge_case(k, d)
        w = C.gc_dev(e, c, a_gc, exists, out_base=77, what="total %d" % total)
        assert w.counts["bytes_done"] == total


def test_many_runs_per_tile_and_one_entry_over_many_tiles(eng):
    e, a_gc, exists = eng
    w = C.gc_dev(e, C.tiny_case(), a_gc, exists, what="10,000 entries of 0 and 1 bytes, alternately kept")
    assert w.counts["n_runs_done"] == 5000
    c = C.huge_case()
    w = C.gc_dev(e, c, a_gc, exists, out_base=5, what="one entry of 1 MiB + 13 among 2,000")
    assert (1 << 20) + 13 in w.rows["len"].tolist()
    through_pack_dev(e, c, w)


# 5 ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    e, a_gc, exists = eng
    c, by_prefix = C.refusal_case()
    w = C.gc_dev(e, c, a_gc, exists, cap_bytes=c["in_bytes"], what="refusals")
    bad = np.nonzero(w.verdicts == GM.BAD)[0].tolist()
    assert w.counts["n_bad"] == 9 and bad == [5, 6, 7, 8, 20, 22, 23, 24, 39] and not set(bad) & set(w.rows["src"].tolist())
    w = C.gc_dev(e, c, a_gc, exists, flags=GM.COUNT_ONLY, no_in=True, what="refusals, counts only without in")
    assert w.counts["n_bad"] == 9 - len(by_prefix)


# 6 ---- caps and small calls -----------------------------------------------------------------------------------------------
def test_caps_continuation_counts_only_and_empty_call(eng):
    e, a_gc, exists = eng
    c, ends = C.caps_case()
    n, nk = len(c["e_len"]), len(ends) - 1
    whole = C.gc_dev(e, c, a_gc, exists, out_base=500, what="uncut")
    # cap_bytes: 0, one byte short of the first entry, exactly at an entry's end, one byte either side, inside a prefix
    for cb, k in ((0, 0), (3, 0), (24, 0), (25, 1), (26, 1), (ends[300] - 1, 299), (ends[300], 300), (ends[300] + 1, 300),
                  (ends[300] + 2, 300), (ends[300] + 3, 300), (ends[128], 128), (ends[-1] - 1, nk - 1)):
        w = C.gc_dev(e, c, a_gc, exists, cap_bytes=cb, out_base=9, what="cap_bytes %d" % cb)
        assert w.counts["n_done"] == k and w.counts["n_keep"] == nk and w.counts["keep_bytes"] == ends[-1]
    for ce in (0, 1, 127, 128, 129, nk - 1):
        w = C.gc_dev(e, c, a_gc, exists, cap_entries=ce, what="cap_entries %d" % ce)
        assert w.counts["n_done"] == ce and w.counts["bytes_done"] == ends[ce]
    C.gc_dev(e, c, a_gc, exists, cap_bytes=ends[400] + 2, cap_entries=300, null_cols=True, no_verdict=True,
             what="both caps, the optional columns NULL")
    # the cut call continued to the end: the concatenation is the uncut answer
    got, first, base = b"", 0, 500
    while first < n:
        part = {k: (v[first:] if isinstance(v, np.ndarray) and k.startswith("e_") else v) for k, v in c.items()}
        w = C.gc_dev(e, part, a_gc, exists, cap_bytes=5000, cap_entries=64, out_base=base, what="continued from row %d" % first)
        assert w.counts["n_done"] > 0
        got += w.bytes
        base += w.counts["bytes_done"]
        first += int(w.rows["src"][-1]) + 1
        if w.counts["n_done"] == w.counts["n_keep"]:
            break
    assert got == whole.bytes and base == 500 + len(whole.bytes)
    w = C.gc_dev(e, c, a_gc, exists, flags=GM.COUNT_ONLY, what="counts only")
    assert w.counts["n_done"] == 0 and w.counts["keep_bytes"] == ends[-1]
    w = C.gc_dev(e, c, a_gc, exists, flags=GM.COUNT_ONLY, no_in=True, what="counts only, in NULL")
    assert w.counts["n_keep"] == nk and w.verdicts.tolist() == whole.verdicts.tolist()
    none = {k: (v[:0] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    none["in_bytes"] = 0
    for flags in (0, GM.COUNT_ONLY):
        w = C.gc_dev(e, none, a_gc, exists, cap_bytes=64, cap_entries=4, flags=flags, what="n = 0")
        assert w.counts["n_keep"] == 0 and w.counts["n_done"] == 0


# 7 ---- sizes --------------------------------------------------------------------------------------------------------------
def test_more_row_tiles_than_one_round_of_the_offsets_kernel(hip_lib):
    """70,000 rows are 274 tiles of rows, more than the 256 one round of k_jg_offsets takes, and a cut by cap_entries
    falls into a tile of the second round"""
    e = make_engine(hip_lib, max_batch=70_000)
    a_gc, exists = state(e)
    c = C.big_case()
    w = C.gc_dev(e, c, a_gc, exists, out_base=1 << 35, what="70,000 rows")
    assert w.counts["n_done"] == 35_000
    w = C.gc_dev(e, c, a_gc, exists, cap_entries=32_800, what="70,000 rows, cut in tile 256")
    assert w.counts["n_done"] == 32_800 and int(w.rows["src"][-1]) // 256 >= 256
    e.close()


# 8 ---- the host twin ------------------------------------------------------------------------------------------------------
def host(e, c, **kw):
    from gigapaxos_amd import journal_gc as J
    out, rows, verdict, counts = J.journal_gc(e, c["data"], c["e_gidx"], c["e_slot"], c["e_off"], c["e_len"], c["e_bnum"],
                                              c["e_bcoord"], c["cp_slot"], in_base=c["in_base"], in_bytes=c["in_bytes"], **kw)
    return (None if out is None else out.tobytes()), rows, verdict, GM.counts_of(counts)


def same_as_model(got, want, runs=True):
    """n_runs_done of the host twin counts a run once per chunk it is part of: compared only where there is one chunk"""
    out, rows, verdict, counts = got
    if not runs:
        assert counts["n_runs_done"] >= want.counts["n_runs_done"]
        counts = dict(counts, n_runs_done=want.counts["n_runs_done"])
    assert counts == want.counts and verdict.tolist() == want.verdicts.tolist()
    if want.rows is None:
        assert out is None
        return
    assert out == want.bytes
    for k, a in zip(GM.ROW_COLS, rows):
        assert (a is None and want.rows[k] is None) or a.tolist() == want.rows[k].tolist(), k


def test_host_twin_equals_the_device_form(eng):
    e, a_gc, exists = eng
    for c in (C.phase_case(), C.runs_case(), C.verdict_case("below")):
        want = C.gc_dev(e, c, a_gc, exists, out_base=1 << 40)
        same_as_model(host(e, c, out_base=1 << 40), want)
    # the refusal case: n_bad, n_usable and the verdicts equal the _dev form's, which tests every prefix on the device
    c, _ = C.refusal_case()
    want = C.gc_dev(e, c, a_gc, exists, cap_bytes=c["in_bytes"])
    same_as_model(host(e, c, cap_bytes=c["in_bytes"]), want)
    same_as_model(host(e, c, flags=GM.COUNT_ONLY), C.model(c, a_gc, exists, flags=GM.COUNT_ONLY))
    c, ends = C.caps_case()
    for cb, ce in ((ends[300] + 2, 5000), (1 << 30, 128), (ends[3], 5000), (3, 5)):
        same_as_model(host(e, c, cap_bytes=cb, cap_entries=ce), C.model(c, a_gc, exists, cap_bytes=cb, cap_entries=ce))
    # the outcome-only paths end after the first pass.  The binding has no staging counters, so that no byte of `in` is
    # read on these paths is covered by the code's structure and the emulation's exact-size `in` only; here: the answers
    c = C.uniform_case(False)
    got = host(e, c, flags=GM.SKIP_UNCHANGED)
    same_as_model(got, C.model(c, a_gc, exists, flags=GM.SKIP_UNCHANGED))
    assert got[3]["n_keep"] == 0 and got[0] == b""
    c = C.uniform_case(True)
    got = host(e, c, flags=GM.SKIP_UNCHANGED)
    same_as_model(got, C.model(c, a_gc, exists, flags=GM.SKIP_UNCHANGED))
    assert got[3]["unchanged"] == 1 and got[3]["n_done"] == 0 and got[0] == b""
    same_as_model(host(e, c), C.model(c, a_gc, exists))


def test_host_twin_in_chunks(hip_lib, monkeypatch):
    """`in` forced through several windows (16 KB instead of 64 MiB), from pageable memory: the same bytes and rows,
    positions, row numbers and caps carried from chunk to chunk; one entry larger than the window is a chunk of its own"""
    monkeypatch.setenv("GPX_TEST_JOURNAL_STAGE", "16384")
    e = make_engine(hip_lib)
    a_gc, exists = state(e)
    c = C.phase_case()                                   # 145 KB of entries: nine windows
    assert c["in_bytes"] >= 5 * 16384
    same_as_model(host(e, c, out_base=12345), C.model(c, a_gc, exists, out_base=12345), runs=False)
    w = C.model(c, a_gc, exists)
    ends = (w.rows["off"] + 4 + w.rows["len"]).tolist()
    for cb, ce in ((ends[900] + 1, 5000), (1 << 30, 1200), (ends[3], 5000)):
        same_as_model(host(e, c, cap_bytes=cb, cap_entries=ce), C.model(c, a_gc, exists, cap_bytes=cb, cap_entries=ce), runs=False)
    c = C.huge_case()
    same_as_model(host(e, c), C.model(c, a_gc, exists), runs=False)
    c = C.swapped_case()                                 # rows out of offset order: a window follows the rows, not the file
    same_as_model(host(e, c), C.model(c, a_gc, exists), runs=False)
    e.close()


# 9 ---- a real round -------------------------------------------------------------------------------------------------------
def test_a_real_round(hip_lib):
    """the ACCEPTs of tests/journal_common.round_records through gpx_accept_batch, packed with gpx_journal_pack; a later
    accept batch with a higher median checkpointed slot moves the acceptors' GC slots; then the journal is compacted"""
    from gigapaxos_amd import journal as J, journal_gc as JG
    e, _ = JC.rounds_engine(hip_lib)
    g, s = JC.round_records()
    frames = JC.round_frames(g, s, 0, 100)
    (_, _, _, r_flags, status), _ = e.accept(g, np.zeros_like(g), np.full_like(g, 100), s, np.full_like(g, -1))
    assert JC.logged(r_flags, status).tolist() == C.round_logged(g, s).tolist() and int(JC.logged(r_flags, status).sum()) == JC.ROUND_LOGGED[0]
    from gigapaxos_amd import wire as W
    buf, off = W.concat_frames(frames)
    z = np.zeros_like(g)
    out, rows, counts = J.journal_pack(e, buf, off, g, s, z, np.full_like(g, 100), r_flags, status, base_offset=4096)
    assert counts.n_done == JC.ROUND_LOGGED[0] == counts.n_entries
    rec, e_gidx, e_slot, e_bnum, e_bcoord, e_off, e_len = rows
    # the first round_commits(g) slots of group g are committed and executed, then one more ACCEPT per group (slot 8 again)
    # carries that many as the median checkpointed slot: the acceptor's GC slot follows it as far as the group has executed
    gg = np.arange(JC.GROUPS, dtype=np.int32)
    k = C.round_commits()
    cg, cs = np.repeat(gg, k), np.concatenate([np.arange(1, q + 1, dtype=np.int32) for q in k])
    stc, _ = e.commit(cg, np.zeros_like(cg), np.full_like(cg, 100), cs, np.full_like(cg, -1), np.full(cg.size, C_HASVALUE, np.uint8))
    assert (stc == S_OK).all()
    (_, _, _, _, st2), _ = e.accept(gg, np.zeros_like(gg), np.full_like(gg, 100), np.full_like(gg, 8), k)
    assert (st2 == S_OK).all()
    snap, st = e.snapshot(gg)
    a_gc = snap["acc_gc_slot"].astype(np.int64)
    assert (st == S_OK).all() and a_gc.tolist() == k.tolist()
    want = GM.compact(out, len(out), 4096, e_gidx, e_slot, e_off, e_len, a_gc, np.ones(JC.GROUPS, bool), e_bnum, e_bcoord,
                      out_base=1 << 20)
    n = len(e_len)
    assert 3 * want.counts["n_keep"] >= n and 3 * (n - want.counts["n_keep"]) >= n and want.counts["n_bad"] == 0
    got, k_rows, verdict, kc = JG.journal_gc(e, out, e_gidx, e_slot, e_off, e_len, e_bnum, e_bcoord, in_base=4096, out_base=1 << 20)
    assert GM.counts_of(kc) == want.counts and got.tobytes() == want.bytes and verdict.tolist() == want.verdicts.tolist()
    for k, a in zip(GM.ROW_COLS, k_rows):
        assert a.tolist() == want.rows[k].tolist(), k
    # the compacted file, read as recovery reads it, is the model's; every logged entry with slot - gc > 0 is still there
    w_off, w_len, n_walk, good = J.journal_walk(got, 1 << 20)
    assert (w_off.tolist(), w_len.tolist(), n_walk, good) == (want.rows["off"].tolist(), want.rows["len"].tolist(), kc.n_keep, len(want.bytes))
    kept = {(int(a), int(b)) for a, b in zip(k_rows[1], k_rows[2])}
    for a, b, r, o, ln in zip(e_gidx, e_slot, rec, e_off, e_len):
        if GM.i32(int(b) - int(a_gc[a])) > 0:
            assert (int(a), int(b)) in kept
    for src, o, ln in zip(k_rows[0], k_rows[5], k_rows[6]):
        assert M.read_entry(got.tobytes(), int(o), int(ln), 1 << 20) == frames[int(rec[src])]
    e.close()


def test_the_profile_names_the_four_kernels(hip_lib):
    e = make_engine(hip_lib, max_batch=1 << 12)
    a_gc, exists = state(e)
    c = C.runs_case()
    e.profile(2)
    C.gc_dev(e, c, a_gc, exists, flags=GM.COUNT_ONLY)
    prof0 = {k: v[0] for k, v in e.profile_read().items()}
    C.gc_dev(e, c, a_gc, exists)
    prof = {k: v[0] for k, v in e.profile_read().items()}
    e.profile(0)
    assert prof0 == {"k_jg_tile": 1, "k_jg_offsets": 1}, prof0
    assert prof == {"k_jg_tile": 2, "k_jg_offsets": 2, "k_jg_rows": 1, "k_jg_copy": 1}, prof
    e.close()
