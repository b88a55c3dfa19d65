"""The log index (include/gpx_logindex.h) on the GPU, bit for bit against tests/logindex_model.py.  Every buffer of a
_dev call sits inside 4 KiB guard bands (tests/journal_common.Guarded): an output column carries a sentinel that is
checked unchanged from the last entry the counts say was written to the end of its band.  The engine has 128 groups and
a table of 1,024 rows unless stated.  The directed cases are those of tests/logindex_model.py; tests/
test_logindex_model.py runs the same list against the restated Java and asserts their non-vacuity, tests/
logindex_emulation.cpp runs it on the CPU under AddressSanitizer.

Deviation (include/gpx_logindex.h): relocate goes by row identity, the reference by the first entry with equal (slot,
ballot); the `relocate` case logs one slot at one ballot twice, and the model test shows the two part exactly there."""
import numpy as np
import pytest

from gigapaxos_amd import Engine, hri_create, S_OK, RETIRE_PAUSE
from tests import journal_common as JC
from tests import journal_model as JM
from tests import logindex_common as LC
from tests import logindex_model as LM

pytestmark = pytest.mark.gpu

G, CAP, K, ME, CREATOR = 128, 1024, 3, 101, 100


def make_engine(lib, cap_rows=CAP, max_batch=1 << 12, groups=G, create=True):
    from gigapaxos_amd import logindex as L
    e = Engine(lib, ME, groups, kmax=K, window=8, max_batch=max_batch)
    if create:
        mem = np.tile(np.arange(CREATOR, CREATOR + K, dtype=np.int32), (groups, 1))
        assert (e.create_groups(np.arange(groups), mem, K, hri_create(groups, K, CREATOR)) == S_OK).all()
    if cap_rows:
        L.open(e, cap_rows)
    return e


def both(e, dev=True, groups=G, cap_rows=CAP):
    return LC.Both(LM.FlatIndex(groups, cap_rows), LC.DevCalls(e) if dev else LC.HostCalls(e))


def test_open_is_required_and_happens_once(hip_lib):
    from gigapaxos_amd import GpxError, logindex as L
    e = make_engine(hip_lib, cap_rows=0, create=False)
    with pytest.raises(GpxError):                                          # not open
        L.compact(e)
    with pytest.raises(GpxError):
        L.open(e, 0)
    L.open(e, 16)
    with pytest.raises(GpxError):                                          # a second open
        L.open(e, 16)
    c = L.compact(e)
    assert LC.counts_dict(c) == dict(LM.FlatIndex(G, 16)._counts(), generation=1)
    e.close()


# a, b, c, d (relocate's refusals), e, f ---- the directed cases on the _dev forms --------------------------------------------
@pytest.mark.parametrize("name", [pytest.param(n, marks=pytest.mark.gpu_fast) if n == "tile_edges" else n
                                  for n in sorted(LM.CASES)])
def test_directed_case_dev(hip_lib, name):
    e = make_engine(hip_lib, create=False)                                 # the index does not ask whether a group exists
    B = both(e)
    LM.CASES[name](B)
    assert B.calls > 5
    e.close()


# h ---- the host twins ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LM.CASES))
def test_directed_case_host_twins(hip_lib, name):
    e = make_engine(hip_lib, create=False)
    B = both(e, dev=False)
    LM.CASES[name](B)
    # the two forms on one index: what the twin wrote, the _dev form reads, and the other way round
    D = LC.Both(B.m, LC.DevCalls(e))
    D.lookup(np.arange(G), [0] * G, cap=CAP)
    LM.add_of(D, LM.recs([7, 7], [LM.INT_MAX - 1, LM.INT_MAX]), file=3)
    B.lookup([7], [LM.INT_MAX - 1], cap=4)
    B.files(0, 16)
    e.close()


# d ---- the compaction loop -------------------------------------------------------------------------------------------------
def test_compaction_loop_pack_add_gc_relocate(hip_lib):
    """gpx_journal_pack_dev -> add (n_dev = the pack's n_done, on the device) -> set_gc -> file_rows -> gpx_journal_gc_dev
    with cp_slot = e_gc -> relocate (n_dev = the compaction's n_done) -> lookup: every (off, len) points at its frame in
    the compacted bytes"""
    from gigapaxos_amd import journal as J, journal_gc as JG, logindex as L
    e = make_engine(hip_lib)
    n, base = 400, 5000
    lens = [20 + (i * 7) % 90 for i in range(n)]
    block, f_off, f_len = JC.frames_of_lengths(lens, seed=11, padded=True)
    i = np.arange(n, dtype=np.int32)
    cols = dict(gidx=i % 100, slot=1 + i // 100 + (i % 100) % 3, bnum=i % 4, bcoord=100 + i % 3,
                r_flags=np.full(n, JM.R_TOLOG, np.uint8), status=np.zeros(n, np.uint8))
    want_pack = JM.pack(block, f_off, cols["gidx"], cols["slot"], cols["bnum"], cols["bcoord"], cols["r_flags"],
                        cols["status"], f_len, None, base, 0, 1 << 20, n)
    assert want_pack.counts["n_done"] == n
    nbytes = want_pack.counts["bytes_done"]
    m = LM.FlatIndex(G, CAP)
    R = want_pack.rows
    m.add(R["gidx"], R["slot"], R["bnum"], R["bcoord"], R["off"], R["len"], 0)
    gcg = np.arange(0, 100, 2, dtype=np.int32)                             # every other group checkpoints at slot 2
    _, c_gc = m.set_gc(gcg, np.full(gcg.size, 2, np.int32))
    fr, c_fr = m.file_rows(0, n)
    k = c_fr["n_done"]
    assert 0 < c_gc["n_stale"] and k == n - c_gc["n_stale"] and k < n

    A = JC.Guarded()
    A.put("frames", block, live=True)
    A.put("frame_off", f_off.astype(np.int64), live=True)
    A.put("frame_len", f_len.astype(np.int32), live=True)
    for q in ("gidx", "slot", "bnum", "bcoord"):
        A.put(q, cols[q].astype(np.int32), live=True)
    for q in ("r_flags", "status"):
        A.put(q, cols[q], live=True)
    A.put("gcg", gcg, live=True)
    A.put("gcs", np.full(gcg.size, 2, np.int32), live=True)
    A.put("allg", np.arange(G, dtype=np.int32), live=True)
    A.put("zero", np.zeros(G, np.int32), live=True)
    sent = lambda b: np.full(b, JC.SENTINEL, np.uint8)  # noqa: E731
    A.put("journal", sent((nbytes + 15) // 16 * 16))
    for q, dt in JC.ROW_DT.items():
        A.put("p_" + q, sent(n * np.dtype(dt).itemsize))
    A.put("pack_counts", sent(32))
    A.put("add_status", sent(n))
    A.put("gc_status", sent(gcg.size))
    for q, dt in L.FILE_ROWS_COLS:
        A.put("f_" + q, sent(n * np.dtype(dt).itemsize))
    A.put("compacted", sent((nbytes + 15) // 16 * 16))
    A.put("verdict", sent(n))
    for q, dt in JG.ROW_COLS:
        A.put("k_" + q, sent(n * dt.itemsize))
    A.put("jg_counts", sent(64))
    for q, dt in L.LOOKUP_COLS:
        A.put("l_" + q, sent(n * np.dtype(dt).itemsize))
    A.put("lk_status", sent(G))
    for q in ("c_add", "c_gc", "c_fr", "c_rel", "c_lk"):
        A.put(q, sent(32))
    A.upload()
    p = A.ptr
    J.journal_pack_dev(e, n, p("frames"), block.shape[0], n, p("frame_off"), p("frame_len"), 0,
                       [p(q) for q in ("gidx", "slot", "bnum", "bcoord")], p("r_flags"), p("status"), base, 0, p("journal"),
                       nbytes, n, [p("p_" + q) for q in JC.ROW_DT], p("pack_counts"))
    L.add_dev(e, n, p("pack_counts") + 4, [p("p_" + q) for q in ("gidx", "slot", "bnum", "bcoord", "off", "len")], 0,
              p("add_status"), p("c_add"))                                 # n_dev: gpx_journal_counts.n_done
    L.set_gc_dev(e, gcg.size, p("gcg"), p("gcs"), 0, p("gc_status"), p("c_gc"))
    L.file_rows_dev(e, 0, n, [p("f_" + q) for q, _ in L.FILE_ROWS_COLS], p("c_fr"))
    # gpx_journal_gc_dev takes its n from the host: the caller reads file_rows' 32 bytes of counts first.  Here the model
    # knows k; the counts are compared below.
    JG.journal_gc_dev(e, k, p("journal"), nbytes, base,
                      [p("f_" + q) for q in ("gidx", "slot", "off", "len", "bnum", "bcoord", "gc")], 0, 0, p("compacted"),
                      nbytes, k, p("verdict"), [p("k_" + q) for q, _ in JG.ROW_COLS], p("jg_counts"))
    L.relocate_dev(e, k, p("jg_counts") + 8, 0, p("f_row"), p("k_src"), 1, p("k_off"), p("k_len"), p("c_rel"))
    L.lookup_dev(e, G, p("allg"), p("zero"), 0, 0, n, [p("l_" + q) for q, _ in L.LOOKUP_COLS], p("lk_status"), p("c_lk"))
    e.sync()
    A.download()

    def counts(q):
        return LC.counts_dict(L.LogIndexCounts.from_buffer_copy(A.get(q).tobytes()))
    assert A.get("journal")[:nbytes].tobytes() == want_pack.bytes
    assert counts("c_add") == dict(c_fr, n_done=n, n_hits=0, n_alive=n) and (A.get("add_status") == LM.ADDED).all()
    assert counts("c_gc") == c_gc and counts("c_fr") == c_fr
    for q, dt in L.FILE_ROWS_COLS:
        assert A.get("f_" + q, dt)[:k].tolist() == fr[q].tolist(), q
    jc = JG.JournalGcCounts.from_buffer_copy(A.get("jg_counts").tobytes())
    # cp_slot = e_gc keeps every alive row: all KEEP, k_src the identity, and the file loses the dead rows' bytes
    assert (A.get("verdict")[:k] == JG.JG_KEEP).all() and jc.n_keep == k == jc.n_done and jc.n_bad == 0 and jc.unchanged == 0
    assert A.get("k_src", np.int32)[:k].tolist() == list(range(k))
    assert jc.bytes_done == int((fr["len"].astype(np.int64) + 4).sum()) < nbytes
    k_off, k_len = A.get("k_off", np.int64)[:k], A.get("k_len", np.int32)[:k]
    c_rel = m.relocate(0, fr["row"], np.arange(k), 1, k_off, k_len)
    assert c_rel["n_done"] == k and counts("c_rel") == c_rel
    out, st, c_lk = m.lookup(np.arange(G), np.zeros(G, np.int32), cap=n)
    assert counts("c_lk") == c_lk and c_lk["n_done"] == k and A.get("lk_status").tolist() == st.tolist()
    for q, dt in L.LOOKUP_COLS:
        assert A.get("l_" + q, dt)[:k].tolist() == out[q].tolist(), q
    # every hit's (off, len) points at its own frame in the compacted bytes
    frame_of = {(int(a), int(b), int(c), int(d)): j for j, (a, b, c, d) in
                enumerate(zip(cols["gidx"], cols["slot"], cols["bnum"], cols["bcoord"]))}
    assert len(frame_of) == n
    comp = A.get("compacted")
    for j in range(k):
        f = frame_of[(int(out["rec"][j]), int(out["slot"][j]), int(out["bnum"][j]), int(out["bcoord"][j]))]  # rec i asks group i
        o, ln = int(out["off"][j]), int(out["len"][j])
        assert out["file"][j] == 1 and ln == lens[f] and int.from_bytes(comp[o:o + 4].tobytes(), "big") == ln
        assert comp[o + 4:o + 4 + ln].tobytes() == block[int(f_off[f]):int(f_off[f]) + ln].tobytes(), j
    written = {"journal": nbytes, "pack_counts": 32, "add_status": n, "gc_status": gcg.size, "compacted": int(jc.bytes_done),
               "verdict": k, "jg_counts": 64, "lk_status": G, "c_add": 32, "c_gc": 32, "c_fr": 32, "c_rel": 32, "c_lk": 32}
    written.update({"p_" + q: n * np.dtype(dt).itemsize for q, dt in JC.ROW_DT.items()})
    written.update({"f_" + q: k * np.dtype(dt).itemsize for q, dt in L.FILE_ROWS_COLS})
    written.update({"k_" + q: k * dt.itemsize for q, dt in JG.ROW_COLS})
    written.update({"l_" + q: k * np.dtype(dt).itemsize for q, dt in L.LOOKUP_COLS})
    A.unchanged_outside(written)
    # the file-deletion questions: file 0 holds no alive row and is no group's min file... except that min files do not
    # move under relocate (LogIndex.modify): they do at the groups' next checkpoint
    rows, groups, lo, _ = L.files(e, 0, 2)
    assert rows.tolist() == [0, k] and groups.tolist() == [100, 0] and lo == 0
    L.set_gc(e, np.arange(100), np.zeros(100, np.int32))
    rows, groups, lo, _ = L.files(e, 0, 2)
    assert rows.tolist() == [0, k] and groups.tolist() == [0, 100] and lo == 1
    e.close()


# g ---- tile rounds ---------------------------------------------------------------------------------------------------------
def test_more_than_256_tiles(hip_lib):
    """cap_rows 70,000 and 66,000 records: 274 tiles of rows and 258 of records, tile_offsets goes round twice"""
    cap, n, groups = 70000, 66000, 64
    e = make_engine(hip_lib, cap_rows=cap, max_batch=1 << 17, groups=groups, create=False)
    B = both(e, groups=groups, cap_rows=cap)
    i = np.arange(n, dtype=np.int64)
    g = ((i * 2654435761) >> 8) % groups
    st, c = LM.add_of(B, LM.recs(g, 1 + i), file=3)
    assert c["n_done"] == n
    st, c = LM.add_of(B, LM.recs(g, 70001 + i), file=4)
    assert c["n_done"] == cap - n and (st == LM.FULL).sum() == 2 * n - cap
    st, c = B.set_gc(np.arange(0, groups, 2), [40000] * (groups // 2))
    assert 15000 < c["n_stale"] < 25000
    out, _, c = B.lookup(np.arange(groups), [30000] * groups, [50000] * groups, [1] * groups, cap=5000)
    assert c["n_done"] == 5000 < c["n_hits"]
    B.file_rows(4, cap)
    B.files(0, 8)
    c = B.compact()
    assert c["n_rows"] == c["n_alive"] < cap - 15000
    B.lookup(np.arange(groups), [0] * groups, cap=cap)
    e.close()


# i ---- independence --------------------------------------------------------------------------------------------------------
def test_index_and_group_state_do_not_touch_each_other(hip_lib):
    """two engines take the same ACCEPT batches (gpx_accept_batch_dev), retirements and exports; one of them runs index
    calls on the same groups in between.  Their accept results, images and dumps are byte-equal, and the index of the
    one that has it follows the model whatever happens to the groups."""
    import torch
    from gigapaxos_amd import image
    ea, eb = make_engine(hip_lib), make_engine(hip_lib, cap_rows=0)
    B = both(ea)
    g = np.arange(G, dtype=np.int32)

    def accept_dev(e, slot):
        cols = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32)).cuda()
                for c in (g, np.zeros(G), np.full(G, CREATOR), np.full(G, slot), np.zeros(G))]
        fl = torch.zeros(G, dtype=torch.uint8, device="cuda")
        o = ([torch.zeros(G, dtype=torch.int32, device="cuda") for _ in range(3)] +
             [torch.zeros(G, dtype=torch.uint8, device="cuda") for _ in range(2)] +
             [torch.zeros(G, dtype=torch.int32, device="cuda") for _ in range(3)] + [torch.zeros(1, dtype=torch.int32, device="cuda")])
        e.call_dev("accept_batch", G, *[c.data_ptr() for c in cols], fl.data_ptr(), *[t.data_ptr() for t in o])
        e.sync()
        return [t.cpu().numpy().tobytes() for t in o[:5]]

    def images(e):
        rows = image.export_groups(e)[0]
        return np.asarray(rows).tobytes(), [e.dump(int(q)).tobytes() for q in (40, 64, 100, G - 1)]

    assert accept_dev(ea, 1) == accept_dev(eb, 1)
    LM.add_of(B, LM.recs(np.tile(g, 3), np.repeat([1, 2, 3], G)), file=0)
    B.set_gc(g[::2], [1] * (G // 2))
    assert images(ea) == images(eb)
    for e in (ea, eb):
        e.retire_groups(g[:32], RETIRE_PAUSE)
    B.lookup(g, [0] * G, cap=CAP)                                          # retired groups keep their rows
    B.set_gc(g[:8], None, LM.RESET)
    B.compact()
    assert accept_dev(ea, 2) == accept_dev(eb, 2)
    LM.add_of(B, LM.recs(g, [4] * G), file=1)
    B.files(0, 4)
    B.lookup(g, [0] * G, [3] * G, [1] * G, cap=CAP)
    assert images(ea) == images(eb)
    ea.close(), eb.close()
