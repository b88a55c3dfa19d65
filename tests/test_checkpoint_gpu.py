"""Checkpoint transfer (include/gpx_checkpoint.h) on the GPU.  Three independent checks of one call: the Java reading
(tests/checkpoint_model.py) over enumerated op sequences, the CPU oracle fed one valued decision per skipped slot, and
the wrap cases worked out from the Java's two kinds of comparison.  Every leg runs with gpx_checkpoint_batch and with
gpx_checkpoint_batch_dev; both write into sentinel-filled buffers with padding behind n."""
import numpy as np
import pytest

from gigapaxos_amd import Engine, S_OK, S_NOGROUP, S_STOPPED, C_HASVALUE, C_STOP, hri_create, streams
from gigapaxos_amd import checkpoint as CK
from gigapaxos_amd import image as IM
from gigapaxos_amd import sweep as SW
from gigapaxos_amd import wire as WR
from gigapaxos_amd._abi import _p
from tests import checkpoint_model as M
from tests.acc_enum_common import COORD
from tests.parity_common import make_pair

pytestmark = pytest.mark.gpu

SENTINEL, PAD = 0xA5, 9
FORMS = ("host", "dev")
G = 3000


def filled(count, dtype):
    return np.frombuffer(bytes([SENTINEL]) * (count * np.dtype(dtype).itemsize), dtype).copy()


def untouched(a):
    return (np.asarray(a).view(np.uint8) == SENTINEL).all()


DENSE = (np.int32, np.int32, np.uint8, np.uint8)


def call(form, e, gidx, cp, flags=0):
    """one call in the given form -> ((from, to, flags, status), runs [k, 3], counts).  Every output column holds n + PAD
    sentinel entries: nothing behind n, no run entry at or beyond n_runs and nothing behind the 16 bytes of the counts
    may be written."""
    gidx, cp = np.ascontiguousarray(gidx, np.int32), np.ascontiguousarray(cp, np.int32)
    n = gidx.shape[0]
    peek = bool(flags & CK.CP_PEEK)
    if form == "host":
        dense = [filled(n + PAD, dt) for dt in DENSE]
        xs = [filled(n + PAD, np.int32) for _ in range(3)]
        cnt = filled(16 + PAD, np.uint8)
        e.lib.check(e.lib.fn["checkpoint_batch"](e.h, n, _p(gidx), _p(cp), int(flags), *[_p(a) for a in dense],
                                                 *[None if peek else _p(a) for a in xs], _p(cnt)), "checkpoint_batch")
    else:
        import torch

        def dev(count, dt):
            return torch.full((count * np.dtype(dt).itemsize,), SENTINEL, dtype=torch.uint8, device="cuda")
        td = [dev(n + PAD, dt) for dt in DENSE]
        tx = [dev(n + PAD, np.int32) for _ in range(3)]
        tc = dev(16 + PAD, np.uint8)
        tg, tcp = torch.from_numpy(gidx).cuda(), torch.from_numpy(cp).cuda()
        if n == 0:
            tg, tcp = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        CK.checkpoint_batch_dev(e, n, tg.data_ptr(), tcp.data_ptr(), flags, [t.data_ptr() for t in td],
                                [0, 0, 0] if peek else [t.data_ptr() for t in tx], tc.data_ptr())
        e.sync()
        dense = [t.cpu().numpy().view(dt) for t, dt in zip(td, DENSE)]
        xs = [t.cpu().numpy().view(np.int32) for t in tx]
        cnt = tc.cpu().numpy()
    assert untouched(cnt[16:]) and all(untouched(a[n:]) for a in dense)
    counts = CK.CpCounts.from_buffer_copy(cnt[:16].tobytes())
    k = counts.n_runs
    assert 0 <= k <= n and (not peek or k == 0)
    assert all(untouched(a[k:]) for a in xs), f"a run column was written at or beyond n_runs = {k}"
    runs = np.stack([a[:k] for a in xs], axis=1) if k else np.zeros((0, 3), np.int32)
    return tuple(a[:n] for a in dense), runs, counts


def engine(lib, n_groups, W, from_disk, starts=None, max_batch=1 << 17):
    e = Engine(lib, COORD + 1, n_groups, kmax=3, window=W, max_batch=max(max_batch, n_groups), flags=1 if from_disk else 0)
    if starts is not None:
        M.create_at(e, starts)
    return e


# 1 ---- enumeration against the Java reading -----------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("from_disk", [True, False])
@pytest.mark.parametrize("W", [pytest.param(8, marks=pytest.mark.gpu_fast), 4, 64])
def test_enumeration_against_the_java_reading(hip_lib, W, from_disk, form):
    """3,000 groups, one op sequence each: acc_enum_common's alphabet plus checkpoint records, every record followed by
    ACCEPTs or commits that observe what the jump left in the rings.  Every dense output, status, run, count, the final
    rows and sampled dumps against the model."""
    seqs = M.enum_sequences(W, n=G)
    e = engine(hip_lib, G, W, from_disk, starts=[1] * G)
    M.reset_coverage()
    _, checked = M.drive(seqs, W, from_disk, engine=e, checkpoint=lambda e_, gi, cp: call(form, e_, gi, cp))
    e.close()
    assert checked > 15000 and M.CP_COVERAGE["jump_gt_W"] and M.CP_COVERAGE["tail_valued"]


# 2 ---- differential against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("from_disk", [True, False])
@pytest.mark.parametrize("W", [4, 8, 64])
def test_differential_against_the_oracle(hip_lib, oracle_lib, W, from_disk, form):
    """One history on both engines; then checkpoint records on the HIP engine and, on the oracle, one valued decision per
    skipped slot (d = 1, W - 1, W, W + 1, 5,000 for a handful of groups).  The dump of EVERY group of the table, the gap
    scan and a mixed-op fuzz continued on both must agree."""
    ds = (1, W - 1, W, W + 1, 5000)
    history, cps = M.diff_plan(G, W, from_disk, ds, every=250)
    assert len(cps) == G // 250
    eh, eo = engine(hip_lib, G, W, from_disk, [1] * G), engine(oracle_lib, G, W, from_disk, [1] * G)
    mh, _ = M.drive(history, W, from_disk, engine=eh, dumps=0)
    mo, _ = M.drive(history, W, from_disk, engine=eo, dumps=0)
    gi, sl, md = M.decisions_for(mo, cps)
    st, runs_o = eo.commit(gi, np.zeros(gi.size, np.int32), np.full(gi.size, COORD, np.int32), sl, md,
                           np.full(gi.size, C_HASVALUE, np.uint8))
    assert set(st.tolist()) <= {S_OK, S_STOPPED}
    slot0 = {g: int(mo[g]._slot) for g, _ in cps}
    (frm, to, fl, status), runs, counts = call(form, eh, [g for g, _ in cps], [cp for _, cp in cps])
    assert (status == S_OK).all() and (fl == (CK.CP_ADOPT | CK.CP_MOVED)).all()
    assert frm.tolist() == [slot0[g] for g, _ in cps]
    assert (counts.n_adopted, counts.n_nogroup, counts.n_stopped) == (len(cps), 0, 0)
    # the oracle's runs of a group continue one another from its slot: (slot, d + t) against the call's (cp + 1, t)
    cp_of = dict(cps)
    tails = {int(g): int(c) for g, f, c in runs.tolist()}
    assert all(int(f) == cp_of[int(g)] + 1 and c > 0 for g, f, c in runs.tolist()) and len(tails) == counts.n_runs
    total = {}
    for g, f, c in runs_o.as_tuple_array().tolist():
        assert f == slot0[g] + total.get(g, 0)
        total[g] = total.get(g, 0) + c
    for (g, cp), t_ in zip(cps, to.tolist()):
        assert total[g] == cp + 1 - slot0[g] + tails.get(g, 0) and t_ == cp + 1 + tails.get(g, 0)
    every = np.arange(G, dtype=np.int32)

    def same_everywhere(what, through_images=False):
        """gpx_group_dump against orc_group_dump for every group of the table, untouched neighbours included (the second
        time the HIP side's dump words come from one export of the whole table: a dump call costs a copy per ring entry)"""
        hip = IM.rows_to_dumps(IM.export_groups(eh)[0], 3, W) if through_images else None
        assert hip is None or len(hip) == G
        for g in range(G):
            a, b = (hip[g] if hip else eh.dump(g)), eo.dump(g)
            assert a.shape == b.shape and (a == b).all(), (what, g, a.tolist(), b.tolist())
        wh, wo = WR.WireEngine(eh), WR.WireEngine(eo)
        for x, y in zip(WR.gap_scan(wh, every, 1), WR.gap_scan(wo, every, 1)):
            assert (x == y).all(), what
    same_everywhere("after the checkpoint")
    # a mixed-op fuzz continued on both: the models only supply the ops' slots
    for g, cp in cps:
        mh[g].handleCheckpoint(cp)
        mo[g].handleCheckpoint(cp)
    rng = np.random.default_rng(W + 7)
    probe = [tuple(M._ops_near(rng, int(mh[g]._slot), 5)) for g in range(G)]
    M.drive(probe, W, from_disk, engine=eh, dumps=0, models=mh)
    M.drive(probe, W, from_disk, engine=eo, dumps=0, models=mo)
    same_everywhere("after the fuzz", through_images=True)
    eh.close()
    eo.close()


# 3 ---- the int wrap -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("from_disk", [True, False])
def test_wrap(hip_lib, from_disk, form):
    """Groups restored at Integer.MAX_VALUE - 3 and MIN_VALUE + 3: cp = MAX_VALUE makes the target MIN_VALUE; a slot just
    past MIN_VALUE with a positive cp is adopted and does not move; a slot near MAX_VALUE with cp past the wrap is not
    adopted.  Against the model."""
    ws = M.wrap_sequences() * 40                                   # more than one wave of them
    starts = [a for a, _ in ws]
    e = engine(hip_lib, len(ws), 8, from_disk, starts=starts)
    M.reset_coverage()
    M.drive([s for _, s in ws], 8, from_disk, starts=starts, engine=e,
            checkpoint=lambda e_, gi, cp: call(form, e_, gi, cp), dumps=len(ws))
    e.close()
    assert M.CP_COVERAGE["wrap_adopted_not_moved"] and M.CP_COVERAGE["wrap_not_adopted"]


# 4 ---- states built by import: the tail rebuilt from an accept -------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("from_disk", [True, False])
def test_tail_rebuilt_from_an_accept(hip_lib, from_disk, form):
    """A placeholder next to the ACCEPT that matches it is a state no handler sequence reaches from empty maps; a group
    image can hold it.  The groups are exported, given such acceptors, imported again and sent checkpoint records."""
    cases = M.STATE_CASES * 70
    n = len(cases)
    e = engine(hip_lib, n, 8, from_disk, starts=[1] * n)
    rows, _ = IM.export_groups(e, flags=IM.IMG_EVICT)
    assert rows.shape[0] == n
    assert (IM.import_groups(e, M.state_image_rows(rows, cases, 8)) == S_OK).all()
    models = [M.state_model(c, 8, from_disk) for c in cases]
    M.reset_coverage()
    M.drive([(("J", c[4], 0, 0, 0),) for c in cases], 8, from_disk, engine=e, models=models, dumps=n,
            checkpoint=lambda e_, gi, cp: call(form, e_, gi, cp))
    e.close()
    assert M.CP_COVERAGE["tail_rebuilt"] == 3 * 70 and M.CP_COVERAGE["tail_stopped"] == 70


# 5 ---- statuses, counts, guards; peek -------------------------------------------------------------------------------------
def mixed_table(lib, from_disk=True):
    """3,000 rows: every 7th dead, every 11th stopped (a stop executed at slot 1), the others with a commit parked at 3"""
    g = np.arange(G)
    dead, stopped = g % 7 == 3, (g % 11 == 5) & (g % 7 != 3)
    e = engine(lib, G, 8, from_disk)
    alive = np.nonzero(~dead)[0].astype(np.int32)
    rows = hri_create(alive.size, 3, COORD)
    mem = np.tile(np.array([COORD, COORD + 1, COORD + 2], np.int32), (alive.size, 1))
    assert (e.create_groups(alive, mem, 3, rows) == S_OK).all()
    sg = np.nonzero(stopped)[0].astype(np.int32)
    one = np.ones(sg.size, np.int32)
    st, _ = e.commit(sg, 0 * one, COORD * one, one, -one, np.full(sg.size, C_HASVALUE | C_STOP, np.uint8))
    assert (st == S_OK).all()
    pg = np.nonzero(~dead & ~stopped)[0].astype(np.int32)
    one = np.ones(pg.size, np.int32)
    st, _ = e.commit(pg, 0 * one, COORD * one, 3 * one, -one, np.full(pg.size, C_HASVALUE, np.uint8))
    assert (st == S_OK).all()
    return e, dead, stopped


def whole_state(e):
    """every word of every live group, in one call"""
    rows, counts = IM.export_groups(e)
    return rows.tobytes(), counts.as_tuple()


@pytest.mark.parametrize("form", FORMS)
def test_statuses_counts_and_peek(hip_lib, form):
    """Dead, out-of-range and stopped groups between live ones: every status, every byte of the counts, nothing written
    at or beyond n_runs.  Under PEEK nothing changes and o_to / o_flags are what the applying call then reports for step
    2."""
    e, dead, stopped = mixed_table(hip_lib)
    gi = np.concatenate([np.arange(G), [-1, G, G + 5, -2**31, 2**31 - 1]]).astype(np.int32)
    rng = np.random.default_rng(3)
    gi = gi[rng.permutation(gi.size)]
    cp = rng.choice([-5, 0, 1, 2, 3, 9, 100], size=gi.size).astype(np.int32)
    inr = (gi >= 0) & (gi < G)
    nog = ~inr
    nog[inr] = dead[gi[inr]]
    stp = np.zeros(gi.size, bool)
    stp[inr] = stopped[gi[inr]]
    live = ~nog & ~stp
    adopt = live & (cp >= 1)
    # step 2 leaves cp + 1; the tail executes slot 3 iff the jump ends there (cp == 2); cp < 1 adopts nothing and finds
    # nothing parked at slot 1
    to2 = np.where(adopt, cp + 1, 1)
    tail = live & (cp == 2)
    before = whole_state(e)
    for _ in range(2):
        (frm, to, fl, st), runs, counts = call(form, e, gi, cp, CK.CP_PEEK)
        assert st.tolist() == np.where(nog, S_NOGROUP, np.where(stp, S_STOPPED, S_OK)).tolist()
        assert frm.tolist() == np.where(live, 1, 0).tolist() and to.tolist() == np.where(live, to2, 0).tolist()
        assert fl.tolist() == np.where(adopt, CK.CP_ADOPT | CK.CP_MOVED, 0).tolist()
        assert (counts.n_adopted, counts.n_nogroup, counts.n_stopped, counts.n_runs) == (adopt.sum(), nog.sum(), stp.sum(), 0)
        assert whole_state(e) == before                            # not a word of any group changed
    (frm, to, fl, st), runs, counts = call(form, e, gi, cp)
    assert st.tolist() == np.where(nog, S_NOGROUP, np.where(stp, S_STOPPED, S_OK)).tolist()
    assert frm.tolist() == np.where(live, 1, 0).tolist()
    assert to.tolist() == np.where(live, to2 + tail, 0).tolist()   # step 2 as the peek said, then the tail
    assert fl.tolist() == np.where(adopt, CK.CP_ADOPT | CK.CP_MOVED, 0).tolist()
    assert (counts.n_adopted, counts.n_nogroup, counts.n_stopped, counts.n_runs) == (adopt.sum(), nog.sum(), stp.sum(), tail.sum())
    assert runs.tolist() == [[int(g), 3, 1] for g in gi[tail]]     # compacted in record order
    assert tail.sum() > 100 and nog.sum() > 400 and stp.sum() > 200
    (frm, to, fl, st), runs, counts = call(form, e, gi[:0], cp[:0])    # n == 0 writes the counts
    assert (counts.n_adopted, counts.n_nogroup, counts.n_stopped, counts.n_runs) == (0, 0, 0, 0)
    e.close()


# 6 ---- more than 256 tiles in one call --------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_70000_groups_in_one_call(hip_lib, form):
    """One table of 70,000 groups, one call of 70,000 records (274 tiles: more than one round of k_cp_offsets), against the
    model: every dense output, every run, the counts and every final row."""
    n = 70_000
    e = engine(hip_lib, n, 8, True, starts=[1] * n)
    g = np.arange(n, dtype=np.int32)
    park = g[g % 3 == 0]                                           # a valued commit parked at 3 ... or at 2 + g % 5
    one = np.ones(park.size, np.int32)
    st, _ = e.commit(park, 0 * one, COORD * one, 2 + park % 5, -one, np.full(park.size, C_HASVALUE, np.uint8))
    assert (st == S_OK).all()
    cp = (g % 13 - 2).astype(np.int32)
    cp[g % 1000 == 999] = 5000
    models = []
    want, want_runs = [], []
    for i in range(n):
        m = M.CpAcceptor(1, (0, COORD), -1, True, 8)
        if i % 3 == 0:
            m.apply(("D", 2 + i % 5, 0, -1, 0))
        s, adopt, frm, to, run = m.handleCheckpoint(int(cp[i]))
        want.append((s, frm, to, (CK.CP_ADOPT if adopt else 0) | (CK.CP_MOVED if to != frm else 0)))
        if run:
            want_runs.append([i, int(run[0]), int(run[1])])
        models.append(m)
    (frm, to, fl, st), runs, counts = call(form, e, g, cp)
    assert list(zip(st.tolist(), frm.tolist(), to.tolist(), fl.tolist())) == want
    assert runs.tolist() == want_runs and len(want_runs) > 1000
    assert (counts.n_adopted, counts.n_nogroup, counts.n_stopped, counts.n_runs) == (sum(w[3] & 1 for w in want), 0, 0, len(want_runs))
    snap, s2 = e.snapshot(g)
    assert (s2 == S_OK).all()
    assert snap["acc_slot"].tolist() == [int(m._slot) for m in models]
    assert snap["acc_gc_slot"].tolist() == [int(m.acceptedGCSlot) for m in models]
    for i in list(range(0, 600, 7)) + [255, 256, 65535, 65536, n - 1]:
        assert M.parse_dump(e.dump(i), models[i]._slot) == models[i].dump_maps(), i
    e.close()


# 7 ---- neighbours ---------------------------------------------------------------------------------------------------------
def test_a_jumped_group_exports_and_imports_to_an_equal_dump(hip_lib):
    seqs = M.enum_sequences(8, n=600)
    e = engine(hip_lib, 600, 8, True, starts=[1] * 600)
    M.drive(seqs, 8, True, engine=e, checkpoint=lambda e_, gi, cp: call("host", e_, gi, cp), dumps=0)
    rows, counts = IM.export_groups(e)
    e2 = engine(hip_lib, 600, 8, True)
    assert (IM.import_groups(e2, rows) == S_OK).all()
    for g in range(600):
        assert e.dump(g).tolist() == e2.dump(g).tolist(), g
    e.close()
    e2.close()


def test_the_pause_sweep_sees_a_jumped_group_as_changed(hip_lib):
    e = engine(hip_lib, 600, 8, True, starts=[1] * 600)
    for _ in range(3):
        SW.pause_sweep(e, min_age=255)                             # nobody is that old: ages 0, 1, 2
    jumped = np.array([0, 63, 64, 255, 256, 257, 599], np.int32)
    (frm, to, fl, st), runs, counts = call("dev", e, jumped, np.full(jumped.size, 41, np.int32))
    assert (to == 42).all() and counts.n_adopted == jumped.size
    (gi, age, _), c = SW.pause_sweep(e, min_age=0, flags=SW.SWEEP_PEEK | SW.SWEEP_HOLD)
    assert gi.tolist() == list(range(600))                          # all caught up, the jumped ones too
    want = np.full(600, 2)
    want[jumped] = 0
    assert age.tolist() == want.tolist()
    e.close()


def test_an_async_accept_reply_call_in_flight_still_equals_the_oracle(hip_lib, oracle_lib):
    n, k = 30_000, 3
    eh, eo = make_pair(hip_lib, oracle_lib, 100, n, k, 8, max_batch=n * k + 4096)
    mem = np.tile(np.array([100, 101, 102], np.int32), (n, 1))
    for e in (eh, eo):
        assert (e.create_groups(np.arange(n), mem, k, hri_create(n, k, 100)) == S_OK).all()
    g = np.arange(n, dtype=np.int32)
    lag = g[g % 3 == 1]
    for r in range(3):
        po = eo.propose(g)
        ph = eh.propose_async(g).wait()
        for x, y in zip(ph, po):
            assert (x == y).all()
        cols = streams.vote_round(n, [100, 101, 102], r, 100)
        tv = eh.accept_reply_async(*cols)
        out = call("host" if r % 2 else "dev", eh, lag, np.full(lag.size, 10 * (r + 1), np.int32))
        do = eo.accept_reply(*cols)
        dh = tv.wait()
        a, b = dh.as_tuple_array(), do.as_tuple_array()
        assert a.shape == b.shape and (a == b).all() and (dh.status == do.status).all(), r
        assert (out[0][1] == 10 * (r + 1) + 1).all() and (out[0][3] == S_OK).all()
    assert eh.snapshot(lag)[0]["acc_slot"].tolist() == [31] * lag.size
    eh.close()
    eo.close()
