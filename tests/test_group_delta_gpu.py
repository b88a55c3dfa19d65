"""Delta images (include/gpx_delta.h) on the GPU.  The reference for "changed" is the engine's own gpx_group_dump against
the dump at the export that last wrote the group (tests/delta_model.py), the reference for the rows is gpx_group_export
of the same groups; neither knows a signature.  Both forms write between 4 KiB guard bands of sentinels.  The traffic of
the mirror test is tests/delta_common.py, shown not to be vacuous on the CPU (tests/test_group_delta_model.py)."""
import ctypes

import numpy as np
import pytest

from gigapaxos_amd import S_OK, S_NOGROUP, C_HASVALUE, RETIRE_KILL, RETIRE_PAUSE
from gigapaxos_amd import checkpoint, image
from tests import delta_common as DC
from tests import image_common as IC
from tests import sweep_common as SC
from tests.delta_model import DeltaModel, EVICT, FULL

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 4096
N, T, ME = DC.N, image.IMAGE_TILE, DC.ME
SHAPES = list(DC.SHAPES)


def untouched(a):
    return bool((np.asarray(a).view(np.uint8) == SENTINEL).all())


def call_export(e, form, entries, flags, cap, cap_gone, null=False):
    """one call, its buffers between guard bands -> (rows region [cap, stride], gone region [cap_gone], counts tuple)"""
    stride = image.image_stride(int(e.cfg.kmax), int(e.cfg.window))
    n = N if entries is None else len(entries)
    nb_r, nb_g = cap * stride, cap_gone * 4
    if form == "host":
        g = None if entries is None else np.ascontiguousarray(entries, np.int32)
        rbuf, gbuf = np.full(2 * GUARD + nb_r + 16, SENTINEL, np.uint8), np.full(2 * GUARD + nb_g, SENTINEL, np.uint8)
        counts = image.DeltaCounts()
        vp = lambda a, ok: ctypes.c_void_p(a.ctypes.data + GUARD) if ok else None
        e.lib.check(e.lib.fn["group_export_delta"](e.h, n, None if g is None else g.ctypes.data_as(ctypes.c_void_p), flags, cap,
                                                   vp(rbuf, cap and not null), cap_gone, vp(gbuf, cap_gone and not null),
                                                   ctypes.byref(counts)), "group_export_delta")
        c = counts.as_tuple()
    else:
        import torch

        g = None if entries is None else torch.from_numpy(np.ascontiguousarray(entries, np.int32)).cuda()
        rt = torch.full((2 * GUARD + nb_r + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        gt = torch.full((2 * GUARD + nb_g,), SENTINEL, dtype=torch.uint8, device="cuda")
        ct = torch.full((2 * GUARD + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        image.export_delta_dev(e, n, 0 if g is None else g.data_ptr(), flags, cap, rt.data_ptr() + GUARD if cap and not null else 0,
                               cap_gone, gt.data_ptr() + GUARD if cap_gone and not null else 0, ct.data_ptr() + GUARD)
        e.sync()
        rbuf, gbuf, craw = rt.cpu().numpy(), gt.cpu().numpy(), ct.cpu().numpy()
        assert untouched(craw[:GUARD]) and untouched(craw[GUARD + 32:])
        c = image.DeltaCounts.from_buffer_copy(craw[GUARD:GUARD + 32].tobytes()).as_tuple()
    assert untouched(rbuf[:GUARD]) and untouched(rbuf[GUARD + nb_r:]) and untouched(gbuf[:GUARD]) and untouched(gbuf[GUARD + nb_g:])
    return rbuf[GUARD:GUARD + nb_r].reshape(cap, stride), gbuf[GUARD:GUARD + nb_g].view("<i4"), c


def table(e):
    """the dump of every group (None: dead) and, from one gpx_group_export of the whole table, the rows of every live one"""
    dumps = [tuple(e.dump(g).tolist()) for g in range(N)]
    dumps = [d if d[0] else None for d in dumps]
    rows, counts = image.export_groups(e, None)
    assert counts.n_done == counts.n_live == sum(d is not None for d in dumps)
    w = rows.view("<i4")
    by = {}
    for j in range(rows.shape[0]):
        by.setdefault(int(w[j, 5]), []).append(rows[j])
    return dumps, {g: np.stack(r) for g, r in by.items()}


def check(e, model, form, entries=None, flags=0, cap=None, cap_gone=None, what="", null=False, tab=None):
    """one delta export against the model over the engine's own dumps; returns the model's answer.  tab: table(e), where
    the caller knows that no state has changed since it was taken (a delta export without EVICT changes none)"""
    dumps, ref = tab or table(e)
    nrows = [ref[g].shape[0] if g in ref else 0 for g in range(N)]
    n_ent = N if entries is None else len(entries)
    cap = 2 * n_ent if cap is None else cap
    cap_gone = n_ent if cap_gone is None else cap_gone
    want = model.export(dumps, nrows, entries, flags, cap, cap_gone)
    rows, gone, counts = call_export(e, form, entries, flags, cap, cap_gone, null)
    tag = f"{what} {form} flags={flags} cap={cap} cap_gone={cap_gone}"
    print(f"{tag}: counts {counts}, model {want['counts']}")
    assert counts == want["counts"], tag
    if not null:
        k = want["counts"][4]
        exp = np.concatenate([ref[g] for g in want["written"]]) if want["written"] else rows[:0]
        assert rows[:k].tobytes() == exp.tobytes(), tag                       # byte for byte gpx_group_export's rows
        assert untouched(rows[k:]), f"{tag}: written at or beyond row {k}"
        assert gone[:len(want["listed"])].tolist() == want["listed"] and untouched(gone[len(want["listed"]):]), tag
    return want


def world(hip_lib, name):
    shape = DC.SHAPES[name]
    e = DC.engine(hip_lib, shape)
    IC.create(e, np.arange(N), shape["kmax"], shape["k"])
    return e, shape, DeltaModel(N)


def res(r, mod=16):
    g = np.arange(N, dtype=np.int32)
    return g[g % mod == r]


# 1 ---- baseline, nothing happened, every way state changes, pause and hot-restore ---------------------------------------
@pytest.mark.gpu_fast
@pytest.mark.parametrize("name", SHAPES)
def test_every_way_state_changes(hip_lib, name):
    e, shape, model = world(hip_lib, name)
    kmax, k = shape["kmax"], shape["k"]
    maj = k // 2 + 1
    forms = ["dev", "host"]
    step = [0]

    def delta(what, groups=None, gone=None):
        form = forms[step[0] % 2]
        step[0] += 1
        tab = table(e)
        w = check(e, model, form, what=what, tab=tab)
        if groups is not None:
            assert set(w["changed"]) == set(np.asarray(groups).tolist()), what
        assert w["gone"] == ([] if gone is None else sorted(np.asarray(gone).tolist())), what
        q = check(e, model, forms[step[0] % 2], what=what + ", nothing happened", tab=tab)   # ... and writes no byte
        assert q["counts"][1] == 0 and q["counts"][5] == 0
        return w

    w = check(e, model, "dev", flags=FULL, what="baseline")
    assert w["counts"][0] == w["counts"][1] == w["counts"][3] == N
    check(e, model, "host", what="nothing happened")
    check(e, model, "dev", what="nothing happened, counts only", cap=0, cap_gone=0, null=True)
    A, B, C, D, E, F, H, P = (res(r) for r in range(8))
    s0, bn, bc, med, st = e.propose(A)
    assert (st == S_OK).all()
    delta("propose", A)
    SC.bare_accepts(e, B, 0)
    delta("ACCEPT", B)
    d = e.accept_reply(A, bn, bc, s0, np.full(A.size, ME, np.int32), np.zeros(A.size, np.int32))
    assert d.gidx.size == 0
    delta("one accept reply below majority", A)
    for a in range(ME + 1, ME + maj):
        d = e.accept_reply(A, bn, bc, s0, np.full(A.size, a, np.int32), np.zeros(A.size, np.int32))
    assert d.gidx.size == A.size
    delta("accept replies to a decision", A)
    st, _ = e.commit(A, bn, bc, s0, med, np.full(A.size, C_HASVALUE, np.uint8))
    assert (st == S_OK).all()
    delta("commit", A)
    slot = e.snapshot(C)[0]["acc_slot"]
    st, runs = e.commit(C, np.zeros(C.size, np.int32), np.full(C.size, ME, np.int32), slot + 1, slot - 1,
                        np.full(C.size, C_HASVALUE, np.uint8))
    assert (st == S_OK).all() and runs.gidx.size == 0
    delta("commit with a gap", C)
    # a PREPARE at a higher ballot from another coordinator: the acceptor's ballot rises (a_bnum, a_bcoord)
    Q = res(8)
    out, _ = e.prepare(Q, np.full(Q.size, 5, np.int32), np.full(Q.size, ME + 1, np.int32), e.snapshot(Q)[0]["acc_slot"])
    assert (out[4] == S_OK).all() and (out[0] == 5).all() and (out[1] == ME + 1).all()
    snap = e.snapshot(Q)[0]
    assert (snap["acc_bnum"] == 5).all() and (snap["acc_bcoord"] == ME + 1).all()
    delta("prepare", Q)
    assert (e.election_begin(D, np.ones(D.size, np.int32)) == 0).all()
    w = delta("election begin", D)
    assert w["counts"][2] == 2 * D.size                                       # a second row appears
    for a in range(ME, ME + maj + 1):
        e.prepare_reply(D, np.full(D.size, a, np.int32), np.ones(D.size, np.int32), np.full(D.size, ME, np.int32),
                        e.snapshot(D)[0]["acc_slot"], None)
    w = delta("election end", D)
    assert w["counts"][2] == D.size
    checkpoint.checkpoint_batch(e, E, e.snapshot(E)[0]["acc_slot"] + 5)
    delta("checkpoint jump", E)
    rows, _ = image.export_groups(e, F)
    e.retire_groups(F, RETIRE_KILL)
    delta("retire", [], gone=F)
    assert (image.import_groups(e, rows) == S_OK).all()
    delta("gpx_group_import", F)
    e.retire_groups(H, RETIRE_KILL)
    IC.create(e, H, kmax, k, base_slot=9)
    delta("retire, then create with a different row", H)
    # pause and hot-restore from the group's own row: where the dumps are equal the group is neither changed nor gone
    before = {int(g): tuple(e.dump(int(g)).tolist()) for g in P}
    hri, st = e.retire_groups(P, RETIRE_PAUSE)
    assert (st == S_OK).all()
    assert (e.create_groups(P, SC.members_of(P.size, kmax, k), k, hri) == S_OK).all()
    same = [g for g in before if tuple(e.dump(g).tolist()) == before[g]]
    print(f"pause and hot-restore: {len(same)} of {P.size} groups have equal dumps")
    assert len(same) == P.size                    # (the groups are caught up: the restore row carries their whole state)
    delta("pause and hot-restore", [])
    e.close()


# 2 ---- caps and listed entries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("form", ["host", "dev"])
def test_caps_and_listed_entries(hip_lib, name, form):
    e, shape, model = world(hip_lib, name)
    k = shape["k"]
    two = np.unique(np.concatenate([res(3, 5), [0, 255, 256, 511, 512, N - 1]])).astype(np.int32)   # two rows each, on the edges too
    assert (e.election_begin(two, np.ones(two.size, np.int32)) == 0).all()
    tab = table(e)
    nrows = np.array([tab[1][g].shape[0] for g in range(N)])
    before = np.concatenate([[0], np.cumsum(nrows)])
    check(e, model, form, cap=0, cap_gone=0, null=True, what="counts only", tab=tab)
    w = check(e, model, form, cap=int(before[100]), what="inside tile 0", tab=tab)
    assert w["written"] == list(range(100))
    w = check(e, model, form, cap=int(before[T] - before[100]), what="on the edge of tile 0", tab=tab)
    assert w["written"] == list(range(100, T)) and nrows[T] == 2
    w = check(e, model, form, cap=int(before[T + 2] - before[T] + 1), what="one row short of a two-row group", tab=tab)
    assert nrows[T + 2] == 2 and w["written"] == [T, T + 1] and w["counts"][4] == 3    # it and everything after it stay
    seen = set(range(T + 2))
    for _ in range(40):                                                        # until nothing is left: 97 rows a call
        w = check(e, model, form, cap=97, what="the rest", tab=tab)
        assert not seen & set(w["written"])
        seen |= set(w["written"])
        if w["counts"][1] == w["counts"][3]:
            break
    assert seen == set(range(N)) and check(e, model, form, what="after", tab=tab)["counts"][1] == 0
    # cap_gone: cuts inside a tile and on its edge, until none is left
    dead = res(1, 3)
    e.retire_groups(dead, RETIRE_KILL)
    in0, tab = int((dead < T).sum()), table(e)
    got = []
    for cg in (0, 5, in0 - 5, 1, 30, N):
        w = check(e, model, form, cap_gone=cg, null=cg == 0, cap=0 if cg == 0 else None, what="gone", tab=tab)
        assert w["counts"][5] == dead.size - len(got)
        got += w["listed"]
    assert got == dead.tolist() and check(e, model, form, what="no gone left", tab=tab)["counts"][5] == 0
    # a listed, unordered, partial scan: unlisted groups keep their marks
    SC.touch_live(e, np.setdiff1d(np.arange(N), two), 3, k)
    lst = np.random.default_rng(5).permutation(N)[:300].astype(np.int32)
    lst[::50] = [-1, N, N + 7, -2**31, 2**31 - 1, -5]
    tab = table(e)
    w = check(e, model, form, entries=lst, what="listed", tab=tab)
    assert 0 < w["counts"][1] < 300
    w = check(e, model, form, what="the unlisted ones", tab=tab)
    assert w["counts"][1] > 0 and not set(w["written"]) & set(lst.tolist())
    e.close()


# 3 ---- EVICT --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "dev"])
def test_evict(hip_lib, form):
    e, shape, model = world(hip_lib, "k3-w8")
    check(e, model, form, flags=FULL, what="baseline")
    moving = res(2, 3)
    SC.touch(e, moving, 1, shape["k"])
    total = int(check(e, model, form, cap=0, cap_gone=0, null=True, what="count")["counts"][2])
    w = check(e, model, form, flags=EVICT, cap=total // 2, what="evict, cut")
    w2 = check(e, model, form, flags=EVICT, what="evict, the rest")
    out = np.array(w["written"] + w2["written"], np.int32)
    assert out.tolist() == moving.tolist()
    assert (e.propose(out)[4] == S_NOGROUP).all() and (e.snapshot(out)[1] == S_NOGROUP).all()
    w = check(e, model, form, what="after")                                   # dead, and not reported gone
    assert w["counts"][0] == N - moving.size and w["counts"][1] == 0 and w["counts"][5] == 0
    e.close()


class TakesOver:
    """engine `e` from now on in the place of the engine `other` mirrors: its counters continue the other's"""

    def __init__(self, e, other):
        self._e = e
        self._base = tuple(b - a for a, b in zip(e.counters(), other.counters()))

    def __getattr__(self, name):
        return getattr(self._e, name)

    def counters(self):
        return tuple(a + b for a, b in zip(self._e.counters(), self._base))


# 4 ---- mirror ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_mirror_follows_six_rounds_of_traffic(hip_lib, oracle_lib, name):
    from tests.parity_common import fuzz

    shape = DC.SHAPES[name]
    rng = np.random.default_rng(shape["seed"])
    eh, eo, em = DC.engine(hip_lib, shape), DC.engine(oracle_lib, shape), DC.engine(hip_lib, shape)
    DC.populate(eh, eo, shape, rng)
    c, st, gst = image.mirror_groups(eh, em, full=True)
    assert c.n_done == c.n_live == N and (st == S_OK).all()
    ctx = {}
    for r in range(DC.ROUNDS):
        DC.mirror_round(eh, eo, shape, rng, r, ctx)
        c, st, gst = image.mirror_groups(eh, em)
        print(f"{name} round {r}: {c.as_tuple()}")
        assert (st == S_OK).all() and (gst == S_OK).all() and 0 < c.n_changed < c.n_live and c.n_gone > 0
        for g in range(N):
            assert em.dump(g).tolist() == eh.dump(g).tolist() == eo.dump(g).tolist(), (r, g)
    c, st, gst = image.mirror_groups(eh, em)
    assert c.n_changed == 0 and c.n_gone == 0
    # the traffic goes on, on the mirror: its answers are the oracle's (the driver also compares the engines' call
    # counters, which are no group state: the mirror's count from the moment it takes over)
    em = TakesOver(em, eo)
    DC.mirror_round(em, eo, shape, rng, DC.ROUNDS, ctx)
    fuzz(em, eo, DC.FUZZ_G, DC.NODES, rng, steps=10, batch=300, gmap=DC.GMAP)
    for g in range(N):
        assert em.dump(g).tolist() == eo.dump(g).tolist(), g
    for e in (eh, eo, em):
        e.close()


# 5 ---- refusals, kernel names ---------------------------------------------------------------------------------------------------
def test_refusals_and_kernel_names(hip_lib):
    shape = DC.SHAPES["k3-w8"]
    e, _, model = world(hip_lib, "k3-w8")
    em = DC.engine(hip_lib, shape)
    IC.create(em, np.arange(N), shape["kmax"], shape["k"], base_slot=40)
    run = res(5, 7)
    assert (e.election_begin(run, np.ones(run.size, np.int32)) == 0).all()
    e.profile(2)
    rows, gone, counts = image.export_delta(e)
    assert set(e.profile_read()) >= {"k_delta_tile", "k_delta_offsets", "k_delta_move"}
    assert counts.n_done == N and counts.n_rows_done == N + run.size
    # a continuation row while the election arrays are missing, without GPX_IMG_VIEWCHANGE: the pair is refused
    before = [em.dump(g).tolist() for g in range(N)]
    st, _ = image.apply_delta(em, rows)
    w = rows.view("<i4")
    pair = np.isin(w[:, 5], run)
    assert (st[pair] == image.S_IMAGE).all() and (st[~pair] == S_OK).all()
    for g in run:
        assert em.dump(int(g)).tolist() == before[int(g)]
    # garbage rows aimed at live destinations: GPX_S_IMAGE, the destinations exactly as they were
    bad = rows.copy()
    bw = bad.view("<i4")
    mains = np.nonzero(bw[:, 1] == image.IMAGE_MAIN)[0]
    bw[mains[0::3], 0] = 9                                                    # not the format
    bw[mains[1::3], 15] = 1                                                   # the reserved word
    bw[mains[2::3], image.layout(3, 8)["acc"] + 3] |= 0x4000                  # an unknown bit in a ring's flag word
    before = [em.dump(g).tolist() for g in range(N)]
    em.profile(2)
    st, gst = image.apply_delta(em, bad, flags=image.IMG_VIEWCHANGE, gone=[3, -1, N])
    assert set(em.profile_read()) >= {"k_delta_check", "k_delta_apply", "k_delta_gone"}
    assert (st == image.S_IMAGE).all() and gst.tolist() == [S_OK, S_NOGROUP, S_NOGROUP]
    for g in range(N):
        assert em.dump(g).tolist() == before[g] if g != 3 else em.dump(g)[0] == 0, g
    # the rows as they were: every group is replaced (or created), the election words come with them
    st, gst = image.apply_delta(em, rows, flags=image.IMG_VIEWCHANGE)
    assert (st == S_OK).all() and gst.size == 0
    for g in range(N):
        assert em.dump(g).tolist() == e.dump(g).tolist(), g
    e.close()
    em.close()
