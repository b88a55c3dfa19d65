"""Group images (include/gpx_image.h) on the GPU.  One history (tests/image_common.py) is applied to a HIP engine and to
the CPU oracle; the expected rows are tests/image_model.py over the ORACLE's dumps - neither the kernels nor
gigapaxos_amd/image.py have a part in them.  Both forms write into sentinel-filled buffers with padding behind cap."""
import numpy as np
import pytest

from gigapaxos_amd import S_OK, S_NOGROUP, S_EXISTS, RETIRE_KILL
from gigapaxos_amd import image, sweep
from tests import image_common as IC
from tests import sweep_common as SC
from tests import image_model as M

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
PAD = 3                                   # rows behind cap that no call may touch
T = image.IMAGE_TILE                      # entries per workgroup of the export's first launch (GPX_IMAGE_TILE_ENTRIES)
G3 = 3 * T + 1
EDGES = np.unique([0, 63, 64, 255, 256, T - 1, T, 2 * T - 1, 2 * T, 3 * T])
S_IMAGE = image.S_IMAGE


def untouched(a):
    return (np.asarray(a).view(np.uint8) == SENTINEL).all()


def export_host(e, gidx, n, flags, cap, null=False):
    stride = image.image_stride(int(e.cfg.kmax), int(e.cfg.window))
    out = None if null else np.full((cap + PAD) * stride, SENTINEL, np.uint8)
    rows, counts = image.export_groups(e, gidx, flags, cap=cap, n=n, out=out)
    return (None if null else out.reshape(-1, stride)), counts


def export_dev(e, gidx, n, flags, cap, null=False):
    import torch

    stride = image.image_stride(int(e.cfg.kmax), int(e.cfg.window))
    buf = None if null else torch.full(((cap + PAD) * stride,), SENTINEL, dtype=torch.uint8, device="cuda")
    cnt = torch.full((16 + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    g = None if gidx is None else torch.from_numpy(np.ascontiguousarray(gidx, np.int32)).cuda()
    torch.cuda.synchronize()
    image.export_groups_dev(e, n, 0 if g is None else g.data_ptr(), flags, cap, 0 if null else buf.data_ptr(), cnt.data_ptr())
    e.sync()
    raw = cnt.cpu().numpy()
    assert untouched(raw[16:])
    counts = image.ImageCounts.from_buffer_copy(raw[:16].tobytes())
    return (None if null else buf.cpu().numpy().reshape(-1, stride)), counts


EXPORT = {"host": export_host, "dev": export_dev}


def expect_export(expected, groups, cap):
    """the rows and counts of an export over entries `groups`: a restatement of include/gpx_image.h"""
    rows, n_live, n_rows, n_done, cut = [], 0, 0, 0, False
    for g in groups:
        r = expected.get(int(g))
        if r is None:
            continue
        n_live += 1
        n_rows += r.shape[0]
        if not cut and sum(x.shape[0] for x in rows) + r.shape[0] <= cap:
            rows.append(r)
            n_done += 1
        else:
            cut = True
    done = np.concatenate(rows) if rows else np.zeros((0, 0), np.uint8)
    return done, (n_live, n_rows, n_done, done.shape[0])


def check_export(e, expected, form, gidx, n, flags, cap, null=False, what=""):
    groups = np.arange(n) if gidx is None else np.asarray(gidx, np.int64)
    want, counts = expect_export(expected, groups, cap)
    out, got = EXPORT[form](e, gidx, n, flags, cap, null)
    tag = f"{what} {form} flags={flags} cap={cap}"
    print(f"{tag}: counts {got.as_tuple()}, model {counts}")
    assert got.as_tuple() == counts, tag
    if out is not None:
        k = counts[3]
        assert out[:k].tobytes() == want.tobytes(), tag
        assert untouched(out[k:]), f"{tag}: written at or beyond row {k}"
    return counts, groups


def build(hip_lib, oracle_lib, n, kmax=3, k=3, window=8, edges=(), n_hip=None):
    eh, eo = IC.engine(hip_lib, n_hip or n, kmax, window), IC.engine(oracle_lib, n, kmax, window)
    cat, dead = IC.categories(n, edges), IC.dead_groups(n, edges)
    for e in (eh, eo):
        IC.create(e, np.arange(n), kmax, k)
        ctx = IC.first_half(e, n, cat, k, dead)
    expected = {}
    for g in range(n):
        d = eo.dump(g)
        if d[0]:
            expected[g] = M.row_from_dump(d, g, IC.ME, kmax, window)
    return dict(eh=eh, eo=eo, n=n, cat=cat, dead=dead, ctx=ctx, expected=expected, kmax=kmax, k=k, window=window)


@pytest.fixture(scope="module")
def world(hip_lib, oracle_lib):
    """3 T + 1 groups in every state, the groups at the wave and tile edges running for coordinator; never changed"""
    w = build(hip_lib, oracle_lib, G3, edges=EDGES)
    yield w
    w["eh"].close()
    w["eo"].close()


def lists():
    rng = np.random.default_rng(3)
    strided = np.concatenate([np.arange(1, G3, 3)[:100], [-1, G3, G3 + 5, -2**31, 2**31 - 1], np.arange(1, G3, 3)[100:]])
    return {"all": None, "ascending": np.arange(G3), "descending": np.arange(G3)[::-1].copy(), "strided": strided,
            "shuffled": rng.permutation(G3)}


# 1 ---- export equals the model over the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "dev"])
def test_export_equals_the_model_over_the_oracle(world, form):
    eh, exp = world["eh"], world["expected"]
    for _ in range(2):
        sweep.pause_sweep(eh, None, min_age=255, cap=0)                      # the idle words exist and hold ages
    ages0 = sweep.pause_sweep(eh, None, min_age=0, flags=sweep.SWEEP_PEEK | sweep.SWEEP_HOLD)[0]
    assert sum(1 for g in EDGES if exp[int(g)].shape[0] == 2) == EDGES.size   # a two-row group on every edge
    for name, gidx in lists().items():
        n = G3 if gidx is None else len(gidx)
        counts, groups = check_export(eh, exp, form, gidx, n, 0, 2 * n + 5, what=name)
        assert counts[1] > counts[0] > 0 and counts[2] == counts[0]
        if name == "strided":
            assert counts[0] < n - 5                                          # dead entries and entries out of range
        check_export(eh, exp, form, gidx, n, 0, 0, null=True, what=name + ", counts only")
        check_export(eh, exp, form, gidx, n, 0, counts[1], what=name + ", cap = n_rows")
    # a cut inside a tile, and cuts exactly between the two rows of a group that runs for coordinator
    check_export(eh, exp, form, None, G3, 0, 100, what="cut inside a tile")
    for edge in (63, 64, T, 2 * T - 1):
        before = sum(exp[g].shape[0] for g in range(edge) if g in exp)
        counts, _ = check_export(eh, exp, form, None, G3, 0, before + 1, what=f"cut inside group {edge}")
        assert counts[3] == before and counts[2] == sum(1 for g in range(edge) if g in exp)
    check_export(eh, exp, form, None, G3, 0, 1, what="cap 1: the first group needs two rows")
    # nothing has changed: every dump, every sweep age
    for g in range(G3):
        assert eh.dump(g).tolist() == world["eo"].dump(g).tolist(), g
    ages1 = sweep.pause_sweep(eh, None, min_age=0, flags=sweep.SWEEP_PEEK | sweep.SWEEP_HOLD)[0]
    assert ages0[0].tolist() == ages1[0].tolist() and ages0[1].tolist() == ages1[1].tolist() and ages0[1].any()


def test_export_of_a_shape_with_whole_chunks_and_limits(hip_lib, oracle_lib):
    """kmax 16, window 64: 624 words per row, 20 chunks, the last one half used; and the n limit"""
    import ctypes as C

    w = build(hip_lib, oracle_lib, T + 1, kmax=16, k=16, window=64, edges=[0, 63, 64, 255, 256])
    for form in ("host", "dev"):
        check_export(w["eh"], w["expected"], form, None, T + 1, 0, 2 * T + 2, what="K16 W64")
    counts = image.ImageCounts()
    n_max = max(int(w["eh"].cfg.max_groups), int(w["eh"].cfg.max_batch))
    assert w["eh"].lib.fn["group_export"](w["eh"].h, n_max + 1, None, 0, 0, None, C.byref(counts)) == -2
    w["eh"].close()
    w["eo"].close()


# 2 ---- evict ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "dev"])
def test_evict_retires_exactly_the_groups_written(hip_lib, oracle_lib, form):
    from gigapaxos_amd import wire as W

    w = build(hip_lib, oracle_lib, G3, edges=EDGES)
    eh, exp = w["eh"], w["expected"]
    names = [b"svc-%d" % g for g in range(G3)]
    wh = W.WireEngine(eh)
    assert (wh.bind(names, np.arange(G3)) == S_OK).all()
    for _ in range(2):
        sweep.pause_sweep(eh, None, min_age=255, cap=0)                      # caught-up groups now have an age of 1
    aged = dict(zip(*[c.tolist() for c in sweep.pause_sweep(eh, None, min_age=0, flags=3)[0][:2]]))
    assert sum(1 for a in aged.values() if a == 1) > 100
    idle = np.array([g for g in range(T) if w["cat"][g] == IC.IDLE and g in exp][:20], np.int32)
    hri = eh.snapshot(idle)[0]                                               # (idle groups: these rows hold all of them)
    before = sum(exp[g].shape[0] for g in range(T) if g in exp)
    counts, _ = check_export(eh, exp, form, None, G3, image.IMG_EVICT, before + 1, what="evict, cut inside group T")
    gone = np.array([g for g in range(T) if g in exp], np.int32)
    rest = np.array([g for g in range(T, G3) if g in exp], np.int32)
    assert counts[2] == gone.size
    st = eh.snapshot(np.arange(G3, dtype=np.int32))[1]
    assert (st[gone] == S_NOGROUP).all() and (st[rest] == S_OK).all() and (st[w["dead"]] == S_NOGROUP).all()
    frames = [W.batched_accept_reply(names[g], g % 5, 101, 0, 100, 0, [1]) for g in range(G3)]
    fs = wh.decode(frames).f_status
    assert (fs[gone] == W.W_NOGROUP).all() and (fs[rest] == W.W_OK).all()
    for g in rest:
        assert eh.dump(int(g)).tolist() == w["eo"].dump(int(g)).tolist()
    # the eviction cleared the idle words: the same state created again in the same row starts at age 0 (gpx_group_create
    # leaves these words alone, and an unchanged signature would go on ageing)
    assert (eh.create_groups(idle, SC.members_of(idle.size, 3, 3), 3, hri) == S_OK).all()
    for g in idle:
        assert eh.dump(int(g)).tolist() == w["eo"].dump(int(g)).tolist()
    aged1 = dict(zip(*[c.tolist() for c in sweep.pause_sweep(eh, None, min_age=0, flags=3)[0][:2]]))
    assert all(aged[int(g)] == 1 and aged1[int(g)] == 0 for g in idle)
    # so does an import: groups that gpx_group_retire killed (it keeps the idle words) come back from their images
    killed = np.array([g for g in rest.tolist() if aged.get(g) == 1][:40], np.int32)
    eh.retire_groups(np.concatenate([killed, idle]), RETIRE_KILL)
    assert (image.import_groups(eh, all_rows(exp, killed), None, image.IMG_VIEWCHANGE) == S_OK).all()
    aged1 = dict(zip(*[c.tolist() for c in sweep.pause_sweep(eh, None, min_age=0, flags=3)[0][:2]]))
    assert killed.size == 40 and all(aged1[g] == 0 for g in killed.tolist())
    aged.update({g: 0 for g in killed.tolist()})
    # the evicted rows are free again: the images go back, with idle words of 0 (the others keep their age)
    rows = np.concatenate([exp[int(g)] for g in gone])
    assert (image.import_groups(eh, rows, None, image.IMG_VIEWCHANGE) == S_OK).all()
    aged2 = dict(zip(*[c.tolist() for c in sweep.pause_sweep(eh, None, min_age=0, flags=3)[0][:2]]))
    assert all(aged2[g] == 0 for g in gone.tolist() if g in aged2) and sum(1 for g in gone.tolist() if g in aged2) > 30
    assert all(aged2[g] == aged[g] for g in rest.tolist() if g in aged)
    fs = wh.decode(frames).f_status
    assert (fs[gone] == W.W_OK).all()
    w["eh"].close()
    w["eo"].close()


# 3 ---- import ---------------------------------------------------------------------------------------------------------------
def all_rows(exp, groups):
    return np.concatenate([exp[int(g)] for g in groups if int(g) in exp])


def row_gidx(rows, dest_of):
    """the gidx column of an import: dest_of[source gidx] for main rows, garbage for continuation rows"""
    w = rows.view("<i4")
    return np.array([dest_of[int(r[5])] if r[1] == M.MAIN else -12345 for r in w], np.int32)


def test_import_into_a_fresh_engine(world, hip_lib):
    from gigapaxos_amd import wire as W

    exp, eo, n = world["expected"], world["eo"], world["n"]
    live = np.array(sorted(exp), np.int32)
    rows = all_rows(exp, live)
    # (a) gidx == NULL, the _dev form through move-free plumbing: restoring a snapshot into an engine of the same shape
    e1 = IC.engine(hip_lib, n)
    names = [b"svc-%d" % g for g in range(n)]
    w1 = W.WireEngine(e1)
    assert (w1.bind(names, np.arange(n)) == S_OK).all()
    frames = [W.batched_accept_reply(names[g], g % 5, 101, 0, 100, 0, [1]) for g in range(n)]
    assert (w1.decode(frames).f_status == W.W_NOGROUP).all()
    st = image.import_groups(e1, rows, None, 0)
    has_cont = rows.view("<i4")[:, 1] == M.CONT
    main_cont = np.roll(has_cont, -1) & ~has_cont
    assert (st[has_cont | main_cont] == S_IMAGE).all() and (st[~(has_cont | main_cont)] == S_OK).all()   # no election arrays yet
    st = image.import_groups(e1, rows, None, image.IMG_VIEWCHANGE)           # the same call with the flag
    assert (st[has_cont | main_cont] == S_OK).all() and (st[~(has_cont | main_cont)] == S_EXISTS).all()
    for g in range(n):
        assert e1.dump(g).tolist() == eo.dump(g).tolist(), g
    out, counts = export_dev(e1, None, n, 0, rows.shape[0])
    assert out[:rows.shape[0]].tobytes() == rows.tobytes()                   # export(import(rows)) == rows
    fs = w1.decode(frames).f_status
    assert (fs[live] == W.W_OK).all() and (fs[world["dead"]] == W.W_NOGROUP).all()   # decodes with the image's version
    wrong = [W.batched_accept_reply(names[g], g % 5 + 1, 101, 0, 100, 0, [1]) for g in live[:50]]
    assert (w1.decode(wrong).f_status == W.W_VERSION).all()
    e1.close()
    # (b) permuted destinations in a table of another size
    n2 = n + 300
    e2 = IC.engine(hip_lib, n2)
    rng = np.random.default_rng(9)
    dest = dict(zip(live.tolist(), rng.permutation(n2)[:live.size].tolist()))
    st = image.import_groups(e2, rows, row_gidx(rows, dest), image.IMG_VIEWCHANGE)
    assert (st == S_OK).all()
    for g in live:
        assert e2.dump(dest[int(g)]).tolist() == eo.dump(int(g)).tolist(), g
    order = sorted(live.tolist(), key=lambda g: dest[g])
    want = all_rows(exp, order).copy()
    wv = want.view("<i4")
    wv[:, 5] = [dest[int(x)] for x in wv[:, 5]]
    out, counts = export_host(e2, None, n2, 0, want.shape[0])
    assert counts.as_tuple() == (live.size, want.shape[0], live.size, want.shape[0])
    assert out[:want.shape[0]].tobytes() == want.tobytes()
    e2.close()


def bad_rows(exp, stride):
    """(what, rows uint8 [1 or 2, stride], expected statuses) for every cause of GPX_S_IMAGE in include/gpx_image.h"""
    one = next(exp[g] for g in sorted(exp) if exp[g].shape[0] == 1 and exp[g].view("<i4")[0, 2] & M.HASCOORD and g > 7)
    two = next(exp[g] for g in sorted(exp) if exp[g].shape[0] == 2 and g > 7)
    busy = next(exp[g] for g in sorted(exp) if exp[g].shape[0] == 1 and
                (exp[g].view("<i4")[0, 30 + 3:30 + 32:4] & 0x100).any())     # a commit waiting (K 3, W 8: acc_ring at 30)

    def mod(src, row, word, value=None, xor=None):
        r = src.copy()
        v = r.view("<i4")
        v[row, word] = value if xor is None else v[row, word] ^ xor
        return r
    out = [("wrong format", mod(one, 0, 0, 2)), ("wrong kind", mod(one, 0, 1, 3)), ("window", mod(one, 0, 4, 3 | (16 << 16))),
           ("kmax", mod(one, 0, 4, 4 | (8 << 16))), ("my_id", mod(one, 0, 3, 101)), ("k = 0", mod(one, 0, 2, xor=3 << 8)),
           ("k > kmax", mod(one, 0, 2, xor=7 << 8)), ("unknown flag bit", mod(one, 0, 2, xor=32)),
           ("unknown high flag bit", mod(one, 0, 2, xor=1 << 20)), ("reserved word", mod(one, 0, 15, 1)),
           ("not alive", mod(one, 0, 2, xor=1)), ("continued, next row is a main row", mod(one, 0, 2, xor=8 | 16)),
           ("continuation row alone", two[1:2]), ("continuation of another group", mod(two, 1, 5, xor=1)),
           ("continuation with a bad format", mod(two, 1, 0, 7)), ("continuation with a header word", mod(two, 1, 9, 1))]
    accd = next(exp[g] for g in sorted(exp) if exp[g].shape[0] == 1 and g > 7 and
                (exp[g].view("<i4")[0, 30 + 3:30 + 32:4] & 1).any())         # an accepted slot
    x_com = int(np.nonzero(busy.view("<i4")[0, 30:62].reshape(8, 4)[:, 3] & 0x100)[0][0])
    out.append(("committed slot at the wrong index", mod(busy, 0, 62 + 4 * x_com, xor=1)))
    x_acc = int(np.nonzero(accd.view("<i4")[0, 30:62].reshape(8, 4)[:, 3] & 1)[0][0])
    out.append(("accepted slot at the wrong index", mod(accd, 0, 30 + 4 * x_acc, xor=2)))
    co = two.view("<i4")[1, 16:48].reshape(8, 4)
    x_co = int(np.nonzero(co[:, 3] & 0x100)[0][0])
    out.append(("carried-over slot at the wrong index", mod(two, 1, 16 + 4 * x_co, xor=4)))
    # c_pcount: other calls use it as a bound (one output plane per pre-active proposal).  K 3, W 8: p_ring at 22
    prop = next(exp[g] for g in sorted(exp) if exp[g].shape[0] == 1 and g > 7 and exp[g].view("<i4")[0, 14] >= 2)
    pv = prop.view("<i4")[0]
    pc, p_in = int(pv[14]), np.nonzero(pv[22:30] & M.P_PRESENT)[0]
    p_out = np.nonzero(pv[22:30] == 0)[0]
    assert pc == p_in.size and p_out.size
    tv = two.view("<i4")
    nx, tpc = int(tv[0, 13]), int(tv[0, 14])
    assert tpc == 2 and int((tv[0, 22:30] & M.P_PRESENT != 0).sum()) == 2
    moved = two.copy()                                       # the older proposal one slot further back: a gap
    mv = moved.view("<i4")
    mv[0, 22 + ((nx - 3) & 7)], mv[0, 22 + ((nx - 2) & 7)] = mv[0, 22 + ((nx - 2) & 7)], 0
    for i in (0, 1):                                         # ... its handle with it (K 3, W 8: p_handle at 64)
        mv[1, 64 + 2 * ((nx - 3) & 7) + i], mv[1, 64 + 2 * ((nx - 2) & 7) + i] = mv[1, 64 + 2 * ((nx - 2) & 7) + i], 0
    out += [("c_pcount far beyond the window", mod(prop, 0, 14, 100000)), ("c_pcount negative", mod(prop, 0, 14, -1)),
            ("c_pcount above the proposals", mod(prop, 0, 14, pc + 1)), ("c_pcount below the proposals", mod(prop, 0, 14, pc - 1)),
            ("coordinator words without a coordinator", mod(one, 0, 2, xor=M.HASCOORD)),
            ("preparing, c_pcount window + 1", mod(two, 0, 14, 9)), ("preparing, c_pcount above the proposals", mod(two, 0, 14, 3)),
            ("preparing, proposals with a gap", moved)]
    # words that are not canonical
    a_out = int(np.nonzero(accd.view("<i4")[0, 30:62].reshape(8, 4)[:, 3] & 1 == 0)[0][0])
    c_out = int(np.nonzero(busy.view("<i4")[0, 30:62].reshape(8, 4)[:, 3] & 0x100 == 0)[0][0])
    co_out = int(np.nonzero(co[:, 3] & 0x100 == 0)[0][0])
    tp_out = int(np.nonzero(tv[0, 22:30] & M.P_PRESENT == 0)[0][0])
    out += [("p_ring: unknown bit", mod(prop, 0, 22 + int(p_in[0]), xor=1 << 18)),
            ("p_ring: word under a clear present bit", mod(prop, 0, 22 + int(p_out[0]), 5)),
            ("accepted entry: unknown flag bit", mod(accd, 0, 30 + 4 * x_acc + 3, xor=0x80)),
            ("accepted entry: word under a clear present bit", mod(accd, 0, 30 + 4 * a_out + 1, 7)),
            ("committed entry: word under a clear present bit", mod(busy, 0, 62 + 4 * c_out + 3, 1)),
            ("carried-over entry: unknown flag bit", mod(two, 1, 16 + 4 * x_co + 3, xor=0x200)),
            ("co_handle without its entry", mod(two, 1, 48 + 2 * co_out, 1)),
            ("p_handle without its proposal", mod(two, 1, 64 + 2 * tp_out + 1, 1)),
            ("member at or beyond k", mod(one, 0, 2, xor=1 << 8))]
    return out


def test_import_status_matrix(world, hip_lib):
    exp, n = world["expected"], world["n"]
    stride = image.image_stride(3, 8)
    e = IC.engine(hip_lib, n)
    good = [g for g in sorted(exp) if g > 300][:40]
    assert any(exp[g].shape[0] == 2 for g in good)
    base = all_rows(exp, range(8))                                           # groups 0 .. 7 live here already
    assert (image.import_groups(e, base, None, image.IMG_VIEWCHANGE) == S_OK).all()
    bad = bad_rows(exp, stride)
    pieces, want, gcol = [], [], []
    for i, g in enumerate(good):                                             # a bad one between every two good ones
        pieces.append(exp[g])
        want += [S_OK] * exp[g].shape[0]
        gcol += [g] + [-7] * (exp[g].shape[0] - 1)
        if i < len(bad):
            what, r = bad[i]
            pieces.append(r)
            want += [S_IMAGE] * r.shape[0]
            gcol += [100 + i] * r.shape[0]
    for what, dst, st in (("alive destination", 3, S_EXISTS), ("out of range", n, S_NOGROUP), ("negative", -1, S_NOGROUP)):
        pieces.append(exp[good[0]][:1] if exp[good[0]].shape[0] == 1 else exp[good[1]][:1])
        want.append(st)
        gcol.append(dst)
    last = next(exp[g] for g in good if exp[g].shape[0] == 2)[:1].copy()   # continued, and no row follows
    pieces.append(last)
    want.append(S_IMAGE)
    gcol.append(250)
    rows = np.concatenate(pieces)
    d0 = [e.dump(g).tolist() for g in range(n)]
    x0 = export_host(e, None, n, 0, 2 * n)[0]
    st_bad = image.import_groups(e, np.concatenate([r for _, r in bad] + [last]), None, image.IMG_VIEWCHANGE)
    assert (st_bad == S_IMAGE).all(), [w for (w, r), s in zip(bad, st_bad) if s != S_IMAGE]
    assert [e.dump(g).tolist() for g in range(n)] == d0                     # a refused group changes nothing
    assert export_host(e, None, n, 0, 2 * n)[0].tobytes() == x0.tobytes()
    import torch

    for form in ("host", "dev"):
        e2 = IC.engine(hip_lib, n)
        assert (image.import_groups(e2, base, None, image.IMG_VIEWCHANGE) == S_OK).all()
        base_d = [e2.dump(g).tolist() for g in range(8)]
        base_x = export_host(e2, None, 8, 0, 16)
        assert base_x[1].as_tuple()[2] == sum(1 for g in range(8) if g in exp) and 3 in exp
        if form == "host":
            st = image.import_groups(e2, rows, np.array(gcol, np.int32), 0)
        else:
            tr, tg = torch.from_numpy(rows.copy()).cuda(), torch.from_numpy(np.array(gcol, np.int32)).cuda()
            ts = torch.full((rows.shape[0] + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            image.import_groups_dev(e2, rows.shape[0], tr.data_ptr(), tg.data_ptr(), 0, ts.data_ptr())
            e2.sync()
            st = ts.cpu().numpy()
            assert untouched(st[rows.shape[0]:])
            st = st[:rows.shape[0]]
        names = [w for w, r in bad for _ in range(r.shape[0])]
        assert st.tolist() == want, (form, [(i, int(s), int(t)) for i, (s, t) in enumerate(zip(st, want)) if s != t], names)
        for g in good:
            assert e2.dump(g).tolist() == world["eo"].dump(g).tolist(), g
        # the alive destination (group 3, GPX_S_EXISTS) and its neighbours are what they were, dump and image
        assert [e2.dump(g).tolist() for g in range(8)] == base_d == [world["eo"].dump(g).tolist() for g in range(8)]
        after_x = export_host(e2, None, 8, 0, 16)
        assert after_x[1].as_tuple() == base_x[1].as_tuple() and after_x[0].tobytes() == base_x[0].tobytes()
        for g in range(8, n):
            if g not in good:
                assert e2.dump(g).tolist() == [0], g
        e2.close()
    e.close()


def test_import_of_garbage_and_over_a_dirty_row(world, hip_lib, oracle_lib):
    exp, n, eo = world["expected"], world["n"], world["eo"]
    stride = image.image_stride(3, 8)
    rng = np.random.default_rng(17)
    e = IC.engine(hip_lib, n)
    junk = rng.integers(0, 256, (600, stride), dtype=np.uint8)
    assert (image.import_groups(e, junk, None, image.IMG_VIEWCHANGE) == S_IMAGE).all()
    # rows that look right up to the ring words: headers of real rows, everything behind them random
    live = [g for g in sorted(exp)][:200]
    half = all_rows(exp, live).copy()
    half[:, 64:] = rng.integers(0, 256, (half.shape[0], stride - 64), dtype=np.uint8)
    st = image.import_groups(e, half, None, image.IMG_VIEWCHANGE)
    assert set(st.tolist()) <= {S_OK, S_IMAGE} and (st == S_IMAGE).sum() > 100
    for g in range(n):
        d = e.dump(g)                                                        # whatever was taken can be read back
        assert d[0] in (0, 1)
    e.close()
    # a busy group is killed; another group's image over its dirty row gives the imported state only
    w = build(hip_lib, oracle_lib, 64)
    busy = [g for g in range(64) if g in w["expected"]]
    w["eh"].retire_groups(np.array(busy, np.int32), RETIRE_KILL)
    src = [g for g in sorted(exp) if g >= 128][:len(busy)]
    rows = all_rows(exp, src)
    dest = dict(zip(src, busy))
    assert (image.import_groups(w["eh"], rows, row_gidx(rows, dest), image.IMG_VIEWCHANGE) == S_OK).all()
    for g in src:
        assert w["eh"].dump(dest[g]).tolist() == eo.dump(g).tolist(), g
    w["eh"].close()
    w["eo"].close()


def test_import_into_130561_groups(world, hip_lib):
    """the image does not depend on bucket geometry: rows from the small table into a large one"""
    exp, eo = world["expected"], world["eo"]
    n2 = 130561
    e = IC.engine(hip_lib, n2)
    live = np.array(sorted(exp), np.int32)
    rows = all_rows(exp, live)
    dest = dict(zip(live.tolist(), (n2 - 1 - np.arange(live.size) * 169).tolist()))
    assert (image.import_groups(e, rows, row_gidx(rows, dest), image.IMG_VIEWCHANGE) == S_OK).all()
    for g in live:
        assert e.dump(dest[int(g)]).tolist() == eo.dump(int(g)).tolist(), g
    order = sorted(live.tolist(), key=lambda g: dest[g])
    want = all_rows(exp, order).copy()
    wv = want.view("<i4")
    wv[:, 5] = [dest[int(x)] for x in wv[:, 5]]
    out, counts = export_dev(e, None, n2, 0, rows.shape[0])
    assert counts.as_tuple() == (live.size, rows.shape[0], live.size, rows.shape[0])
    assert out[:want.shape[0]].tobytes() == want.tobytes() and untouched(out[want.shape[0]:])
    e.close()


# 4 ---- the protocol goes on ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmax,k,window", [(3, 3, 8), (3, 3, 4), (3, 3, 64), (16, 16, 8), (3, 1, 8)])
def test_the_protocol_goes_on_after_moves(hip_lib, oracle_lib, kmax, k, window):
    n = T + 65
    w = build(hip_lib, oracle_lib, n, kmax, k, window, edges=[0, 63, 64, 255, 256])
    a, eo, exp = w["eh"], w["eo"], w["expected"]
    nb = n + 11
    b = IC.engine(hip_lib, nb, kmax, window)
    IC.create(b, np.array([nb - 1 - 6], np.int32), kmax, k)                   # one destination is taken
    where = {g: (0, g) for g in range(n)}
    taken = np.array([nb - 1 - 6], np.int32)
    taken_d, taken_x = b.dump(nb - 1 - 6).tolist(), export_host(b, taken, 1, 0, 2)
    assert taken_d[0] == 1 and taken_x[1].as_tuple() == (1, 1, 1, 1)
    out_g = np.arange(0, n, 2, dtype=np.int32)                               # half of them, dead ones among them
    st = image.move_groups(a, b, out_g, nb - 1 - out_g)
    # the refused move (GPX_S_EXISTS) left the occupant of that row as it was, dump and image
    assert b.dump(nb - 1 - 6).tolist() == taken_d
    again = export_host(b, taken, 1, 0, 2)
    assert again[1].as_tuple() == (1, 1, 1, 1) and again[0].tobytes() == taken_x[0].tobytes()
    for g, s in zip(out_g.tolist(), st.tolist()):
        assert s == (S_NOGROUP if g not in exp else S_EXISTS if g == 6 else S_OK), (g, s)
        if s == S_OK:
            where[g] = (1, nb - 1 - g)
    assert a.dump(6).tolist() == eo.dump(6).tolist()                         # refused over there: back in its row
    st_a = a.snapshot(np.arange(n, dtype=np.int32))[1]
    assert all((st_a[g] == S_OK) == (where[g][0] == 0 and g in exp) for g in range(n))
    back_g = np.array([g for g in range(0, n - 2, 4) if where[g][0] == 1 and g != 4], np.int32)   # some back, into other rows
    st = image.move_groups(b, a, np.array([where[int(g)][1] for g in back_g], np.int32), back_g + 2)
    assert (st == S_OK).all()
    for g in back_g.tolist():
        where[g] = (0, g + 2)
    assert len({v for g, v in where.items() if g in exp}) == len(exp)
    assert IC.all_dumps(where, [a, b], n, w["dead"]) == IC.all_dumps({g: (0, g) for g in range(n)}, [eo], n, w["dead"])
    split = np.array([where[g][0] for g in range(n)])
    log_h = IC.second_half(where, [a, b], n, w["cat"], k, w["ctx"], w["dead"], split)
    log_o = IC.second_half({g: (0, g) for g in range(n)}, [eo], n, w["cat"], k, w["ctx"], w["dead"], split)
    assert len(log_h) == len(log_o) > 10
    for i, (x, y) in enumerate(zip(log_h, log_o)):
        assert x == y, (i, x[0])
    assert IC.all_dumps(where, [a, b], n, w["dead"]) == IC.all_dumps({g: (0, g) for g in range(n)}, [eo], n, w["dead"])
    for e in (a, b, eo):
        e.close()


# 5 ---- the host twin -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("memory", ["pageable", "registered", "host_alloc"])
def test_host_twin_from_every_kind_of_memory(world, hip_lib, memory):
    from gigapaxos_amd import Engine

    eh, exp, n = world["eh"], world["expected"], world["n"]
    stride = image.image_stride(3, 8)
    want, counts = expect_export(exp, np.arange(n), 2 * n)
    nbytes = (counts[1] + PAD) * stride
    if memory == "pageable":
        buf = np.empty(nbytes, np.uint8)
    elif memory == "registered":
        buf = Engine.page_array(nbytes, np.uint8)
        eh.host_register(buf)
    else:
        buf = eh.host_alloc(nbytes, np.uint8)
    buf[:] = SENTINEL
    rows, got = image.export_groups(eh, None, 0, cap=counts[1], out=buf)
    assert got.as_tuple() == counts and rows.tobytes() == want.tobytes() and untouched(buf[counts[1] * stride:])
    e2 = IC.engine(hip_lib, n)
    buf[:want.size] = want.reshape(-1)
    st = image.import_groups(e2, buf[:want.size], None, image.IMG_VIEWCHANGE)
    assert (st == S_OK).all()
    for g in range(n):
        assert e2.dump(g).tolist() == world["eo"].dump(g).tolist(), g
    e2.close()
    if memory == "registered":
        eh.host_unregister(buf)
    elif memory == "host_alloc":
        eh.host_free(buf)
    del buf


def test_host_twin_in_chunks_equals_one_call(world, hip_lib, monkeypatch):
    """GPX_TEST_IMAGE_STAGE (read at engine creation) bounds the staging at five rows: 2 entries per export chunk, 5 rows
    per import chunk, so chunk boundaries fall between, before and behind two-row groups"""
    exp, n, eo = world["expected"], world["n"], world["eo"]
    stride = image.image_stride(3, 8)
    live = np.array(sorted(exp), np.int32)
    rows = all_rows(exp, live)
    monkeypatch.setenv("GPX_TEST_IMAGE_STAGE", "1")
    with pytest.raises(Exception):
        IC.engine(hip_lib, 16)                                              # the library reads the name: a bad value is refused
    monkeypatch.setenv("GPX_TEST_IMAGE_STAGE", str(5 * stride))
    e = IC.engine(hip_lib, n)
    monkeypatch.delenv("GPX_TEST_IMAGE_STAGE")
    st = image.import_groups(e, rows, None, image.IMG_VIEWCHANGE)
    assert (st == S_OK).all()
    for g in range(n):
        assert e.dump(g).tolist() == eo.dump(g).tolist(), g
    for name, gidx in lists().items():
        m = n if gidx is None else len(gidx)
        check_export(e, exp, "host", gidx, m, 0, 2 * m, what="chunked " + name)
    check_export(e, exp, "host", None, n, 0, 0, null=True, what="chunked, counts only")
    for edge in (63, 64, T):
        before = sum(exp[g].shape[0] for g in range(edge) if g in exp)
        check_export(e, exp, "host", None, n, 0, before + 1, what=f"chunked, cut inside group {edge}")
    # a refused pair at a chunk boundary, among good rows: the same statuses as from one call
    e3 = IC.engine(hip_lib, n)
    mixed = rows.copy()
    v = mixed.view("<i4")
    conts = np.nonzero(v[:, 1] == M.CONT)[0]
    v[conts[::3], 5] ^= 1                                                   # every third continuation names another group
    st3 = image.import_groups(e3, mixed, None, image.IMG_VIEWCHANGE)        # five rows per chunk
    monkeypatch.setenv("GPX_TEST_IMAGE_STAGE", str(1 << 26))
    e5 = IC.engine(hip_lib, n)
    monkeypatch.delenv("GPX_TEST_IMAGE_STAGE")
    st5 = image.import_groups(e5, mixed, None, image.IMG_VIEWCHANGE)        # one chunk
    assert st3.tolist() == st5.tolist() and (st5 == S_IMAGE).sum() == 2 * conts[::3].size
    for x in (e, e3, e5):
        x.close()
