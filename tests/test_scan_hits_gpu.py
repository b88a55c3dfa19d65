"""The hit-compacting scans (include/gpx_scan.h) on the GPU.  Every case applies one history to a HIP engine and to the
CPU oracle (tests/scan_hits_common.py); the expected answer is tests/scan_hits_model.py applied to the ORACLE's dense
scan.  Hits are placed by construction: on the edges of waves, of workgroup passes and of GPX_SCAN_TILE, in whole tiles
around an empty one, sparsely, everywhere and nowhere; the table ends in a partial tile."""
import numpy as np
import pytest

from gigapaxos_amd import scan
from tests import scan_hits_common as SC
from tests import scan_hits_model as M

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
PAD = 9                                   # entries behind cap that no call may touch
DENSE_KERNELS = ("k_election_scan", "k_poke_scan", "k_gap_scan")


def filled(count, dtype):
    return np.frombuffer(bytes([SENTINEL]) * (count * np.dtype(dtype).itemsize), dtype).copy()


def untouched(a):
    return (np.asarray(a).view(np.uint8) == SENTINEL).all()


def call_host(kind, eh, gidx, n, cap, params, null_cols=False):
    """The host twin into sentinel-filled arrays of cap + PAD entries -> (whole arrays, ScanCounts)"""
    out = None if null_cols else [filled(cap + PAD, dt) for dt in M.DTYPES[kind]]
    fn = {"election": scan.election_scan_hits, "poke": scan.poke_scan_hits, "gap": scan.gap_scan_hits}[kind]
    cols, counts = fn(eh, gidx, cap=cap, n=n, out=out, **params)
    if out is not None:
        for c, a in zip(cols, out):
            assert c.shape[0] == max(0, min(counts.n_hits, cap)) and c.ctypes.data == a.ctypes.data
    return out, counts


def call_dev(kind, eh, gidx, n, cap, params, null_cols=False):
    """The _dev form into sentinel-filled device buffers -> (whole arrays, ScanCounts), after one engine sync"""
    import torch

    bufs = [] if null_cols else [torch.full(((cap + PAD) * np.dtype(dt).itemsize,), SENTINEL, dtype=torch.uint8, device="cuda")
                                 for dt in M.DTYPES[kind]]
    cnt = torch.full((16 + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    g = None if gidx is None else torch.from_numpy(np.ascontiguousarray(gidx, np.int32)).cuda()
    torch.cuda.synchronize()
    ptrs = [b.data_ptr() for b in bufs] if bufs else [0] * len(M.DTYPES[kind])
    gp = 0 if g is None else g.data_ptr()
    if kind == "election":
        scan.election_scan_hits_dev(eh, n, gp, params.get("down_nodes", ()), params.get("long_dead_nodes", ()),
                                    params.get("force", False), cap, ptrs, cnt.data_ptr())
    elif kind == "poke":
        scan.poke_scan_hits_dev(eh, n, gp, cap, ptrs, cnt.data_ptr())
    else:
        scan.gap_scan_hits_dev(eh, n, gp, params["threshold"], params["sync_mode"], params["size_limit"],
                               params["require"], cap, ptrs, cnt.data_ptr())
    eh.sync()
    raw = cnt.cpu().numpy()
    assert untouched(raw[16:])
    counts = scan.ScanCounts.from_buffer_copy(raw[:16].tobytes())
    out = None if null_cols else [b.cpu().numpy().view(dt) for b, dt in zip(bufs, M.DTYPES[kind])]
    return out, counts


def dense_of(kind, eo, gidx, n, params):
    if kind == "election":
        return SC.election_dense(eo, gidx, n, params.get("force", False), params.get("down_nodes", ()),
                                 params.get("long_dead_nodes", ()))
    if kind == "poke":
        return SC.poke_dense(eo, gidx, n)
    return SC.gap_dense(eo, gidx, n, (params["threshold"], params["sync_mode"], params["size_limit"]))


def check(kind, eh, eo, gidx, n, cap, params, forms=("host", "dev"), null_cols=False, what=""):
    """Both forms against the model over the oracle's dense scan: columns, counts, and the sentinel from the last
    written entry on.  Returns the expected (columns, n_hits, n_nogroup)."""
    groups = np.arange(n, dtype=np.int32) if gidx is None else gidx
    want, n_hits, n_nog = M.compact(kind, dense_of(kind, eo, gidx, n, params), groups, cap, params.get("require", 0))
    k = max(0, min(n_hits, cap))
    for form in forms:
        out, counts = (call_host if form == "host" else call_dev)(kind, eh, gidx, n, cap, params, null_cols)
        tag = f"{kind} {what} {form} cap={cap}"
        assert (counts.n_hits, counts.n_nogroup, counts.reserved[0], counts.reserved[1]) == (n_hits, n_nog, 0, 0), tag
        if out is not None:
            SC.same([a[:k] for a in out], want, tag)
            assert all(untouched(a[k:]) for a in out), f"{tag}: written at or beyond entry {k}"
    return want, n_hits, n_nog


def params_of(kind):
    if kind == "election":
        return [dict(down_nodes=SC.ELECTION_DOWN), dict(down_nodes=SC.ELECTION_DOWN, force=True)]
    if kind == "poke":
        return [dict()]
    return [dict(threshold=t, sync_mode=m, size_limit=lim, require=r) for t, m, lim in SC.GAP_SETTINGS
            for r in SC.GAP_REQUIRES]


def build(kind, lib, hits, **kw):
    if kind == "election":
        return SC.election_engine(lib, hits, mine=4, **kw)
    if kind == "poke":
        return SC.poke_engine(lib, hits, **kw)
    return SC.gap_engine(lib, hits, **kw)[0]


@pytest.fixture(scope="module")
def pairs(hip_lib, oracle_lib):
    """(HIP engine, oracle engine) per (scan, hit set), built on first use and shared by the cases of this file"""
    made = {}

    def get(kind, name):
        if (kind, name) not in made:
            hits = SC.hit_set(name)
            made[(kind, name)] = (build(kind, hip_lib, hits), build(kind, oracle_lib, hits))
        return made[(kind, name)]
    yield get
    for eh, eo in made.values():
        eh.close()
        eo.close()


# 1 ---- the whole table -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.SET_NAMES)
@pytest.mark.parametrize("kind", ["election", "poke", "gap"])
def test_whole_table_both_forms(pairs, kind, name):
    eh, eo = pairs(kind, name)
    eh.profile(2)
    seen = set()
    for p in params_of(kind):
        _, n_hits, _ = check(kind, eh, eo, None, SC.G, SC.G, p, what=f"{name} {p}")
        seen.add(n_hits)
    prof = eh.profile_read()
    eh.profile(0)
    assert prof[f"k_scan_{kind}_tile"][0] == 2 * len(params_of(kind)) == prof["k_scan_offsets"][0]
    assert prof[f"k_scan_{kind}_move"][0] == 2 * len(params_of(kind))
    assert not any(k in prof for k in DENSE_KERNELS), sorted(prof)
    if kind != "gap":
        assert SC.hit_set(name).size in seen
    # gidx == NULL with n == max_groups: the spare groups at the end count as n_nogroup
    p = params_of(kind)[-1]
    _, _, n_nog = check(kind, eh, eo, None, SC.G + SC.SPARE, SC.G + SC.SPARE, p, what=f"{name} whole table")
    assert n_nog == SC.SPARE


def test_host_twin_into_host_alloc_memory(pairs):
    """The same call with its outputs in gpx_host_alloc blocks (one DMA per column instead of staged pieces)"""
    eh, eo = pairs("poke", "sparse")
    out = [eh.host_alloc(SC.G + PAD, dt) for dt in M.DTYPES["poke"]]
    for a in out:
        a.view(np.uint8)[...] = SENTINEL
    cols, counts = scan.poke_scan_hits(eh, None, n=SC.G, out=out)
    want, n_hits, _ = M.compact("poke", SC.poke_dense(eo, None, SC.G), np.arange(SC.G), SC.G)
    assert counts.n_hits == n_hits == SC.hit_set("sparse").size
    SC.same(cols, want, "host_alloc outputs")
    assert all(untouched(a[n_hits:]) for a in out)
    del cols
    eh.host_free(*out)


# 2 ---- a listed scan ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["election", "poke", "gap"])
def test_listed_scan(pairs, kind):
    eh, eo = pairs(kind, "hole")
    lst = SC.listed()
    for p in params_of(kind)[:3]:
        want, n_hits, n_nog = check(kind, eh, eo, lst, lst.shape[0], lst.shape[0], p, what="listed")
        assert n_nog == 6 and n_hits > 40
        # array order, duplicates kept: the hits' groups are the listed groups that hit, in the order listed
        hit_groups = set(want[0].tolist())
        assert want[0].tolist() == [g for g in lst.tolist() if g in hit_groups]
        assert len(hit_groups) < n_hits


# 3 ---- short capacity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["election", "poke", "gap"])
def test_short_capacity(pairs, kind):
    eh, eo = pairs(kind, "sparse")
    p = params_of(kind)[0] if kind != "gap" else dict(threshold=1, sync_mode=0, size_limit=64, require=SC.GAP_HIT_AHEAD)
    _, n_hits, _ = check(kind, eh, eo, None, SC.G, SC.G, p)
    assert n_hits > 8
    for cap in (n_hits - 1, 1, 0):
        _, again, _ = check(kind, eh, eo, None, SC.G, cap, p, what="short")
        assert again == n_hits                                   # the full count, whatever was written
    check(kind, eh, eo, None, SC.G, 0, p, null_cols=True, what="counts only")
    # the scan of the 'all' set into a capacity that ends inside the second tile
    eh, eo = pairs(kind, "all")
    p = params_of(kind)[0] if kind != "gap" else dict(threshold=1, sync_mode=0, size_limit=64, require=0)
    check(kind, eh, eo, None, SC.G, SC.T + 5, p, what="short, all")


# 4 ---- nothing of an earlier call survives in the scratch ------------------------------------------------------------------
def test_one_engine_all_none_sparse_edges_then_a_small_call(hip_lib, oracle_lib):
    eh, eo = SC.election_multi_engine(hip_lib), SC.election_multi_engine(oracle_lib)
    sizes = []
    for name in ("all", "none", "sparse", "edges"):
        down, long_dead, force = SC.multi_params(name)
        p = dict(down_nodes=down, long_dead_nodes=long_dead, force=force)
        want, n_hits, _ = check("election", eh, eo, None, SC.G, SC.G, p, what=name)
        assert want[0].tolist() == SC.hit_set(name).tolist()
        sizes.append(n_hits)
    assert sizes == [SC.G, 0, SC.hit_set("sparse").size, 11]
    edges = SC.hit_set("edges")
    lst = np.array([edges[3], 5, edges[0], edges[3], SC.G + 1], np.int32)
    down, long_dead, force = SC.multi_params("edges")
    want, n_hits, n_nog = check("election", eh, eo, lst, 5, 5, dict(down_nodes=down, long_dead_nodes=long_dead), what="n=5")
    assert (n_hits, n_nog) == (3, 1) and want[0].tolist() == [edges[3], edges[0], edges[3]]
    check("election", eh, eo, None, 0, 0, dict(), null_cols=True, what="n=0")
    eh.close()
    eo.close()


# 5 ---- every k_poke_scan instantiation, both window sizes ---------------------------------------------------------------------
@pytest.mark.parametrize("kmax,k,window", [(3, 3, 64), (5, 5, 8), (5, 4, 64), (16, 9, 8), (16, 16, 64)])
def test_poke_instantiations_and_windows(hip_lib, oracle_lib, kmax, k, window):
    hits = SC.hit_set("sparse")
    eh, eo = (SC.poke_engine(lib, hits, kmax=kmax, k=k, window=window) for lib in (hip_lib, oracle_lib))
    want, n_hits, _ = check("poke", eh, eo, None, SC.G, SC.G, {})
    assert n_hits == hits.size and len(set(want[5].tolist())) > 1          # median_cp is not one value
    lst = SC.listed()
    check("poke", eh, eo, lst, lst.shape[0], lst.shape[0], {}, what="listed")
    eh.close()
    eo.close()


def test_gap_window_64(hip_lib, oracle_lib):
    hits = SC.hit_set("edges")
    eh, eo = (SC.gap_engine(lib, hits, window=64)[0] for lib in (hip_lib, oracle_lib))
    for p in params_of("gap"):
        check("gap", eh, eo, None, SC.G, SC.G, p, what=f"W=64 {p}")
    eh.close()
    eo.close()


# 6 ---- scan -> begin on the device --------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [False, True])
def test_scan_then_begin_without_a_host_round_trip(hip_lib, oracle_lib, short):
    import torch

    hits = SC.hit_set("sparse")
    eh, eo = SC.election_engine(hip_lib, hits, mine=4), SC.election_engine(oracle_lib, hits, mine=4)
    cap = hits.size - 5 if short else SC.G
    # the reference: the oracle's dense scan, the host's filter, election_begin
    run, pb, pf, st = SC.election_dense(eo, None, SC.G)
    sel = np.nonzero((st == M.S_OK) & (run != M.RUN_NO))[0][:cap].astype(np.int32)
    assert sel.size == min(hits.size, cap)
    want_status = eo.election_begin(sel, pb[sel])
    # the device: scan and begin queued back to back, one sync at the end
    i32 = lambda: torch.full((cap + PAD,), -1, dtype=torch.int32, device="cuda")  # noqa: E731
    u8 = lambda: torch.full((cap + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")  # noqa: E731
    o_g, o_b, o_f, o_r, e_st = i32(), i32(), i32(), u8(), u8()
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    scan.election_scan_hits_dev(eh, SC.G, 0, SC.ELECTION_DOWN, (), False, cap,
                                [o_g.data_ptr(), o_r.data_ptr(), o_b.data_ptr(), o_f.data_ptr()], cnt.data_ptr())
    scan.election_begin_hits_dev(eh, cap, cnt.data_ptr(), o_g.data_ptr(), o_b.data_ptr(), e_st.data_ptr())
    eh.sync()
    assert cnt.cpu().tolist() == [hits.size, 0, 0, 0]
    got = e_st.cpu().numpy()
    assert got[:sel.size].tolist() == want_status.tolist() and untouched(got[sel.size:])
    assert o_g.cpu().numpy()[:sel.size].tolist() == sel.tolist()
    for g in range(SC.G):
        assert eh.dump(g).tolist() == eo.dump(g).tolist(), g
    # ... and exactly those groups wait for PREPARE replies now
    want, n_hits, _ = check("poke", eh, eo, None, SC.G, SC.G, {}, what="after begin")
    assert n_hits == sel.size and want[0].tolist() == sel.tolist() and set(want[1].tolist()) == {2}
    eh.close()
    eo.close()


def test_capacity_limit_and_bad_arguments_on_a_live_engine(pairs):
    eh, _ = pairs("election", "edges")
    n_max = max(int(eh.cfg.max_groups), int(eh.cfg.max_batch))
    counts = scan.ScanCounts()
    import ctypes as C
    fn = eh.lib.fn
    assert fn["poke_scan_hits"](eh.h, n_max + 1, None, 0, *[None] * 8, C.byref(counts)) == -2
    assert fn["gap_scan_hits"](eh.h, n_max + 1, None, 1, 0, 64, 0, 0, *[None] * 5, C.byref(counts)) == -2
    assert fn["election_scan_hits"](eh.h, n_max + 1, None, None, 0, None, 0, 0, 0, *[None] * 4, C.byref(counts)) == -2
    assert fn["election_begin_hits_dev"](eh.h, n_max + 1, 1, 1, 1, 1) == -2
    assert fn["poke_scan_hits"](eh.h, 4, None, 4, *[None] * 8, C.byref(counts)) == -1


# 7 ---- many tiles: the offsets go past what one workgroup sums in one round ----------------------------------------------------
@pytest.mark.gpu_fast
def test_a_million_groups_sparse_then_all(hip_lib, oracle_lib):
    n = (1 << 20) + 1
    eh, eo = SC.election_multi_engine(hip_lib, n), SC.election_multi_engine(oracle_lib, n)
    for name in ("sparse", "all"):
        down, long_dead, force = SC.multi_params(name)
        p = dict(down_nodes=down, long_dead_nodes=long_dead, force=force)
        want, n_hits, _ = check("election", eh, eo, None, n, n, p, what=f"2^20 + 1 groups, {name}")
        assert n_hits == SC.hit_set(name, n).size and want[0][-1] == SC.hit_set(name, n)[-1]
    eh.close()
    eo.close()
