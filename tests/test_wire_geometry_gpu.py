"""The wire codec and the host-row kernels at the bucket-geometry edges, engine against oracle.

gpx_wire_pack_accept_replies (k_hist -> k_scatter_ac -> k_bucket_pack_ar -> k_emit_frames) and gpx_request_batch
(the same front end -> k_bucket_reqbatch -> k_emit_dec) run one workgroup per bucket with their own loop over the
bucket's lanes; the other wire calls decide which group row a frame reaches.  Sizes: test_geometry_gpu.SIZES (4,096
buckets, shift 10, shift 11 past 4 M groups; GPX_FULL_MATRIX=1 adds the rest) and buckets wider than a workgroup under
GPX_BUCKET_SHIFT=11 / 12.  At each size the groups are created in bulk and names of mixed lengths are bound on
geometry_common.hot_set (first / last bucket, bucket boundaries, the 4 M range boundary, lanes that share a thread),
then: an ACCEPT batch and its replies packed (host form, then the one-pass device form against a restatement of its
per-call limits, a short capacity, a misaligned buffer), a request burst batched (host form against the oracle, device
form against the host form), a damaged frame burst decoded, an accept-reply round's decisions packed, and the gap,
election and coordinator scans.  Every case asserts the kernels it meant to reach."""
import numpy as np
import pytest

from gigapaxos_amd import hri_create, S_OK, GpxError
from gigapaxos_amd import wire as W
from tests.geometry_common import geometry, hot_set
from tests.parity_common import make_pair
from tests.test_geometry_gpu import SIZES
from tests.wire_common import random_frames, assert_same_decode

pytestmark = pytest.mark.gpu

MEMBERS = [100, 101, 102]
BAR_MAX_RECS, BAR_MAX_BALLOTS = 256, 4  # gpx_wire.hip.h: GPX_W_BAR_MAX_RECS / GPX_W_BAR_MAX_BALLOTS
CASES = [pytest.param(getattr(s, "values", (s,))[0], None, id=str(getattr(s, "values", (s,))[0])) for s in SIZES]
CASES += [pytest.param(3000, 11, id="wide-s11", marks=pytest.mark.gpu_fast), pytest.param(9000, 12, id="wide-s12")]
WANT_KERNELS = {"k_hist", "k_scatter_ac", "k_bucket_pack_ar", "k_emit_frames", "k_bucket_reqbatch", "k_emit_dec",
                "k_wire_decode1", "k_pack_scan", "k_pack_write", "k_gap_scan", "k_election_scan",
                "k_names_coordinator"}


@pytest.fixture(autouse=True)
def _default_paths(monkeypatch):
    for v in ("GPX_AR_TILES", "GPX_TRY_RUNS", "GPX_SAR_MAX_N", "GPX_BUCKET_SHIFT", "GPX_TILE_T", "GPX_TILE_NT",
              "GPX_WD_TILE"):
        monkeypatch.delenv(v, raising=False)


def hot_name(g):
    """A paxosID of 1 - 127 bytes: the decimal row, then bytes >= 0x80 (so no name is a prefix of another's digits)."""
    base = b"%d" % g
    pad = (g * 37) % (128 - len(base))
    return base + bytes([0x80 + g % 100]) * pad


def first_pass(g, status, sender, r_bnum, r_bcoord, slot, named, name_len):
    """gpx_wire_pack_accept_replies_dev's one pass, restated from k_bucket_pack_ar: per group, its records in array
    order; a reply is packed when it exists, its group is named and alive, its sender is its ballot's coordinator,
    it is among the group's first 256 records and its ballot among the first 4 packed ones; 2 = coalescable but over
    one of those limits.  Returns (unbatched, frames, bytes)."""
    n = g.shape[0]
    ub = np.zeros(n, np.uint8)
    frames = nbytes = 0
    order = np.argsort(g, kind="stable")
    bounds = np.flatnonzero(np.diff(g[order])) + 1
    for idx in np.split(order, bounds):
        gg = int(g[idx[0]])
        if not 0 <= gg < named.shape[0]:
            continue
        bal = {}
        for t, i in enumerate(idx):
            has = status[i] == S_OK
            coal = has and named[gg] and sender[i] == r_bcoord[i]
            ok = coal and t < BAR_MAX_RECS
            if ok:
                key = (int(r_bnum[i]), int(r_bcoord[i]))
                if key not in bal and len(bal) < BAR_MAX_BALLOTS:
                    bal[key] = set()
                ok = key in bal
                if ok:
                    bal[key].add(int(slot[i]))
            ub[i] = 2 if coal and not ok else 1 if has and not ok else 0
        for slots in bal.values():
            frames += 1
            nbytes += (13 + int(name_len[gg]) + 29 + 4 + 12 * len(slots) + 3) & ~3
    return ub, frames, nbytes


def _setup(hip_lib, oracle_lib, G, shift, monkeypatch):
    if shift:
        monkeypatch.setenv("GPX_BUCKET_SHIFT", str(shift))
    geo = geometry(G, 3, shift)
    rng = np.random.default_rng(G + (shift or 0))
    hot, place = hot_set(G, geo, rng)
    eh, eo = make_pair(hip_lib, oracle_lib, 100, G, 3, 8, max_batch=1 << 17)
    version = np.zeros(G, np.int64)
    version[hot] = np.arange(hot.shape[0]) % 3  # random_frames addresses names[i] with version i % 3
    rows = hri_create(G, 3, 100)
    rows["version"] = version
    mem = np.tile(np.array(MEMBERS, np.int32), (G, 1))
    for e in (eh, eo):
        assert (e.create_groups(np.arange(G), mem, 3, rows) == S_OK).all()
    unnamed = hot[5::17]
    named_rows = np.setdiff1d(hot, unnamed).astype(np.int32)
    wh, wo = W.WireEngine(eh), W.WireEngine(eo)
    for w in (wh, wo):
        assert (w.bind([hot_name(int(x)) for x in named_rows], named_rows) == S_OK).all()
    named = np.zeros(G, bool)
    named[named_rows] = True
    name_len = np.zeros(G, np.int32)
    name_len[named_rows] = [len(hot_name(int(x))) for x in named_rows]
    return geo, rng, hot, place, eh, eo, wh, wo, named, name_len


def _accept_batch(hot, place, G, rng):
    """An ACCEPT batch on the hot set: several slots and ballots per group, out-of-range rows, and one group in the
    last bucket with 9,000 records over 6 ballots (more than 256 replies, more than 4 reply ballots, more records
    than any bucket's LDS staging)."""
    n = 24_000
    g = rng.choice(hot, n).astype(np.int32)
    g[rng.random(n) < 0.01] = -1
    g[rng.random(n) < 0.01] = G
    big = int(place["last bucket"][-1])
    g = np.concatenate([g, np.full(9000, big, np.int32)])
    g = g[rng.permutation(g.shape[0])]
    n = g.shape[0]
    bnum = rng.choice([0, 0, 0, 1, 2, 3, 4, 5], n).astype(np.int32)
    bcoord = rng.integers(100, 105, n).astype(np.int32)
    slot = rng.integers(1, 12, n).astype(np.int32)
    median = rng.integers(0, 3, n).astype(np.int32)
    sender = np.where(rng.random(n) < 0.9, bcoord, 100).astype(np.int32)
    return g, bnum, bcoord, slot, median, sender, big


def _dev_pack(we, cols, cap, out_shift=0):
    """pack_accept_replies_dev on device columns; returns numpy copies of its outputs (buffer filled with 0xAB)."""
    import torch
    dev = torch.device("cuda:0")
    g, slot, sender, req, rb, rc, rm, st = cols
    n = g.shape[0]
    t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (g, slot, sender, req, rb, rc, rm, st)]
    ub = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    out = torch.full((cap + 4096,), 0xAB, dtype=torch.uint8, device=dev)
    foff = torch.zeros(n, dtype=torch.int64, device=dev)
    flen, fg, fd = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
    nf, nb = torch.full((1,), -5, dtype=torch.int32, device=dev), torch.full((1,), -5, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    P = lambda x: x.data_ptr()  # noqa: E731
    W.pack_accept_replies_dev(we, n, [P(x) for x in t[:7]], P(t[7]), P(ub), P(out) + out_shift, cap, P(foff), P(flen),
                              P(fg), P(fd), P(nf), P(nb))
    we.e.sync()
    torch.cuda.synchronize()
    k = int(nf.cpu()[0])
    return dict(ub=ub.cpu().numpy(), out=out.cpu().numpy(), nf=k, nb=int(nb.cpu()[0]), foff=foff.cpu().numpy()[:k],
                flen=flen.cpu().numpy()[:k], fg=fg.cpu().numpy()[:k], fd=fd.cpu().numpy()[:k])


def _request_batch_dev(we, g, est, wt, stop, max_bytes, max_size):
    import torch
    dev = torch.device("cuda:0")
    n = g.shape[0]
    t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (g, est, wt, stop)]
    leader, bc = torch.zeros(n, dtype=torch.int32, device=dev), [torch.zeros(n, dtype=torch.int32, device=dev)
                                                                 for _ in range(5)]
    st, bstop, nbt = (torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev),
                      torch.zeros(1, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    V = lambda x: W._VP(x.data_ptr())  # noqa: E731
    we.lib.check(we.lib.fn["request_batch_dev"](we.e.h, n, *[V(x) for x in t], int(max_bytes), int(max_size), V(leader),
                                                V(st), *[V(c) for c in bc], V(bstop), V(nbt)), "request_batch_dev")
    we.e.sync()
    torch.cuda.synchronize()
    k = int(nbt.cpu()[0])
    b = {nm: c[:k].cpu().numpy() for nm, c in zip(("gidx", "leader", "count", "bytes", "size"), bc)}
    b["stop"] = bstop[:k].cpu().numpy()
    return leader.cpu().numpy(), st.cpu().numpy(), b


@pytest.mark.parametrize("G,shift", CASES)
def test_wire_kernels_at_geometry_edges_vs_oracle(hip_lib, oracle_lib, monkeypatch, G, shift):
    geo, rng, hot, place, eh, eo, wh, wo, named, name_len = _setup(hip_lib, oracle_lib, G, shift, monkeypatch)
    assert geo["shift"] == (shift or geo["shift"])
    eh.profile(2)

    # an accept-reply round's decisions, packed into BATCHED_COMMIT frames (before the ACCEPT batch
    # below moves the acceptors' ballots)
    ph, po = eh.propose(hot), eo.propose(hot)
    for x, y in zip(ph, po):
        assert x.tolist() == y.tolist(), "propose"
    gi = np.repeat(hot, 3).astype(np.int32)
    nv = gi.shape[0]
    vs = [gi, np.repeat(ph[1], 3), np.repeat(ph[2], 3), np.repeat(ph[0], 3),
          np.tile(np.array(MEMBERS, np.int32), hot.shape[0]), np.zeros(nv, np.int32)]
    order = rng.permutation(nv)
    vs = [np.ascontiguousarray(c[order]) for c in vs]
    dh, do = eh.accept_reply(*vs), eo.accept_reply(*vs)
    assert (dh.as_tuple_array() == do.as_tuple_array()).all()
    (fh, gh, nbh), (fo, go, nbo) = wh.pack_commits(dh), wo.pack_commits(do)
    assert gh.tolist() == go.tolist() and nbh == nbo and fh == fo
    assert len(fh) > hot.shape[0] // 2

    # an ACCEPT batch on the hot set, then its replies packed (host form: every pass) - against the oracle
    g, bnum, bcoord, slot, median, sender, big = _accept_batch(hot, place, G, rng)
    (rh, _), (ro, _) = eh.accept(g, bnum, bcoord, slot, median), eo.accept(g, bnum, bcoord, slot, median)
    for x, y, nm in zip(rh, ro, ("r_bnum", "r_bcoord", "r_maxcp", "r_flags", "status")):
        assert x.tolist() == y.tolist(), "accept " + nm
    rb, rc, rm, _, st = rh
    req = rng.integers(-2**62, 2**62, g.shape[0])
    a = wh.pack_accept_replies(g, slot, rb, rc, rm, st, sender, req)
    b = wo.pack_accept_replies(g, slot, rb, rc, rm, st, sender, req)
    assert a[1].tolist() == b[1].tolist() and a[2].tolist() == b[2].tolist(), "frame table"
    assert a[3].tolist() == b[3].tolist(), "unbatched"
    assert a[4] == b[4] and a[0] == b[0], "bytes"
    assert eh.counters() == eo.counters()
    assert len(a[0]) > 1000

    # the one-pass device form: exactly the host form's first pass; unbatched = 2 exactly where a limit was hit
    ub, nf, nb = first_pass(g, st, sender, rb, rc, slot, named, name_len)
    assert (ub == 2).any() and (ub[g == big] == 2).any()
    cols = (g, slot, sender, req, rb, rc, rm, st)
    d = _dev_pack(wh, cols, 188 * g.shape[0])
    assert d["nf"] == nf and d["nb"] == nb, "counts in device memory"
    assert d["ub"].tolist() == ub.tolist()
    assert d["fg"].tolist() == a[1][:nf].tolist() and d["fd"].tolist() == a[2][:nf].tolist()
    assert [d["out"][o:o + n].tobytes() for o, n in zip(d["foff"], d["flen"])] == a[0][:nf]
    assert int(d["foff"][-1]) + (int(d["flen"][-1]) + 3) // 4 * 4 == nb
    assert (d["out"][nb:] == 0xAB).all()
    # one bucket short: the buckets before the last one are written, nothing at or past its start; n_bytes in full
    last_b = int(d["fg"].max()) >> geo["shift"]
    start = int(d["foff"][(d["fg"] >> geo["shift"]) == last_b].min())
    s = _dev_pack(wh, cols, nb - 1)
    assert s["nb"] == nb and s["ub"].tolist() == ub.tolist()
    assert (s["out"][:start] == d["out"][:start]).all() and (s["out"][start:] == 0xAB).all()
    with pytest.raises(GpxError, match="rc=-1 "):  # GPX_EINVAL: the output buffer is not 4-byte aligned
        _dev_pack(wh, cols, 188 * g.shape[0], out_shift=1)

    # a request burst on the hot set: a hot group with thousands of requests, weights, stops, rows out of range
    n = 20_000
    rq = rng.choice(hot, n).astype(np.int32)
    rq[rng.random(n) < 0.2] = int(place.get("shared threads", place["last bucket"])[-1])
    rq[rng.random(n) < 0.01] = -1
    rq[rng.random(n) < 0.01] = G + 3
    est = rng.integers(1, 400, n).astype(np.int32)
    wt = rng.choice([1, 1, 1, 2, 7, 300], n).astype(np.int32)
    stop = (rng.random(n) < 0.01).astype(np.uint8)
    for kw in (dict(max_bytes=2000, max_size=400), dict(max_bytes=1 << 20, max_size=2000)):
        lh, sh, bh = W.request_batch(wh, rq, est, wt, stop, **kw)
        lo, so, bo = W.request_batch(wo, rq, est, wt, stop, **kw)
        assert lh.tolist() == lo.tolist() and sh.tolist() == so.tolist(), kw
        assert {k: v.tolist() for k, v in bh.items()} == {k: v.tolist() for k, v in bo.items()}, kw
        ld, sd, bd = _request_batch_dev(wh, rq, est, wt, stop, **kw)
        assert ld.tolist() == lh.tolist() and sd.tolist() == sh.tolist(), kw
        assert {k: v.tolist() for k, v in bd.items()} == {k: v.tolist() for k, v in bh.items()}, kw

    # a damaged burst addressed to the hot set (row hot[i] has version i % 3, as random_frames writes it)
    names = [hot_name(int(x)) for x in hot]
    frames = random_frames(names, 4000, rng, 0.2)
    assert_same_decode(wh.decode(frames), wo.decode(frames), "hot-set burst")

    # the scans of the host rows over the hot set
    q = np.concatenate([hot, [-1, G]]).astype(np.int32)
    for x, y in zip(W.gap_scan(wh, q, 3), W.gap_scan(wo, q, 3)):
        assert x.tolist() == y.tolist(), "gap_scan"
    for x, y in zip(W.election_scan(wh, q, (101,), ()), W.election_scan(wo, q, (101,), ())):
        assert x.tolist() == y.tolist(), "election_scan"
    for bal in (0, 5):
        assert W.names_coordinator(wh, q, bal).tolist() == W.names_coordinator(wo, q, bal).tolist()
    assert eh.snapshot(hot)[0].tobytes() == eo.snapshot(hot)[0].tobytes()
    assert eh.counters() == eo.counters()

    ran = set(eh.profile_read())
    assert WANT_KERNELS <= ran, sorted(WANT_KERNELS - ran)
    eh.close()
    eo.close()
