"""Packed 8-byte vote records on the device (include/gpx_packed.h): k_votes_unpack against the host unpacker and the
numpy model, and the packed accept-reply calls against the oracle run on the SAME unpacked columns - by definition a
packed call is the plain call on those (decisions, per-vote status, snapshots and counters bit-identical)."""
import numpy as np
import pytest

from gigapaxos_amd import Engine, hri_create, streams, S_OK, S_NOGROUP
from gigapaxos_amd._abi import GpxError
from gigapaxos_amd.packed import PackedVotes, pack_votes, unpack_votes
from tests import packed_model as M
from tests.parity_common import make_pair
from tests.test_packed_abi import BATCHES, _hdr

pytestmark = pytest.mark.gpu


def _same(dh, do, what):
    a, b = dh.as_tuple_array(), do.as_tuple_array()
    assert a.shape == b.shape and (a == b).all(), what
    assert (dh.status == do.status).all(), what


def _pair(hip_lib, oracle_lib, G, k, extra=0):
    members = list(range(100, 100 + k))
    eh, eo = make_pair(hip_lib, oracle_lib, 100, G, k, 8, max_batch=G * k + G * k // 40 + 4096 + extra)
    mem = np.tile(np.array(members, np.int32), (G, 1))
    for e in (eh, eo):
        assert (e.create_groups(np.arange(G), mem, k, hri_create(G, k, 100)) == S_OK).all()
    return eh, eo, members


def _with(p, rec=None, n_exc=None):
    return PackedVotes(p.n, p.n_exc if n_exc is None else n_exc, p.bnum, p.bcoord, p.base_slot, p.base_cp,
                       p.base_acceptor, p.rec if rec is None else rec, p.exc)


def _unpack_on_device(torch, eh, p, offset_words=0):
    """votes_unpack_dev over device copies of p's records and rows -> six numpy columns."""
    rec = torch.zeros(2 * max(p.n, 1) + 8, dtype=torch.int32, device="cuda")
    rec[offset_words:offset_words + 2 * p.n] = torch.from_numpy(np.ascontiguousarray(p.rec).view(np.int32).reshape(-1)).cuda()
    exc = torch.from_numpy(np.ascontiguousarray(p.exc).reshape(-1)).cuda() if p.n_exc else None
    cols = [torch.full((max(p.n, 1) + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in range(6)]
    torch.cuda.synchronize()
    eh.votes_unpack_dev(p, rec.data_ptr() + 4 * offset_words, exc.data_ptr() if exc is not None else 0,
                        [c.data_ptr() for c in cols])
    eh.sync()
    out = [c.cpu().numpy() for c in cols]
    assert all((c[p.n:] == 0x5A5A5A5A).all() for c in out), "stores past n"
    return tuple(c[:p.n] for c in out)


def test_unpack_kernel_equals_host_unpack_and_model(hip_lib):
    import torch

    big = streams.vote_round(100_000, [100, 101, 102], 3, 100, mix=True)
    eh = Engine(hip_lib, 100, 64, kmax=3, window=8, max_batch=big[0].shape[0])
    rng = np.random.default_rng(11)
    cases = {name: pack_votes(cols, lib=hip_lib, exc_cap=cols[0].shape[0] // 4) for name, cols in BATCHES.items()}
    # ("own slots", and the first 3 / 4 / 5 votes of a mix round, need more than n / 4 rows: not a call the engine takes -
    # the capacity test's case; small calls with the rows they may carry follow)
    over = [name for name, p in cases.items() if p.needed > p.n_exc]
    assert over == ["own slots", "n=3", "n=4", "n=5"]
    for name in over:
        del cases[name]
    plain = streams.vote_round(3, [100, 101, 102], 1, 100)
    for n in (3, 4, 5, 7):
        cases[f"{n} votes"] = pack_votes([c[:n] for c in plain], lib=hip_lib)
    for n in (4, 5, 7):
        cases[f"{n} votes, one row"] = pack_votes(M.odd_first_batch(n), lib=hip_lib)
        assert cases[f"{n} votes, one row"].n_exc == 1
    pb = pack_votes(big, lib=hip_lib)
    for cut in range(4):                                                     # n % 4 = 0 .. 3
        n = pb.n - ((pb.n - cut) % 4)
        assert n % 4 == cut
        cases[f"300 k mix, n % 4 = {cut}"] = PackedVotes(n, pb.n_exc, pb.bnum, pb.bcoord, pb.base_slot, pb.base_cp,
                                                        pb.base_acceptor, pb.rec[:n], pb.exc)
    bad_rec, bad_idx = M.malformed(pb.rec, pb.n_exc, rng, 200)
    cases["malformed records"] = _with(pb, rec=bad_rec)
    twice = pb.rec.copy()
    e = np.nonzero(twice[:, 1] & M.EXC_BIT)[0]
    twice[e[1::2], 1] = twice[e[0:2 * len(e[1::2]):2], 1]                    # every second exception names its neighbour's row
    cases["rows named twice"] = _with(pb, rec=twice)
    for name, p in cases.items():
        host = unpack_votes(p, lib=hip_lib)
        model = M.unpack(_hdr(p), p.rec, p.exc)
        dev = _unpack_on_device(torch, eh, p)
        for k in range(6):
            assert (dev[k] == host[k]).all() and (host[k] == model[k]).all(), f"{name}: column {k}"
    got = _unpack_on_device(torch, eh, cases["malformed records"])
    assert (got[0][bad_idx] == -1).all()
    # records, rows and columns must be 16-byte aligned
    with pytest.raises(GpxError, match="rc=-1"):
        _unpack_on_device(torch, eh, pb, offset_words=2)
    eh.close()


@pytest.mark.parametrize("G,k", [(3000, 3), (300_000, 3), (100_000, 5)])
def test_packed_rounds_match_oracle(hip_lib, oracle_lib, G, k):
    """tests/test_async_gpu.py's rounds with the votes as packed records from pageable memory: four calls in flight
    (plain propose, PACKED votes, plain accept, plain commit); round 3 is the adversarial mix.  The oracle gets the
    unpacked columns through its synchronous call."""
    eh, eo, members = _pair(hip_lib, oracle_lib, G, k)
    g = np.arange(G, dtype=np.int32)
    for r in range(5):
        po = eo.propose(g)
        tp = eh.propose_async(g)
        cols = streams.vote_round(G, members, r, 100, config_id=4, mix=(r == 3))
        p = pack_votes(cols, lib=hip_lib)
        assert p.needed == p.n_exc and (p.n_exc > 0) == (r == 3)
        ucols = unpack_votes(p, lib=hip_lib)
        assert all((x == y).all() for x, y in zip(ucols, cols))
        tv = eh.accept_reply_packed_async(p)
        do = eo.accept_reply(*ucols)
        ta = eh.accept_async(g, po[1], po[2], po[0], po[3])
        tc = eh.commit_async(do.gidx, do.bnum, do.bcoord, do.slot, do.median_cp, np.full(do.gidx.shape[0], 1, np.uint8))
        with pytest.raises(GpxError):            # a fifth call, packed: GPX_EBUSY until a ticket is waited for
            eh.accept_reply_packed_async(p)
        for x, y in zip(tp.wait(), po):
            assert (x == y).all()
        _same(tv.wait(), do, f"round {r} votes")
        (ra, xa), (rb, xb) = ta.wait(), eo.accept(g, po[1], po[2], po[0], po[3])
        for x, y in zip(ra, rb):
            assert (x == y).all()
        assert (xa.as_tuple_array() == xb.as_tuple_array()).all()
        (sa, ca), (sb, cb) = tc.wait(), eo.commit(do.gidx, do.bnum, do.bcoord, do.slot, do.median_cp,
                                                   np.full(do.gidx.shape[0], 1, np.uint8))
        assert (sa == sb).all() and (ca.as_tuple_array() == cb.as_tuple_array()).all()
        with pytest.raises(GpxError):            # a ticket is good for one wait
            tv.wait()
    assert eh.snapshot(g)[0].tobytes() == eo.snapshot(g)[0].tobytes()
    assert eh.counters() == eo.counters()
    eh.close()
    eo.close()


@pytest.mark.parametrize("source", ["registered, outputs pinned", "gpx_host_alloc"])
def test_packed_pipeline_from_pinned_memory(hip_lib, oracle_lib, source):
    """A stream of (propose, packed votes) steps two deep, packed and plain vote calls alternating: records from registered
    pages with the outputs registered too (k_copy_out writes the decisions), and from gpx_host_alloc memory."""
    G, k, R = 300_000, 3, 6
    eh, eo, members = _pair(hip_lib, oracle_lib, G, k)
    g = np.arange(G, dtype=np.int32)
    pin = source.startswith("registered")
    rounds, packs, blocks = [], [], []
    for r in range(R):
        cols = streams.vote_round(G, members, r, 100, mix=(r == 3))
        rounds.append(cols)
        if r % 2 == 1 and r != 3:
            packs.append(None)                                   # a plain call between packed ones
        elif pin:
            n = cols[0].shape[0]
            rec, exc = Engine.page_array(2 * n, np.uint32), Engine.page_array(8 * (n // 4), np.int32)
            eh.host_register(rec, exc)
            blocks += [rec, exc]
            packs.append(pack_votes(cols, lib=hip_lib, rec_out=rec, exc_out=exc))
        else:
            packs.append(pack_votes(cols, engine=eh))
    pend, got = [], []
    for r in range(R):
        tp = eh.propose_async(g, pin_outputs=pin)
        tv = (eh.accept_reply_packed_async(packs[r], pin_outputs=pin) if packs[r] is not None
              else eh.accept_reply_async(*rounds[r], pin_outputs=pin))
        pend.append((tp, tv))
        if len(pend) == 2:
            tp, t = pend.pop(0)
            tp.wait()
            got.append(t.wait())
    for tp, t in pend:
        tp.wait()
        got.append(t.wait())
    if pin:
        eh.host_unregister(*blocks)
    for r in range(R):
        eo.propose(g)
        do = eo.accept_reply(*rounds[r])
        _same(got[r], do, f"round {r}")
    assert eh.snapshot(g)[0].tobytes() == eo.snapshot(g)[0].tobytes()
    assert eh.counters() == eo.counters()
    del packs
    eh.close(force=True)
    eo.close()


def test_packed_dev_call_is_the_plain_dev_call_on_the_unpacked_columns(hip_lib, oracle_lib):
    """gpx_accept_reply_packed_dev on one engine, gpx_accept_reply_batch_dev on the unpacked columns on another: the same
    outputs and state.  At 300,000 x 3 the packed call must go through the tiled front end (k_scatter_tiles: the
    engine's scratch columns are 16-byte aligned) and count as written in place."""
    import torch

    G, k = 300_000, 3
    ea, eb, members = _pair(hip_lib, hip_lib, G, k)
    g = np.arange(G, dtype=np.int32)
    P = lambda t: t.data_ptr()  # noqa: E731
    for r in range(3):
        for x, y in zip(ea.propose(g), eb.propose(g)):
            assert (x == y).all()
        cols = streams.vote_round(G, members, r, 100, mix=(r == 2))
        p = pack_votes(cols, lib=hip_lib)
        n = p.n
        rec = torch.from_numpy(p.rec.view(np.int32).reshape(-1)).cuda()
        exc = torch.from_numpy(p.exc.reshape(-1)).cuda() if p.n_exc else None
        dc = [torch.from_numpy(c).cuda() for c in unpack_votes(p, lib=hip_lib)]
        outs = []
        for _ in range(2):
            outs.append([torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(5)] +
                        [torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
                         torch.zeros(n, dtype=torch.uint8, device="cuda")])
        torch.cuda.synchronize()
        ea.profile(2)
        ea.accept_reply_packed_dev(p, P(rec), P(exc) if exc is not None else 0, *[P(t) for t in outs[0]])
        ea.sync()
        ran = ea.profile_read()
        ea.profile(0)
        eb.call_dev("accept_reply_batch", n, *[P(c) for c in dc], *[P(t) for t in outs[1]])
        eb.sync()
        assert "k_votes_unpack" in ran and "k_scatter_tiles" in ran, sorted(ran)
        if r == 0:
            assert ea.path_counters() == (1, 0) == eb.path_counters()
        m = int(outs[0][6].item())
        assert m == int(outs[1][6].item()) and m > 0
        for a, b in zip(outs[0][:6], outs[1][:6]):
            assert torch.equal(a[:m], b[:m])
        assert torch.equal(outs[0][7], outs[1][7])
    assert ea.snapshot(g)[0].tobytes() == eb.snapshot(g)[0].tobytes()
    assert ea.counters() == eb.counters() and ea.path_counters() == eb.path_counters()
    ea.close()
    eb.close()


def test_malformed_record_in_a_large_batch_and_capacity_errors(hip_lib, oracle_lib):
    """Malformed records inside a 300,000-group batch: those votes get GPX_S_NOGROUP, everything else is the oracle's
    answer on the unpacked columns.  n_exc > n / 4 and n > max_batch are refused with GPX_ECAPACITY, bad pointers with
    GPX_EINVAL, and the engine then still answers a plain call correctly."""
    G, k = 300_000, 3
    eh, eo, members = _pair(hip_lib, oracle_lib, G, k)
    g = np.arange(G, dtype=np.int32)
    rng = np.random.default_rng(3)
    for e in (eh, eo):
        e.propose(g)
    cols = streams.vote_round(G, members, 0, 100, mix=True)
    p = pack_votes(cols, lib=hip_lib)
    rec, idx = M.malformed(p.rec, p.n_exc, rng, 7)
    q = _with(p, rec=rec)
    ucols = unpack_votes(q, lib=hip_lib)
    assert (ucols[0][idx] == -1).all() and int((ucols[0] == -1).sum()) == 7
    dh, do = eh.accept_reply_packed_async(q).wait(), eo.accept_reply(*ucols)
    _same(dh, do, "malformed records")
    assert (dh.status[idx] == S_NOGROUP).all()
    assert eh.snapshot(g)[0].tobytes() == eo.snapshot(g)[0].tobytes()
    # refused whole: more exception rows than a call may carry, more votes than max_batch, missing arrays
    own = M.own_slot_batch(4000)
    po = pack_votes(own, lib=hip_lib, exc_cap=4000)
    assert po.needed == po.n_exc > 4000 // 4
    with pytest.raises(GpxError, match="rc=-2"):
        eh.accept_reply_packed_async(po)
    nbig = int(eh.cfg.max_batch) + 1
    big = PackedVotes(nbig, 0, 0, 100, 0, 0, 0, np.zeros((nbig, 2), np.uint32), np.zeros((0, 8), np.int32))
    with pytest.raises(GpxError, match="rc=-2"):
        eh.accept_reply_packed_async(big)
    import ctypes as C
    keep = [np.zeros(p.n, np.int32) for _ in range(8)]
    outs = [a.ctypes.data_as(C.c_void_p) for a in keep]
    t = C.c_uint64(0)
    for field, value in (("n_exc", -1), ("n", -1), ("rec", None), ("exc", None)):   # (exc == NULL with n_exc > 0)
        pv = p.struct()
        assert pv.n_exc > 0
        setattr(pv, field, value)
        assert hip_lib.fn["accept_reply_packed_async"](eh.h, C.byref(pv), *outs, C.byref(t)) == -1, field
    # the same batch as plain columns is taken (the caller's way out), and the next round is right
    _same(eh.accept_reply_async(*own).wait(), eo.accept_reply(*own), "plain call after the refusals")
    for e in (eh, eo):
        e.propose(g)
    cols = streams.vote_round(G, members, 1, 100)
    _same(eh.accept_reply_packed_async(pack_votes(cols, lib=hip_lib)).wait(), eo.accept_reply(*cols), "next round")
    assert eh.snapshot(g)[0].tobytes() == eo.snapshot(g)[0].tobytes()
    assert eh.counters() == eo.counters()
    eh.close()
    eo.close()
