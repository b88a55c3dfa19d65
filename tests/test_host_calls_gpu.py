"""The host-pointer data-path calls, every transport against the oracle's synchronous calls: synchronous (the staged
one-block path up to 32,768 records, a copy per column above), asynchronous from pageable memory, asynchronous with
inputs and outputs in registered whole-page arrays (the engine writes the outputs through the mapping), and the same
arrays with GPX_ASYNC_DIRECT=0 (gpx_engine_wait fetches them).  33,001 groups: a whole-table propose / accept / commit
batch is one record above the staged path's limit, and neither 33,001 nor the 99,003 votes are a multiple of 4, so every
16-byte copy loop has a tail."""
import numpy as np
import pytest

from gigapaxos_amd import (Engine, hri_create, streams, S_OK, C_HASVALUE, ORDERED_ACCEPT, ORDERED_COMMIT)
from gigapaxos_amd._abi import GpxError
from gigapaxos_amd.packed import pack_votes
from gigapaxos_amd.packed_out import packed_out_bytes
from tests.parity_common import make_pair

pytestmark = pytest.mark.gpu

G, K, W, NODE = 33_001, 3, 8, 100
MEMBERS = [100, 101, 102]
MAX_BATCH = 3 * G + 4096
SIZES = [0, 1001, G]
TRANSPORTS = ["sync", "pageable", "registered", "registered, GPX_ASYNC_DIRECT=0"]
# (accept-reply form, proposal packed out) per round; the synchronous ABI has the six-column form alone
ASYNC_ROUNDS = [("columns", False), ("common ballot", True), ("packed", False), ("packed io", True), ("mix", False)]
SYNC_ROUNDS = [("columns", False), ("mix", False)]


def _pair(hip_lib, oracle_lib):
    eh, eo = make_pair(hip_lib, oracle_lib, NODE, G, K, W, max_batch=MAX_BATCH)
    mem = np.tile(np.array(MEMBERS, np.int32), (G, 1))
    for e in (eh, eo):
        assert (e.create_groups(np.arange(G), mem, K, hri_create(G, K, NODE)) == S_OK).all()
    return eh, eo


class _Pins:
    """The registered transport's inputs: copies in whole-page arrays of their own, registered for one round."""

    def __init__(self, eng, on):
        self.eng, self.on, self.held = eng, on, []

    def fresh(self, n, dtype):
        a = Engine.page_array(n, dtype) if self.on else np.zeros(n, dtype)
        if self.on and a.nbytes:
            self.eng.host_register(a)
            self.held.append(a)
        return a

    def __call__(self, a):
        if not self.on or a is None or a.size == 0:
            return a
        p = self.fresh(a.size, a.dtype)
        p[:] = a
        return p

    def release(self):
        self.eng.host_unregister(*self.held)
        self.held = []


def _once(pend):
    """wait(), and a second wait on the same ticket is refused"""
    res = pend.wait()
    with pytest.raises(GpxError, match="rc=-5"):
        pend.wait()
    return res


def _same_cols(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and (x == y).all(), what


def _same_runs(ra, rb, what):
    (sa, xa), (sb, xb) = ra, rb
    _same_cols(sa if isinstance(sa, tuple) else (sa,), sb if isinstance(sb, tuple) else (sb,), what)
    assert xa.as_tuple_array().shape == xb.as_tuple_array().shape and (xa.as_tuple_array() == xb.as_tuple_array()).all(), what


def _same_decisions(dh, do, what):
    a, b = dh.as_tuple_array(), do.as_tuple_array()
    assert a.shape == b.shape and (a == b).all(), what
    assert dh.status.shape == do.status.shape and (dh.status == do.status).all(), what


def _round(hip_lib, eh, eo, transport, g, r, form, packed_proposals):
    """propose -> the proposals' ACCEPTs -> their votes in `form` -> the decisions' commits, on one replica"""
    sync = transport == "sync"
    pin = transport.startswith("registered")
    P = _Pins(eh, pin)
    n = g.shape[0]
    what = f"{transport}, n = {n}, round {r} ({form})"
    # proposals
    po = eo.propose(g)
    if sync:
        ph = eh.propose(g)
    elif packed_proposals:
        t = eh.propose_packed_out_async(P(g), out=P.fresh(packed_out_bytes(n), np.uint8))
        ph = _once(t)
        assert t.packed.n == n and (n > 0 or t.packed.nbytes == 32), what
    else:
        ph = _once(eh.propose_async(P(g), pin_outputs=pin))
    _same_cols(ph, po, what + ": proposals")
    # their ACCEPTs (the acceptor side of the same engine)
    acc = (g, po[1], po[2], po[0], po[3])
    ro = eo.accept(*acc)
    rh = eh.accept(*acc) if sync else _once(eh.accept_async(*[P(c) for c in acc], pin_outputs=pin))
    _same_runs(rh, ro, what + ": accepts")
    # the votes
    if form == "mix" and n == 0:
        cols = tuple(np.zeros(0, np.int32) for _ in range(6))    # (no records to duplicate or make stale)
    else:
        cols = streams.vote_round(n, MEMBERS, r, NODE, config_id=4, mix=form == "mix", groups=g)
    do = eo.accept_reply(*cols)
    nv = cols[0].shape[0]
    if sync:
        dh = eh.accept_reply(*cols)
    elif form in ("packed", "packed io"):
        pv = pack_votes(cols, lib=hip_lib, rec_out=P.fresh(2 * max(nv, 1), np.uint32),
                        exc_out=P.fresh(8 * max(nv // 4, 1), np.int32))
        assert pv.needed <= pv.n_exc, what
        if form == "packed":
            dh = _once(eh.accept_reply_packed_async(pv, pin_outputs=pin))
        else:
            t = eh.accept_reply_packed_io_async(pv, out=P.fresh(packed_out_bytes(nv), np.uint8), status=P.fresh(nv, np.uint8))
            dh = _once(t)
            assert t.packed.n == do.gidx.shape[0] and (nv > 0 or t.packed.nbytes == 32), what
    elif form == "common ballot":
        dh = _once(eh.accept_reply_async(P(cols[0]), None, None, P(cols[3]), P(cols[4]), P(cols[5]), common_ballot=(0, NODE),
                                         pin_outputs=pin))
    else:
        dh = _once(eh.accept_reply_async(*[P(c) for c in cols], pin_outputs=pin))
    _same_decisions(dh, do, what + ": votes")
    m = do.gidx.shape[0]
    assert m == n if form != "mix" else (n == 0 or 0 < m < nv), what    # every group decides; the mixed round's count is irregular
    # the decisions' commits
    com = (do.gidx, do.bnum, do.bcoord, do.slot, do.median_cp, np.full(m, C_HASVALUE, np.uint8))
    co = eo.commit(*com)
    ch = eh.commit(*com) if sync else _once(eh.commit_async(*[P(c) for c in com], pin_outputs=pin))
    _same_runs(ch, co, what + ": commits")
    if n == 0:
        assert rh[1].gidx.shape[0] == 0 and dh.gidx.shape[0] == 0 and ch[1].gidx.shape[0] == 0, what
    P.release()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("transport", TRANSPORTS)
def test_rounds_on_every_transport_match_oracle(hip_lib, oracle_lib, monkeypatch, transport, n):
    if transport.endswith("GPX_ASYNC_DIRECT=0"):
        monkeypatch.setenv("GPX_ASYNC_DIRECT", "0")     # read at the engine's first asynchronous call
    else:
        monkeypatch.delenv("GPX_ASYNC_DIRECT", raising=False)
    eh, eo = _pair(hip_lib, oracle_lib)
    g = np.arange(n, dtype=np.int32)
    for r, (form, packed_proposals) in enumerate(SYNC_ROUNDS if transport == "sync" else ASYNC_ROUNDS):
        _round(hip_lib, eh, eo, transport, g, r, form, packed_proposals)
    every = np.arange(G, dtype=np.int32)
    assert eh.snapshot(every)[0].tobytes() == eo.snapshot(every)[0].tobytes()
    assert eh.counters() == eo.counters()
    eh.close()
    eo.close()


def test_ordered_engine_column_path_compacts_on_demand(hip_lib, oracle_lib):
    """ORDERED_ACCEPT | ORDERED_COMMIT without LAZY_OUTPUTS, synchronous calls of 33,001 records (a copy per column): the
    call asks for on-demand compaction itself.  A regular batch comes back without a compaction launch; an irregular one -
    slot 3 before slot 2 for a third of the groups, then placeholders and the ACCEPTs that release them, built as
    test_one_gpu.py's lazy-outputs test builds them - has a negative
    count on the device, the call compacts (k_one_count) and fetches the count again."""
    eh, eo = _pair(hip_lib, oracle_lib)
    for e in (eh, eo):
        e.set_ordered_batches(ORDERED_ACCEPT | ORDERED_COMMIT)
    g = np.arange(G, dtype=np.int32)
    z, bc = np.zeros(G, np.int32), np.full(G, NODE, np.int32)
    kind = np.full(G, C_HASVALUE, np.uint8)

    def both(fn, *a):
        return getattr(eh, fn)(*a), getattr(eo, fn)(*a)

    def compactions():
        return eh.profile_read().get("k_one_count", (0, 0.0))[0]
    eh.profile(2)
    _same_cols(*both("propose", g), "propose")
    _same_runs(*both("accept", g, z, bc, np.ones(G, np.int32), z), "regular accepts")
    ra, rb = both("commit", g, z, bc, np.ones(G, np.int32), z, kind)
    _same_runs(ra, rb, "regular commits")
    assert ra[1].gidx.shape[0] == G and compactions() == 0, eh.profile_read()
    sl = np.where(g % 3 == 0, 3, 2).astype(np.int32)
    ra, rb = both("commit", g, z, bc, sl, z, kind)
    _same_runs(ra, rb, "commits: slot 3 before slot 2")
    assert 0 < ra[1].gidx.shape[0] < G and compactions() == 1, eh.profile_read()
    gg = g[g % 3 == 0]                                              # the missing slot 2 (11,001 records: the staged path)
    n3 = gg.shape[0]
    _same_runs(*both("commit", gg, z[:n3], bc[:n3], np.full(n3, 2, np.int32), z[:n3], kind[:n3]), "commits: two slots execute")
    assert compactions() == 1, eh.profile_read()
    _same_runs(*both("commit", g, z, bc, np.full(G, 4, np.int32), z, np.zeros(G, np.uint8)), "placeholders")
    assert compactions() == 2, eh.profile_read()
    ra, rb = both("accept", g, z, bc, np.full(G, 4, np.int32), z)
    _same_runs(ra, rb, "accepts release placeholders")
    assert compactions() == 3, eh.profile_read()
    eh.profile(0)
    assert eh.snapshot(g)[0].tobytes() == eo.snapshot(g)[0].tobytes()
    assert eh.counters() == eo.counters()
    eh.close()
    eo.close()


def test_refused_async_call_leaves_no_registration(hip_lib):
    """Every asynchronous method with pin_outputs, refused with GPX_EBUSY: the outputs it registered for the call are
    unregistered again, so the engine's registrations are what they were; a fresh array registers and close() succeeds."""
    n = 64
    eh = Engine(hip_lib, NODE, 256, kmax=K, window=W, max_batch=1 << 12)
    mem = np.tile(np.array(MEMBERS, np.int32), (256, 1))
    assert (eh.create_groups(np.arange(256), mem, K, hri_create(256, K, NODE)) == S_OK).all()
    live = set()
    register, unregister = eh.host_register, eh.host_unregister

    def counted_register(*arrays):
        register(*arrays)
        live.update(a.ctypes.data for a in arrays)
        return arrays

    def counted_unregister(*arrays):
        unregister(*arrays)
        live.difference_update(a.ctypes.data for a in arrays)
    eh.host_register, eh.host_unregister = counted_register, counted_unregister
    g = np.arange(n, dtype=np.int32)
    z = np.zeros(n, np.int32)
    cols = streams.vote_round(n, MEMBERS, 0, NODE, groups=g)
    inflight = [eh.propose_async(g, pin_outputs=True) for _ in range(4)]     # GPX_ASYNC_DEPTH calls: every set is busy
    before, views = set(live), len(eh.live_host_views())
    assert len(before) == 4 * 5
    refused = [lambda: eh.propose_async(g, pin_outputs=True),
               lambda: eh.accept_async(g, z, z, z, z, pin_outputs=True),
               lambda: eh.accept_reply_async(*cols, pin_outputs=True),
               lambda: eh.accept_reply_packed_async(pack_votes(cols, lib=hip_lib), pin_outputs=True),
               lambda: eh.commit_async(g, z, z, z, z, pin_outputs=True)]
    for call in refused:
        with pytest.raises(GpxError, match="rc=-5"):
            call()
        assert live == before and len(eh.live_host_views()) == views
    for t in inflight:
        t.wait()
    assert not live
    fresh = Engine.page_array(n, np.int32)
    eh.host_register(fresh)
    eh.host_unregister(fresh)
    eh.close()
