"""Packed proposal and decision outputs on the device (include/gpx_packed_out.h): the pack kernels against the host packer
and the numpy model byte for byte, and the packed asynchronous calls against the oracle run on the same inputs - by
definition a packed output is the plain columns (decisions, proposals, per-vote status, snapshots and counters
bit-identical), and its raw bytes are what the host packer makes of the oracle's columns."""
import ctypes as C

import numpy as np
import pytest

from gigapaxos_amd import Engine, streams, S_OK
from gigapaxos_amd._abi import GpxError
from gigapaxos_amd.packed import pack_votes
from gigapaxos_amd.packed_out import PackedOut, pack_decisions, pack_proposals, packed_out_bytes
from tests import packed_out_model as M
from tests.parity_common import make_pair
from tests.test_packed_out_abi import EXPECTED, SENTINEL

pytestmark = pytest.mark.gpu
FILL = 0x5A5A5A5A


def _same(dh, do, what):
    a, b = dh.as_tuple_array(), do.as_tuple_array()
    assert a.shape == b.shape and (a == b).all(), what
    assert (dh.status == do.status).all(), what


def _dec_cols(d):
    return [d.gidx, d.slot, d.bnum, d.bcoord, d.median_cp, d.kind]


def _pair(hip_lib, oracle_lib, G, k, case=None):
    members = list(range(100, 100 + k))
    eh, eo = make_pair(hip_lib, oracle_lib, 100, G, k, 8, max_batch=G * k + G * k // 40 + 4096)
    mem = np.tile(np.array(members, np.int32), (G, 1))
    for e in (eh, eo):
        assert (e.create_groups(np.arange(G), mem, k, M.ahead_rows(case, G, k, 100)) == S_OK).all()
    return eh, eo, members


def _raw_is_host_pack(hip_lib, pend, kind, cols, what):
    """The buffer a call left == the host packer's bytes of the oracle's columns; -> its view"""
    host = (pack_decisions if kind == M.DECISIONS else pack_proposals)(cols, lib=hip_lib)
    got = pend.packed
    assert got.header() == host.header(), what
    assert got.nbytes == host.nbytes and got.raw.tobytes() == host.raw.tobytes(), what
    return got


def _pack_on_device(torch, eh, hip_lib, kind, cols, what, spare=0):
    """The _dev pack call over device copies of `cols` (columns with `spare` more entries than the call has, filled with
    garbage) into a sentinel-filled buffer; compared with the host packer and the model; -> PackedOut"""
    n = len(cols[-1])
    cap = n + spare
    dev = []
    for k, c in enumerate(cols):
        last = k == len(cols) - 1
        t = torch.full((max(cap, 1) + 16,), 0x5A if last else FILL, dtype=torch.uint8 if last else torch.int32, device="cuda")
        if n:
            t[:n] = torch.from_numpy(np.ascontiguousarray(c, np.uint8 if last else np.int32)).cuda()
        dev.append(t)
    out = torch.full((packed_out_bytes(cap) + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    n_out = torch.full((4,), n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if kind == M.DECISIONS:
        eh.decisions_pack_dev(n_out.data_ptr(), cap, [t.data_ptr() for t in dev], out.data_ptr())
    else:
        assert spare == 0
        eh.proposals_pack_dev(n, [t.data_ptr() for t in dev], out.data_ptr())
    eh.sync()
    got = out.cpu().numpy()
    host = (pack_decisions if kind == M.DECISIONS else pack_proposals)(cols, lib=hip_lib)
    model, hdr, needed = M.pack(kind, cols)
    p = PackedOut(got, lib=hip_lib)
    assert p.header() == host.header() == hdr, what
    assert p.nbytes == host.nbytes == model.shape[0], what
    assert got[:p.nbytes].tobytes() == host.raw.tobytes() == model.tobytes(), what
    assert (got[p.nbytes:] == SENTINEL).all(), f"{what}: bytes written past gpx_packed_out_size"
    return p


def test_pack_kernels_equal_host_packer_and_model(hip_lib, oracle_lib):
    import torch

    from tests.test_packed_out_abi import oracle_rounds

    eh = Engine(hip_lib, 100, 64, kmax=3, window=8, max_batch=1 << 17)
    eh.profile(2)
    for kind_name, K in (("decisions", M.DECISIONS), ("proposals", M.PROPOSALS)):
        for name, cols in M.synthetic_cases(K).items():
            p = _pack_on_device(torch, eh, hip_lib, K, cols, f"{kind_name}, {name}")
            if K == M.DECISIONS:                                 # the count on the device is below the capacity
                _pack_on_device(torch, eh, hip_lib, K, cols, f"{kind_name}, {name}, n_out < cap", spare=37)
            assert p.n == len(cols[-1])
    assert _pack_on_device(torch, eh, hip_lib, M.DECISIONS, M.steady(M.DECISIONS, 0), "n_out = 0 of 5000", spare=5000).nbytes == 32
    assert _pack_on_device(torch, eh, hip_lib, M.DECISIONS, M.steady(M.DECISIONS, 1), "n_out = 1 of 5000", spare=5000).nbytes == 64
    for case in (None, "A", "B", "C"):                           # the oracle's own outputs, every form
        for r, (po, dec, _) in enumerate(oracle_rounds(3000, 3, 2, case=case, mix_round=1)):
            p = _pack_on_device(torch, eh, hip_lib, M.PROPOSALS, po, f"case {case} round {r} proposals")
            d = _pack_on_device(torch, eh, hip_lib, M.DECISIONS, dec, f"case {case} round {r} decisions", spare=9000 - len(dec[0]))
            if case is not None and case != "C":
                assert (p.form, p.n_exc) == EXPECTED[case][0][:2]
    ran = eh.profile_read()
    eh.profile(0)
    assert ran["k_po_count"][0] == ran["k_po_write"][0] > 60, sorted(ran)
    # every device pointer must be 16-byte aligned; a capacity above max_batch is refused
    cols = M.steady(M.DECISIONS, 100)
    dev = [torch.from_numpy(np.concatenate([c, c[:28]])).cuda() for c in cols]
    out = torch.zeros(packed_out_bytes(100) + 64, dtype=torch.uint8, device="cuda")
    n_out = torch.full((4,), 100, dtype=torch.int32, device="cuda")
    ptrs = [t.data_ptr() for t in dev]
    for k in range(6):
        off = ptrs[:k] + [ptrs[k] + 4] + ptrs[k + 1:]
        with pytest.raises(GpxError, match="rc=-1"):
            eh.decisions_pack_dev(n_out.data_ptr(), 100, off, out.data_ptr())
        if k:
            with pytest.raises(GpxError, match="rc=-1"):
                eh.proposals_pack_dev(100, off[1:], out.data_ptr())
    with pytest.raises(GpxError, match="rc=-1"):
        eh.decisions_pack_dev(n_out.data_ptr(), 100, ptrs, out.data_ptr() + 8)
    with pytest.raises(GpxError, match="rc=-1"):
        eh.decisions_pack_dev(0, 100, ptrs, out.data_ptr())
    with pytest.raises(GpxError, match="rc=-2"):
        eh.proposals_pack_dev((1 << 17) + 1, ptrs[1:], out.data_ptr())
    eh.decisions_pack_dev(n_out.data_ptr(), 100, ptrs, out.data_ptr())      # ... and the call itself is taken
    eh.sync()
    assert PackedOut(out.cpu().numpy(), lib=hip_lib).n == 100
    eh.close()


def _votes(hip_lib, case, G, members, r, mix=False):
    """The round's votes and their packed form (None: the batch needs more rows than a packed call may carry)."""
    cols = M.ahead_votes(case, G, members, r, 100, mix=mix)
    p = pack_votes(cols, lib=hip_lib, exc_cap=cols[0].shape[0] // 4)
    if p.needed > p.n_exc and case != "C":
        # the votes' own reference (include/gpx_packed.h: the first vote of the majority ballot) fell on a group that is
        # ahead: put an ordinary group's vote first.  At 3,000 x 3, where the CPU tests prove the row counts, no swap is needed.
        assert (G, len(members)) != (3000, 3)
        cols = [c.copy() for c in cols]
        j = int(np.argmax(cols[0] == 0))
        for c in cols:
            c[0], c[j] = c[j], c[0]
        cols = tuple(cols)
        p = pack_votes(cols, lib=hip_lib, exc_cap=cols[0].shape[0] // 4)
    return cols, (p if p.needed == p.n_exc else None)


@pytest.mark.parametrize("case", [None, "A", "B", "C"])
@pytest.mark.parametrize("G,k", [(3000, 3), (300_000, 3), (100_000, 5)])
def test_packed_io_rounds_match_oracle(hip_lib, oracle_lib, G, k, case):
    """Whole rounds, four calls in flight: PACKED-OUT propose, PACKED-IO votes, plain accept, plain commit, from pageable
    memory.  case None: five steady rounds, round 3 the adversarial mix (no row: RECORDS at 4 and 8 bytes per entry); A, B,
    C: groups ahead of the others (tests/packed_out_model.py), two rounds - rows, the columns form, and (C) votes a
    packed call may not carry, which go in as plain columns."""
    eh, eo, members = _pair(hip_lib, oracle_lib, G, k, case)
    g = np.arange(G, dtype=np.int32)
    for r in range(5 if case is None else 2):
        po = eo.propose(g)
        tp = eh.propose_packed_out_async(g)
        cols, pv = _votes(hip_lib, case, G, members, r, mix=(case is None and r == 3))
        assert (pv is None) == (case == "C")
        tv = eh.accept_reply_packed_io_async(pv) if pv is not None else eh.accept_reply_async(*cols)
        do = eo.accept_reply(*cols)
        ta = eh.accept_async(g, po[1], po[2], po[0], po[3])
        ones = np.full(do.gidx.shape[0], 1, np.uint8)
        tc = eh.commit_async(do.gidx, do.bnum, do.bcoord, do.slot, do.median_cp, ones)
        with pytest.raises(GpxError, match="rc=-5"):          # a fifth call, packed: GPX_EBUSY until a ticket is waited for
            eh.propose_packed_out_async(g)
        if pv is not None:
            with pytest.raises(GpxError, match="rc=-5"):
                eh.accept_reply_packed_io_async(pv)
        for x, y in zip(tp.wait(), po):
            assert x.dtype == y.dtype and (x == y).all(), f"round {r} proposals"
        _same(tv.wait(), do, f"round {r} votes")
        pp = _raw_is_host_pack(hip_lib, tp, M.PROPOSALS, po, f"round {r} proposals, raw")
        assert (pp.form, pp.n_exc) == (M.rule(M.PROPOSALS, po)[0]["form"], M.rule(M.PROPOSALS, po)[0]["n_exc"])
        pd = None
        if pv is not None:
            pd = _raw_is_host_pack(hip_lib, tv, M.DECISIONS, _dec_cols(do), f"round {r} decisions, raw")
            hd = M.rule(M.DECISIONS, _dec_cols(do))[0]
            assert (pd.form, pd.n_exc, pd.n) == (hd["form"], hd["n_exc"], do.gidx.shape[0])
        if case is None:                                          # the steady state: no row, 4 and 8 bytes per entry
            assert (pp.form, pp.n_exc, pp.nbytes) == (M.RECORDS, 0, 32 + M.R(4 * G))
            assert (pd.form, pd.n_exc, pd.nbytes) == (M.RECORDS, 0, 32 + M.R(8 * pd.n))
        elif (G, k) == (3000, 3):                                 # the counts the CPU part proves of these inputs
            assert (pp.form, pp.n_exc) == EXPECTED[case][0][:2]
            assert pd is None or (pd.form, pd.n_exc) == EXPECTED[case][1][:2]
            assert pack_votes(cols, lib=hip_lib, exc_cap=9000).needed == EXPECTED[case][2]
        (ra, xa), (rb, xb) = ta.wait(), eo.accept(g, po[1], po[2], po[0], po[3])
        for x, y in zip(ra, rb):
            assert (x == y).all()
        assert (xa.as_tuple_array() == xb.as_tuple_array()).all()
        (sa, ca), (sb, cb) = tc.wait(), eo.commit(do.gidx, do.bnum, do.bcoord, do.slot, do.median_cp, ones)
        assert (sa == sb).all() and (ca.as_tuple_array() == cb.as_tuple_array()).all()
        for t in (tp, tv):
            with pytest.raises(GpxError, match="rc=-5"):      # a ticket is good for one wait
                t.wait()
    assert eh.snapshot(g)[0].tobytes() == eo.snapshot(g)[0].tobytes()
    assert eh.counters() == eo.counters()
    eh.close()
    eo.close()


@pytest.mark.parametrize("source", ["pageable", "registered", "gpx_host_alloc"])
def test_packed_io_pipeline_from_every_kind_of_memory(hip_lib, oracle_lib, source):
    """A stream of (propose, votes) steps two deep on one engine, packed-output and plain calls alternating; the buffers
    (records in, packed buffers and status out) pageable, registered whole pages, or gpx_host_alloc memory - the last two
    are written by the device through the mapping, with the length read on the device.  Round 3 is the mix round; case
    A's engine brings rows."""
    G, k, R = 300_000, 3, 6
    case = "A"
    eh, eo, members = _pair(hip_lib, oracle_lib, G, k, case)
    g = np.arange(G, dtype=np.int32)
    nv_max = G * k + G * k // 40 + 4096
    blocks = []

    def mk(n, dtype):
        if source == "pageable":
            return np.zeros(n, dtype)
        if source == "registered":
            a = Engine.page_array(n, dtype)
            eh.host_register(a)
            blocks.append(a)
            return a
        return eh.host_alloc(n, dtype)

    rounds, packs = [], []
    for r in range(R):
        cols, _ = _votes(hip_lib, case, G, members, r, mix=(r == 3))
        rounds.append(cols)
        n = cols[0].shape[0]
        packs.append(pack_votes(cols, lib=hip_lib, rec_out=mk(2 * n, np.uint32), exc_out=mk(8 * (n // 4), np.int32)))
        assert packs[-1].needed == packs[-1].n_exc > 0
    ring = [(mk(packed_out_bytes(G), np.uint8), mk(packed_out_bytes(nv_max), np.uint8), mk(nv_max, np.uint8)) for _ in range(2)]
    pend, got = [], []
    for r in range(R):
        if r % 2 == 0 or r == 3:
            o_p, o_d, st = ring[r % 2]
            o_p[:], o_d[:] = SENTINEL, SENTINEL
            n = packs[r].n
            tp = eh.propose_packed_out_async(g, out=o_p)
            tv = eh.accept_reply_packed_io_async(packs[r], out=o_d, status=st[:n])
        else:                                                    # a plain step between packed ones
            tp = eh.propose_async(g, pin_outputs=(source == "registered"))
            tv = eh.accept_reply_packed_async(packs[r], pin_outputs=(source == "registered"))
        pend.append((r, tp, tv))
        if len(pend) == 2:
            got.append(_finish(hip_lib, pend.pop(0)))
    while pend:
        got.append(_finish(hip_lib, pend.pop(0)))
    if blocks:
        eh.host_unregister(*blocks)
    for r in range(R):
        po, do = eo.propose(g), eo.accept_reply(*rounds[r])
        props, dec, raw_p, raw_d, tail = got[r]
        for x, y in zip(props, po):
            assert (x == y).all(), f"round {r} proposals"
        _same(dec, do, f"round {r}")
        if raw_p is not None:
            hp, hd = pack_proposals(po, lib=hip_lib), pack_decisions(_dec_cols(do), lib=hip_lib)
            assert raw_p == hp.raw.tobytes() and raw_d == hd.raw.tobytes(), f"round {r}: raw buffers"
            # a row for every group that is ahead; from the mix round on, a group whose coordinator was preempted there
            # answers its proposal with GPX_S_FORWARD and no slot, which fits a delta record: the model says how many
            assert hp.form == hd.form == M.RECORDS
            assert hp.n_exc == M.needed_rows(M.PROPOSALS, po) and hd.n_exc == M.needed_rows(M.DECISIONS, _dec_cols(do))
            assert G // 10 - G // 1000 <= hp.n_exc <= G // 10 and (r > 3 or hp.n_exc == G // 10) and hd.n_exc > 0
            assert tail, f"round {r}: bytes written past gpx_packed_out_size"
    assert eh.snapshot(g)[0].tobytes() == eo.snapshot(g)[0].tobytes()
    assert eh.counters() == eo.counters()
    del packs, ring, got
    eh.close(force=True)
    eo.close()


def _finish(hip_lib, item):
    """wait for a step; copies of what it left (the ring's buffers are reused two steps later)"""
    r, tp, tv = item
    props, dec = tp.wait(), tv.wait()
    if not hasattr(tp, "raw"):
        return props, dec, None, None, True
    tail = bool((tp.raw[tp.packed.nbytes:] == SENTINEL).all() and (tv.raw[tv.packed.nbytes:] == SENTINEL).all())
    dec.status = dec.status.copy()
    return props, dec, tp.packed.raw.tobytes(), tv.packed.raw.tobytes(), tail


def test_capacity_and_argument_errors(hip_lib, oracle_lib):
    """A short buffer is refused with GPX_ECAPACITY before anything is queued, null pointers and bad vote headers with
    GPX_EINVAL, a batch above max_batch with GPX_ECAPACITY; empty calls leave a header alone; an unaligned buffer inside
    gpx_host_alloc memory is filled all the same; and the engine then still answers plain and packed calls correctly."""
    G, k = 3000, 3
    eh, eo, members = _pair(hip_lib, oracle_lib, G, k)
    g = np.arange(G, dtype=np.int32)
    fn = hip_lib.fn
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    cols = streams.vote_round(G, members, 0, 100)
    pv = pack_votes(cols, lib=hip_lib)
    nv = pv.n
    t = C.c_uint64(0)
    buf = np.full(packed_out_bytes(nv) + 64, SENTINEL, np.uint8)
    st = np.zeros(nv, np.uint8)
    s = pv.struct()
    assert fn["propose_packed_out_async"](eh.h, G, ptr(g), None, ptr(buf), packed_out_bytes(G) - 1, C.byref(t)) == -2
    assert fn["accept_reply_packed_io_async"](eh.h, C.byref(s), ptr(buf), packed_out_bytes(nv) - 1, ptr(st), C.byref(t)) == -2
    assert fn["propose_packed_out_async"](eh.h, G, ptr(g), None, None, buf.nbytes, C.byref(t)) == -1
    assert fn["propose_packed_out_async"](eh.h, G, None, None, ptr(buf), buf.nbytes, C.byref(t)) == -1
    assert fn["propose_packed_out_async"](eh.h, G, ptr(g), None, ptr(buf), buf.nbytes, None) == -1
    assert fn["propose_packed_out_async"](None, G, ptr(g), None, ptr(buf), buf.nbytes, C.byref(t)) == -1
    assert fn["accept_reply_packed_io_async"](eh.h, None, ptr(buf), buf.nbytes, ptr(st), C.byref(t)) == -1
    assert fn["accept_reply_packed_io_async"](eh.h, C.byref(s), None, buf.nbytes, ptr(st), C.byref(t)) == -1
    big = int(eh.cfg.max_batch) + 1
    gb = np.zeros(big, np.int32)
    bb = np.zeros(packed_out_bytes(big), np.uint8)
    assert fn["propose_packed_out_async"](eh.h, big, ptr(gb), None, ptr(bb), bb.nbytes, C.byref(t)) == -2
    s2 = pv.struct()
    s2.n_exc = pv.n // 4 + 1
    s2.exc = s2.rec
    assert fn["accept_reply_packed_io_async"](eh.h, C.byref(s2), ptr(buf), buf.nbytes, ptr(st), C.byref(t)) == -2
    assert (buf == SENTINEL).all() and t.value == 0             # nothing was queued, nothing written
    # empty calls: a header and nothing else
    e0 = eh.propose_packed_out_async(np.zeros(0, np.int32), out=buf[:packed_out_bytes(0)])
    assert [x.shape[0] for x in e0.wait()] == [0] * 5
    assert e0.packed.header() == dict(form=M.RECORDS, kind=M.PROPOSALS, n=0, n_exc=0, bnum=0, bcoord=0, base_slot=0, base_cp=0)
    assert (buf[32:] == SENTINEL).all()
    empty = pack_votes([np.zeros(0, np.int32)] * 6, lib=hip_lib)
    e1 = eh.accept_reply_packed_io_async(empty, out=buf[:packed_out_bytes(0)])
    assert e1.wait().gidx.shape[0] == 0 and e1.packed.kind == M.DECISIONS and e1.packed.nbytes == 32
    # a round with the packed buffers at an odd offset inside gpx_host_alloc memory, no per-vote status wanted
    block = eh.host_alloc(packed_out_bytes(nv) + packed_out_bytes(G) + 64, np.uint8)
    o_p, o_d = block[4:4 + packed_out_bytes(G)], block[8 + packed_out_bytes(G):8 + packed_out_bytes(G) + packed_out_bytes(nv)]
    po = eo.propose(g)
    tp = eh.propose_packed_out_async(g, out=o_p)
    tv = eh.accept_reply_packed_io_async(pv, out=o_d, want_status=False)
    do = eo.accept_reply(*cols)
    for x, y in zip(tp.wait(), po):
        assert (x == y).all()
    dh = tv.wait()
    assert dh.status is None and (dh.as_tuple_array() == do.as_tuple_array()).all()
    _raw_is_host_pack(hip_lib, tv, M.DECISIONS, _dec_cols(do), "odd offset")
    # ... and the next round through the plain calls
    for x, y in zip(eh.propose_async(g).wait(), eo.propose(g)):
        assert (x == y).all()
    cols = streams.vote_round(G, members, 1, 100)
    _same(eh.accept_reply_async(*cols).wait(), eo.accept_reply(*cols), "plain round after the refusals")
    assert eh.snapshot(g)[0].tobytes() == eo.snapshot(g)[0].tobytes()
    assert eh.counters() == eo.counters()
    del block, o_p, o_d, tp, tv, e0, e1
    eh.close(force=True)
    eo.close()
