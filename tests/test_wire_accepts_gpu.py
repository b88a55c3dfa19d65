"""gpx_wire_pack_accepts_dev / gpx_wire_request_sizes_dev on the GPU: the device chain REQUEST frames -> decode_dev
-> request_sizes_dev -> request_batch_dev -> propose_batch_dev -> pack_accepts_dev against the restatement of
latchToBatch + makeAcceptFrame (tests/wire_accepts_model.py), byte for byte."""
import struct

import numpy as np
import pytest

from gigapaxos_amd import Engine, hri_create, S_OK, D_DECISION, C_HASVALUE, A_STOP
from gigapaxos_amd import wire as W
from tests import wire_accepts_model as AM
from tests import wire_model as JM

pytestmark = pytest.mark.gpu

MY_ID = 100


def _coordinator(lib, names, max_batch=1 << 16, my_id=MY_ID, k=3, coord=MY_ID):
    G = len(names)
    e = Engine(lib, my_id, G, kmax=k, window=8, max_batch=max_batch)
    we = W.WireEngine(e)
    members = np.tile(np.arange(MY_ID, MY_ID + k, dtype=np.int32), (G, 1))
    assert (e.create_groups(np.arange(G, dtype=np.int32), members, k, hri_create(G, k, coord)) == S_OK).all()
    assert (we.bind(names, np.arange(G, dtype=np.int32)) == S_OK).all()
    return e, we


def _names(rng, G):
    out = []
    for g in range(G):
        ln = int(rng.integers(1, 128))
        nm = (b"n%d." % g + bytes(rng.integers(0x21, 0x7f, 127).astype(np.uint8)))[:ln]
        out.append(nm if len(nm) >= len(b"n%d." % g) else b"n%d." % g)
    assert len(set(out)) == G
    return out


def _single_frames(rng, names, n):
    frames = []
    for i in range(n):
        g = int(rng.integers(0, len(names)))
        frames.append(AM.random_request(rng, names[g], 0, (i << 16) | g))
    return frames


@pytest.mark.gpu_fast
def test_single_request_proposals_small(hip_lib):
    rng = np.random.default_rng(1)
    names = _names(rng, 40)
    e, we = _coordinator(hip_lib, names)
    try:
        frames = _single_frames(rng, names, 200)
        r = AM.Chain(we).run(frames, batch=False)
        assert r["m"] == 200
        want, have = AM.check_against_model(r, frames, MY_ID)
        # more than `window` proposals of one group in a call: those past the window are refused (GPX_S_WINDOW)
        assert len(have) == int((r["status"] == S_OK).sum()) > 150
    finally:
        e.close()


@pytest.mark.parametrize("lead", list(range(16)))
def test_single_request_proposals_every_lead_offset(hip_lib, lead):
    rng = np.random.default_rng(100 + lead)
    names = _names(rng, 300)
    e, we = _coordinator(hip_lib, names)
    try:
        frames = _single_frames(rng, names, 600)
        r = AM.Chain(we).run(frames, batch=False, lead=lead)
        AM.check_against_model(r, frames, MY_ID)
    finally:
        e.close()


@pytest.mark.parametrize("seed,max_size,max_bytes", [(3, 4, 1 << 20), (4, 50, 6000), (5, 2000, 1 << 20)])
def test_batches_from_request_batch(hip_lib, seed, max_size, max_bytes):
    rng = np.random.default_rng(seed)
    names = _names(rng, 30)
    e, we = _coordinator(hip_lib, names)
    try:
        frames = _single_frames(rng, names, 900)
        r = AM.Chain(we).run(frames, batch=True, max_size=max_size, max_bytes=max_bytes)
        assert (r["b_count"] > 1).any()
        want, have = AM.check_against_model(r, frames, MY_ID)
        # the Java reading of every frame: the leader's request id, FIFO member order, the total count
        req = [frames[int(fi)] for fi in r["rec_frame"]]
        for f, b in enumerate(have):
            fr = r["out"][r["frame_off"][f]:r["frame_off"][f] + r["frame_len"][f]].tobytes()
            st, t, p = JM.to_paxos_packet(fr)
            assert st == W.W_OK and t == W.WT_ACCEPT
            L = int(r["b_leader"][b])
            mem = [L] + [i for i in range(r["m"]) if r["leader"][i] == L and i != L]
            assert p.request_id == struct.unpack_from(">q", req[L], 13 + req[L][12])[0]
            if r["b_count"][b] > 1:
                want_n = sum(AM.request_head(req[i])[1] for i in mem) + len(mem) - 1
                assert len(p.batched or ()) == want_n
                ids = [q.request_id for q in p.batched or ()]
                heads = [struct.unpack_from(">q", req[i], 13 + req[i][12])[0] for i in mem[1:]]
                assert [x for x in ids if x in set(heads)] == heads  # FIFO
    finally:
        e.close()


def test_non_ok_status_gives_no_frame(hip_lib):
    rng = np.random.default_rng(7)
    names = _names(rng, 50)
    e, we = _coordinator(hip_lib, names)
    try:
        frames = _single_frames(rng, names, 500)
        bad = np.array([1, 2, 3, 4, 5, 8, 9], np.uint8)

        def st(s):
            s = s.copy()
            pick = rng.random(s.shape[0]) < 0.5
            s[pick] = bad[rng.integers(0, bad.shape[0], int(pick.sum()))]
            return s
        r = AM.Chain(we).run(frames, batch=True, max_size=3, status_fn=st)
        want, have = AM.check_against_model(r, frames, MY_ID)
        assert (r["frame_of"][r["status"] != 0] == -1).all()
        assert len(have) == int((r["status"] == 0).sum())
    finally:
        e.close()


def test_cap_too_small(hip_lib):
    rng = np.random.default_rng(8)
    names = _names(rng, 50)
    e, we = _coordinator(hip_lib, names)
    try:
        frames = _single_frames(rng, names, 400)
        full = AM.Chain(we).run(frames, batch=False)
        cap = (full["n_bytes"] // 3) & ~3
        e.close()
        e, we = _coordinator(hip_lib, names)  # the same slots again
        r = AM.Chain(we).run(frames, batch=False, cap_bytes=cap + 2)
        assert r["n_bytes"] == full["n_bytes"] > r["cap"]
        AM.check_against_model(r, frames, MY_ID)  # every frame that fits is exact
        ends = r["frame_off"] + ((r["frame_len"] + 3) & ~3)
        fit_end = int(ends[ends <= r["cap"]].max())
        assert (r["out"][fit_end:] == 0xAB).all()  # nothing of a frame that does not fit, nothing past cap
    finally:
        e.close()


def test_n_dev_count(hip_lib):
    rng = np.random.default_rng(9)
    names = _names(rng, 60)
    e, we = _coordinator(hip_lib, names)
    try:
        frames = _single_frames(rng, names, 300)
        r = AM.Chain(we).run(frames, batch=True, max_size=5, use_n_dev=True)
        AM.check_against_model(r, frames, MY_ID)
        k = r["nB"] // 2
        r2 = AM.Chain(we).run(frames, batch=True, max_size=5, use_n_dev=True, n_dev_value=k)
        assert r2["nB"] == r["nB"]
        AM.check_against_model(r2, frames, MY_ID, n_props=k)
    finally:
        e.close()


def test_request_sizes_match_host(hip_lib):
    rng = np.random.default_rng(10)
    names = _names(rng, 40)
    e, we = _coordinator(hip_lib, names)
    try:
        frames = _single_frames(rng, names, 700)
        r = AM.Chain(we).run(frames, batch=False)
        req = [frames[int(fi)] for fi in r["rec_frame"]]
        assert r["est"].tolist() == [len(f) for f in req]
        assert r["weight"].tolist() == [AM.request_head(f)[1] + 1 for f in req]
    finally:
        e.close()


def _fixed_requests(name_rows, value_len, rid0=0):
    """REQUEST frames of equal length, requestID = rid0 + index (the request part of W.accept_frames_fixed)"""
    buf, off = W.accept_frames_fixed(name_rows, 0, 0, 0, 0, 0, 0, value_len=value_len)
    n = name_rows.shape[0]
    L = int(off[1]) - AM.ACCEPT_TAIL
    f = buf.reshape(n, -1)[:, :L].copy()
    f[:, 4:8] = np.frombuffer(struct.pack(">i", W.WT_REQUEST), np.uint8)
    o = 13 + name_rows.shape[1]
    rid = np.arange(rid0, rid0 + n, dtype=np.int64)
    f[:, o:o + 4] = W._be32_cols(rid >> 32)
    f[:, o + 4:o + 8] = W._be32_cols(rid & 0xFFFFFFFF)
    return f


def test_scale_and_skew(hip_lib):
    """1 M groups: a proposal of one 64-byte request for each but the last, one batch of 2,000 requests of 1 KB for
    the last, checked exactly (the engine sized as scripts/bench_wire.py's)"""
    import torch
    G, NB, VB = 1_000_000, 2000, 1024
    G1 = G - 1
    names = W.fixed_names(np.arange(G))
    e = Engine(hip_lib, MY_ID, G, kmax=3, window=8, max_batch=2 * G + 1024)
    we = W.WireEngine(e)
    try:
        mem = np.tile(np.array([100, 101, 102], np.int32), (G, 1))
        assert (e.create_groups(np.arange(G, dtype=np.int32), mem, 3, hri_create(G, 3, MY_ID)) == S_OK).all()
        for g0 in range(0, G, 125_000):
            rows = np.arange(g0, min(G, g0 + 125_000), dtype=np.int32)
            nb_ = np.ascontiguousarray(names[rows].reshape(-1))
            noff = np.arange(rows.shape[0] + 1, dtype=np.int32) * names.shape[1]
            st = np.zeros(rows.shape[0], np.uint8)
            we.lib.check(we.lib.fn["names_bind"](e.h, rows.shape[0], nb_.ctypes.data, noff.ctypes.data,
                                                 rows.ctypes.data, st.ctypes.data), "names_bind")
            assert (st == S_OK).all(), (g0, np.bincount(st))
        singles = _fixed_requests(names[:G1], 64)
        big = _fixed_requests(np.repeat(names[G1:G1 + 1], NB, axis=0), VB, rid0=1 << 40)
        # the big batch's records sit in the middle of the burst
        h = G1 // 2
        rows = [singles[:h], big, singles[h:]]
        lens = np.concatenate([np.full(h, singles.shape[1]), np.full(NB, big.shape[1]),
                               np.full(G1 - h, singles.shape[1])]).astype(np.int64)
        buf = np.concatenate([x.reshape(-1) for x in rows])
        off = np.zeros(G1 + NB + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        dev = torch.device("cuda:0")
        n = G1 + NB
        d_buf, d_off = torch.from_numpy(buf).to(dev), torch.from_numpy(off).to(dev)
        i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)  # noqa: E731
        u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device=dev)  # noqa: E731
        P = lambda t: t.data_ptr()  # noqa: E731
        rg, rs, ri, rf = i32(n), u8(n), torch.zeros(n, dtype=torch.int64, device=dev), i32(n)
        counts = i32(8)
        torch.cuda.synchronize()
        W.decode_dev(we, n, P(d_buf), P(d_off), P(u8(n)), P(i32(n)), P(i32(n)),
                     requests=(n, [P(rg), P(rs), P(ri), P(rf)]), counts_ptr=P(counts))
        est, wgt, leader, bst = i32(n), i32(n), i32(n), u8(n)
        W.request_sizes_dev(we, n, P(d_buf), P(d_off), n, P(rf), P(est), P(wgt))
        bc = [i32(n) for _ in range(5)]
        bstop, nbt = u8(n), i32(1)
        we.lib.check(we.lib.fn["request_batch_dev"](e.h, n, W._VP(P(rg)), W._VP(P(est)), W._VP(P(wgt)), W._VP(P(rs)),
                                                    4 << 20, NB, W._VP(P(leader)), W._VP(P(bst)),
                                                    *[W._VP(P(c)) for c in bc], W._VP(P(bstop)), W._VP(P(nbt))),
                     "request_batch_dev")
        torch.cuda.synchronize()
        nB = int(nbt[0])
        assert nB == G1 + 1
        pc = [i32(nB) for _ in range(4)]
        pst = u8(nB)
        e.call_dev("propose_batch", nB, P(bc[0]), P(bstop), *[P(c) for c in pc], P(pst))
        cap = int(off[-1]) + 32 * nB + 64 * NB
        out = torch.full((cap,), 0xAB, dtype=torch.uint8, device=dev)
        foff, flen, fgi, fba, fof = (torch.zeros(nB, dtype=torch.int64, device=dev), i32(nB), i32(nB), i32(nB),
                                     i32(nB))
        nfo, nbo = i32(1), torch.zeros(1, dtype=torch.int64, device=dev)
        W.pack_accepts_dev(we, n, P(d_buf), P(d_off), n, P(rf), P(leader), nB, P(nbt), (P(bc[0]), P(bc[1]), P(bc[2])),
                           [P(c) for c in pc] + [P(pst)], P(out), cap, P(foff), P(flen), P(fgi), P(fba), P(fof),
                           P(nfo), P(nbo))
        torch.cuda.synchronize()
        assert (pst.cpu().numpy() == S_OK).all()
        assert int(nfo[0]) == nB and int(nbo[0]) <= cap
        o = out.cpu().numpy()
        fo, fl, fb = foff.cpu().numpy(), flen.cpu().numpy(), fba.cpu().numpy()
        b_leader, b_count = bc[1][:nB].cpu().numpy(), bc[2][:nB].cpu().numpy()
        slot, bnum, bcoord, med = (c.cpu().numpy() for c in pc)
        recf = rf[:n].cpu().numpy()
        assert (fb == np.arange(nB)).all()
        # the big batch: the restatement
        bigb = int(np.nonzero(b_count > 1)[0][0])
        assert b_count[bigb] == NB
        reqs = {}
        ld = leader[:n].cpu().numpy()
        mem_ = [i for i in range(n) if ld[i] == b_leader[bigb]]
        for i in mem_:
            fi = int(recf[i])
            reqs[i] = buf[off[fi]:off[fi + 1]].tobytes()
        L = int(b_leader[bigb])
        want = AM.make_accept(AM.latch_to_batch(reqs[L], [reqs[i] for i in mem_ if i != L]), int(slot[bigb]),
                              int(bnum[bigb]), int(bcoord[bigb]), int(med[bigb]), MY_ID)
        f = bigb
        assert fl[f] == len(want) and o[fo[f]:fo[f] + fl[f]].tobytes() == want
        # the singles, vectorised: request bytes with the type patched, then the tail
        sel = np.nonzero(b_count == 1)[0]
        Ls = b_leader[sel]
        R = singles.shape[1]
        assert (fl[sel] == R + AM.ACCEPT_TAIL).all()
        for c0 in range(0, sel.shape[0], 100_000):
            s = sel[c0:c0 + 100_000]
            got = o[fo[s][:, None] + np.arange(R + AM.ACCEPT_TAIL)[None, :]]
            src = recf[Ls[c0:c0 + 100_000]].astype(np.int64)
            exp = np.empty_like(got)
            exp[:, :R] = buf[off[src][:, None] + np.arange(R)[None, :]]
            exp[:, 4:8] = np.frombuffer(struct.pack(">i", W.WT_ACCEPT), np.uint8)
            t = np.zeros((s.shape[0], AM.ACCEPT_TAIL), np.uint8)
            t[:, 0:4], t[:, 4:8], t[:, 8:12] = W._be32_cols(slot[s]), W._be32_cols(bnum[s]), W._be32_cols(bcoord[s])
            t[:, 13:17], t[:, 18:22] = W._be32_cols(med[s]), W._be32_cols(np.full(s.shape[0], MY_ID))
            exp[:, R:] = t
            assert (got == exp).all(), c0
        pad = (fl + 3) & ~3
        assert (fo[1:] == fo[:-1] + pad[:-1]).all() and int(nbo[0]) == int(fo[-1] + pad[-1])
    finally:
        e.close()


def test_round_trip_through_both_decoders_and_accept(hip_lib, oracle_lib):
    rng = np.random.default_rng(11)
    names = _names(rng, 80)
    e, we = _coordinator(hip_lib, names)
    acc = []
    try:
        frames = _single_frames(rng, names, 500)
        r = AM.Chain(we).run(frames, batch=True, max_size=4)
        AM.check_against_model(r, frames, MY_ID)
        packed = [r["out"][r["frame_off"][f]:r["frame_off"][f] + r["frame_len"][f]].tobytes()
                  for f in range(r["n_frames"])]
        req = [frames[int(fi)] for fi in r["rec_frame"]]
        results = []
        for lib in (hip_lib, oracle_lib):
            a, wa = _coordinator(lib, names, my_id=MY_ID + 1)
            acc.append(a)
            d = wa.decode(packed)
            assert (d.f_status == W.W_OK).all()
            A = d.accepts
            b = r["f_batch"]
            assert A["slot"].tolist() == r["slot"][b].tolist()
            assert A["bnum"].tolist() == r["bnum"][b].tolist() and A["bcoord"].tolist() == r["bcoord"][b].tolist()
            assert A["median_cp"].tolist() == r["median"][b].tolist()
            assert (A["sender"] == MY_ID).all() and A["gidx"].tolist() == r["b_gidx"][b].tolist()
            lids = [struct.unpack_from(">q", req[L], 13 + req[L][12])[0] for L in r["b_leader"][b]]
            assert A["req_id"].tolist() == lids
            mem = {}
            for i, L in enumerate(r["leader"]):
                mem.setdefault(int(L), []).append(i)
            stops = [int(any(JM.is_stop_request(JM.to_paxos_packet(req[i])[2]) for i in mem[int(L)]))
                     for L in r["b_leader"][b]]
            assert (A["flags"] & A_STOP).tolist() == stops
            out, runs = a.accept(A["gidx"], A["bnum"], A["bcoord"], A["slot"], A["median_cp"], A["flags"])
            results.append([np.asarray(x).tolist() for x in out])
        assert results[0] == results[1]
    finally:
        e.close()
        for a in acc:
            a.close()


class DeviceAcceptCluster:
    """tests/wire_cluster.py's WireCluster with ONE hop swapped: the coordinator's ACCEPT frames come from the
    device chain (decode_dev -> request_sizes_dev -> propose_batch_dev -> pack_accepts_dev) instead of W.accept"""

    @staticmethod
    def make(lib, node_ids, names, coord):
        from tests.wire_cluster import WireCluster

        class _C(WireCluster):
            def round(self, groups, rnd, value_len=64):
                groups = np.asarray(groups, np.int32)
                inbox_acc = {nid: [] for nid in self.ids}
                for c in self.ids:
                    mine = groups[self.coord[groups] == c]
                    if mine.size == 0:
                        continue
                    req_frames = [W.request(self.names[g], 0, (rnd << 32) | int(g), bytes([g & 0xFF]) * value_len)
                                  for g in mine]
                    self.trace += req_frames
                    r = AM.Chain(self.wire[c]).run(req_frames, batch=False)
                    assert (r["status"] == S_OK).all() and r["n_frames"] == len(req_frames)
                    for f in range(r["n_frames"]):
                        acc = r["out"][r["frame_off"][f]:r["frame_off"][f] + r["frame_len"][f]].tobytes()
                        for nid in [c] + [n for n in self.ids if n != c]:
                            inbox_acc[nid].append(acc)
                return self.after_accepts(inbox_acc)

            def after_accepts(self, inbox_acc):
                """the rest of WireCluster.round, from the acceptors' decode of the ACCEPT frames on"""
                inbox_bar = {nid: [] for nid in self.ids}
                for nid in self.ids:
                    if not inbox_acc[nid]:
                        continue
                    self.trace += inbox_acc[nid]
                    d = self.wire[nid].decode(inbox_acc[nid])
                    assert (d.f_status == W.W_OK).all()
                    a = d.accepts
                    (rb, rc, rm, rf, st), runs = self.eng[nid].accept(a["gidx"], a["bnum"], a["bcoord"], a["slot"],
                                                                      a["median_cp"], a["flags"])
                    assert runs.gidx.shape[0] == 0
                    frames, fg, fd, ub, _ = self.wire[nid].pack_accept_replies(a["gidx"], a["slot"], rb, rc, rm, st,
                                                                               sender=a["sender"], req_id=a["req_id"])
                    assert not ub.any()
                    for f, dest in zip(frames, fd):
                        inbox_bar[int(dest)].append(f)
                inbox_bc = {nid: [] for nid in self.ids}
                decisions = {}
                for c in self.ids:
                    if not inbox_bar[c]:
                        continue
                    self.trace += inbox_bar[c]
                    d = self.wire[c].decode(inbox_bar[c])
                    assert (d.f_status == W.W_OK).all()
                    v = d.votes
                    dec = self.eng[c].accept_reply(v["gidx"], v["bnum"], v["bcoord"], v["slot"], v["acceptor"],
                                                   v["max_cp"])
                    decisions[c] = dec
                    frames, fg, _ = self.wire[c].pack_commits(dec)
                    for nid in self.ids:
                        if nid != c:
                            inbox_bc[nid] += frames
                    sel = dec.kind == D_DECISION
                    st, runs = self.eng[c].commit(dec.gidx[sel], dec.bnum[sel], dec.bcoord[sel], dec.slot[sel],
                                                  dec.median_cp[sel], np.full(int(sel.sum()), C_HASVALUE, np.uint8))
                    assert (st == S_OK).all()
                    self.exec_log[c].append(runs.as_tuple_array())
                for nid in self.ids:
                    if not inbox_bc[nid]:
                        continue
                    self.trace += inbox_bc[nid]
                    d = self.wire[nid].decode(inbox_bc[nid])
                    assert (d.f_status == W.W_OK).all()
                    cm = d.commits
                    st, runs = self.eng[nid].commit(cm["gidx"], cm["bnum"], cm["bcoord"], cm["slot"], cm["median_cp"],
                                                    cm["kind"])
                    assert (st == S_OK).all()
                    self.exec_log[nid].append(runs.as_tuple_array())
                return decisions

        return _C(lib, node_ids, names, coord)


def test_three_replica_cluster_with_device_accepts(hip_lib, oracle_lib):
    """the round of tests/wire_cluster.py with the coordinator's ACCEPT frames from the device chain: the wire
    trace, execution logs and snapshots equal the oracle cluster's (which builds them with W.accept)"""
    from tests.wire_cluster import WireCluster
    G, R = 1500, 5
    names = [b"service/%d" % g for g in range(G)]
    rng = np.random.default_rng(12)
    coord = rng.choice([100, 101, 102], size=G).astype(np.int32)
    ch = DeviceAcceptCluster.make(hip_lib, [100, 101, 102], names, coord)
    co = WireCluster(oracle_lib, [100, 101, 102], names, coord)
    try:
        for r in range(R):
            grp = rng.permutation(G)[: G - 100 * r]
            dh, do = ch.round(grp, r), co.round(grp, r)
            assert sorted(dh) == sorted(do)
            for c in dh:
                assert (dh[c].as_tuple_array() == do[c].as_tuple_array()).all()
        assert ch.trace == co.trace
        for nid in (100, 101, 102):
            assert ch.executed(nid).tolist() == co.executed(nid).tolist()
            sh, so = ch.eng[nid].snapshot(np.arange(G))[0], co.eng[nid].snapshot(np.arange(G))[0]
            assert sh.tobytes() == so.tobytes()
    finally:
        ch.close()
        co.close()


def test_profile_shows_the_new_kernels(hip_lib):
    rng = np.random.default_rng(13)
    names = _names(rng, 20)
    e, we = _coordinator(hip_lib, names)
    try:
        e.profile(2)
        frames = _single_frames(rng, names, 100)
        AM.Chain(we).run(frames, batch=True, max_size=3)
        e.sync()
        ks = e.profile_read()
        e.profile(0)
        for k in ("k_acc_req_sizes", "k_acc_parse", "k_acc_size", "k_acc_place", "k_acc_members", "k_acc_rank",
                  "k_acc_copy"):
            assert ks.get(k, (0, 0))[0] >= 1, (k, sorted(ks))
    finally:
        e.close()
