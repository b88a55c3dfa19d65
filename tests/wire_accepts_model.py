"""A Python restatement of what the coordinator sends for a proposal (the checker of gpx_wire_pack_accepts_dev):
RequestPacket.latchToBatch / toArray (RequestPacket.java:1090-1150) and AcceptPacket.toBytes (AcceptPacket.java:95-135),
read the way gigapaxos_amd/host/gpx_host.cpp's latchToBatch + makeAcceptFrame build them; plus the device chain
REQUEST frames -> decode_dev -> request_sizes_dev -> request_batch_dev -> propose_batch_dev -> pack_accepts_dev over
torch buffers."""
import struct

import numpy as np

from gigapaxos_amd import wire as W

ACCEPT_TAIL = 22


def request_head(f):
    """-> (h, nb, e): offset of the batched-count field, the batched count, the end of the batched list
    (None where RequestPacket(byte[]) would throw)"""
    try:
        if len(f) < 13:
            return None
        idl = f[12]
        if idl >= 128:
            return None
        p = 13 + idl + 39
        dl = struct.unpack_from(">i", f, p)[0]
        p += 4 + max(dl, 0)
        for _ in range(2):
            vl = struct.unpack_from(">i", f, p)[0]
            if vl < 0:
                return None
            p += 4 + vl
        h = p
        nb = struct.unpack_from(">i", f, p)[0]
        if nb < 0:
            return None
        p += 4
        for _ in range(nb):
            ln = struct.unpack_from(">i", f, p)[0]
            if ln < 0 or p + 4 + ln > len(f):
                return None
            p += 4 + ln
        if p > len(f):
            return None
        return h, nb, p
    except struct.error:
        return None


def elements(f):
    """RequestPacket.toArray of one frame: its head with an empty batched list, then its own batched elements"""
    h, nb, _ = request_head(f)
    out, p = [f[:h] + struct.pack(">i", 0)], h + 4
    for _ in range(nb):
        ln = struct.unpack_from(">i", f, p)[0]
        out.append(f[p + 4:p + 4 + ln])
        p += 4 + ln
    return out


def latch_to_batch(first, rest):
    """first.latchToBatch(rest): the head of `first`, then every unbatched request of first and rest as its batched list"""
    allr = elements(first)
    for r in rest:
        allr += elements(r)
    head = allr[0][:-4]
    return head + struct.pack(">i", len(allr) - 1) + b"".join(struct.pack(">i", len(x)) + x for x in allr[1:])


def make_accept(req, slot, bnum, bcoord, median, sender):
    """AcceptPacket.toBytes over the request bytes: the packet type int -> ACCEPT, then the 22-byte tail"""
    return (req[:4] + struct.pack(">i", W.WT_ACCEPT) + req[8:]
            + struct.pack(">iiibibi", slot, bnum, bcoord, 0, median, 0, sender))


def expected_accepts(req_frames, leader, b_leader, b_count, slot, bnum, bcoord, median, status, my_id):
    """per proposal the ACCEPT frame gpx_host.cpp would send, or None.  req_frames[i] = record i's REQUEST frame."""
    members = {}
    for i, L in enumerate(leader):
        if L >= 0 and L != i:
            members.setdefault(int(L), []).append(i)
    out, seen = [], set()
    for b in range(len(b_leader)):
        L = int(b_leader[b])
        if status[b] != 0 or L in seen or request_head(req_frames[L]) is None:
            out.append(None)
            seen.add(L)
            continue
        seen.add(L)
        if b_count[b] > 1:
            rest = [req_frames[i] for i in members.get(L, [])]
            if any(request_head(r) is None for r in rest):
                out.append(None)
                continue
            req = latch_to_batch(req_frames[L], rest)
        else:
            req = req_frames[L]
        out.append(make_accept(req, int(slot[b]), int(bnum[b]), int(bcoord[b]), int(median[b]), my_id))
    return out


def random_request(rng, name, version, rid, depth=0, max_value=1000):
    """a REQUEST frame with odd-length value, optional digest / response and (at depth 0) its own batched list"""
    value = bytes(rng.integers(0, 256, int(rng.integers(0, max_value + 1))).astype(np.uint8))
    digest = bytes(rng.integers(0, 256, int(rng.integers(1, 20))).astype(np.uint8)) if rng.random() < 0.3 else b""
    resp = bytes(rng.integers(0, 256, int(rng.integers(1, 30))).astype(np.uint8)) if rng.random() < 0.3 else b""
    batched = ()
    if depth == 0 and rng.random() < 0.3:
        batched = [random_request(rng, name, version, rid * 7 + q + 1, depth + 1, 200) for q in range(int(rng.integers(1, 4)))]
    return W.request(name, version, rid, value, stop=bool(rng.random() < 0.05), batched=batched,
                     entry_replica=int(rng.integers(-1, 5)), digest=digest, response=resp)


# ---- the device chain over torch buffers -------------------------------------------------------------------------


class Chain:
    """decode_dev -> request_sizes_dev -> request_batch_dev -> propose_batch_dev -> pack_accepts_dev on one engine,
    with every intermediate column kept for the checks"""

    def __init__(self, we, dev="cuda:0"):
        import torch
        self.torch, self.we, self.dev = torch, we, torch.device(dev)

    def _i32(self, n):
        return self.torch.zeros(max(n, 1), dtype=self.torch.int32, device=self.dev)

    def run(self, frames, batch=True, max_bytes=1 << 20, max_size=2000, lead=0, cap_bytes=None, status_fn=None,
            use_n_dev=False, n_dev_value=None):
        torch, we = self.torch, self.we
        P = lambda t: t.data_ptr()  # noqa: E731
        buf, off = W.concat_frames(frames)
        n = len(frames)
        # the burst starts `lead` bytes into the buffer (garbage before it): every source offset shifts
        host = np.concatenate([np.random.default_rng(lead).integers(0, 256, lead).astype(np.uint8), buf])
        raw = torch.from_numpy(host).to(self.dev)
        fptr = P(raw)
        d_off = torch.from_numpy(off + lead).to(self.dev)
        torch.cuda.synchronize()  # torch's copies before the engine's stream reads them
        fst, fg, ft = (torch.zeros(n, dtype=torch.uint8, device=self.dev), self._i32(n), self._i32(n))
        rg, rs, ri, rf = self._i32(n), torch.zeros(n, dtype=torch.uint8, device=self.dev), \
            torch.zeros(n, dtype=torch.int64, device=self.dev), self._i32(n)
        counts = self._i32(8)
        W.decode_dev(we, n, fptr, P(d_off), P(fst), P(fg), P(ft), requests=(n, [P(rg), P(rs), P(ri), P(rf)]),
                     counts_ptr=P(counts))
        torch.cuda.synchronize()
        m = int(counts[3])
        est, wgt = self._i32(m), self._i32(m)
        W.request_sizes_dev(we, n, fptr, P(d_off), m, P(rf), P(est), P(wgt))
        leader, bst = self._i32(m), torch.zeros(max(m, 1), dtype=torch.uint8, device=self.dev)
        bcols = [self._i32(m) for _ in range(5)]
        bstop, nb = torch.zeros(max(m, 1), dtype=torch.uint8, device=self.dev), self._i32(1)
        if batch:
            we.lib.check(we.lib.fn["request_batch_dev"](we.e.h, m, W._VP(P(rg)), W._VP(P(est)), W._VP(P(wgt)),
                                                        W._VP(P(rs)), int(max_bytes), int(max_size), W._VP(P(leader)),
                                                        W._VP(P(bst)), *[W._VP(P(c)) for c in bcols],
                                                        W._VP(P(bstop)), W._VP(P(nb))), "request_batch_dev")
            torch.cuda.synchronize()
            nB = int(nb[0])
            b_gidx, b_leader, b_count = bcols[0], bcols[1], bcols[2]
            pst = bstop
        else:
            nB = m
            b_gidx, b_leader, b_count, pst = rg, None, None, rs
        pcols = [self._i32(nB) for _ in range(4)]
        pstat = torch.zeros(max(nB, 1), dtype=torch.uint8, device=self.dev)
        if nB:
            we.e.call_dev("propose_batch", nB, P(b_gidx), P(pst), *[P(c) for c in pcols], P(pstat))
        torch.cuda.synchronize()
        if status_fn is not None and nB:
            pstat[:nB] = torch.from_numpy(status_fn(pstat[:nB].cpu().numpy())).to(self.dev)
            torch.cuda.synchronize()
        total_est = int(est[:m].sum()) + 64 * max(m, 1) if m else 64
        cap = total_est if cap_bytes is None else int(cap_bytes)
        out = torch.full((cap + 256,), 0xAB, dtype=torch.uint8, device=self.dev)
        foff, flen = torch.zeros(max(nB, 1), dtype=torch.int64, device=self.dev), self._i32(nB)
        fgi, fba, fof = self._i32(nB), self._i32(nB), self._i32(nB)
        nfo, nbo = self._i32(1), torch.zeros(1, dtype=torch.int64, device=self.dev)
        n_dev = None
        if use_n_dev:
            n_dev = self._i32(1)
            n_dev[0] = nB if n_dev_value is None else n_dev_value
        torch.cuda.synchronize()
        W.pack_accepts_dev(we, n, fptr, P(d_off), m, P(rf), P(leader) if batch else 0, nB + (5 if use_n_dev else 0),
                           P(n_dev) if use_n_dev else 0,
                           (P(b_gidx), P(b_leader) if batch else 0, P(b_count) if batch else 0),
                           [P(c) for c in pcols] + [P(pstat)], P(out), cap, P(foff), P(flen), P(fgi), P(fba), P(fof),
                           P(nfo), P(nbo))
        torch.cuda.synchronize()
        np_ = lambda t, k: t[:k].cpu().numpy()  # noqa: E731
        nF = int(nfo[0])
        r = dict(m=m, nB=nB, n_frames=nF, n_bytes=int(nbo[0]), cap=cap, out=out.cpu().numpy(),
                 frame_off=np_(foff, nF), frame_len=np_(flen, nF), f_gidx=np_(fgi, nF), f_batch=np_(fba, nF),
                 frame_of=np_(fof, nB), est=np_(est, m), weight=np_(wgt, m), rec_frame=np_(rf, m),
                 rec_gidx=np_(rg, m), leader=np_(leader, m) if batch else np.arange(m, dtype=np.int32),
                 b_gidx=np_(b_gidx, nB), b_leader=np_(b_leader, nB) if batch else np.arange(nB, dtype=np.int32),
                 b_count=np_(b_count, nB) if batch else np.ones(nB, np.int32),
                 slot=np_(pcols[0], nB), bnum=np_(pcols[1], nB), bcoord=np_(pcols[2], nB), median=np_(pcols[3], nB),
                 status=np_(pstat, nB), counts=counts.cpu().numpy())
        return r


def check_against_model(r, frames, my_id, n_props=None):
    """every frame of a Chain.run result equals the restatement byte for byte; pad bytes are zero"""
    nB = r["nB"] if n_props is None else n_props
    req = [frames[int(fi)] for fi in r["rec_frame"]]
    want = expected_accepts(req, r["leader"], r["b_leader"][:nB], r["b_count"][:nB], r["slot"], r["bnum"], r["bcoord"],
                            r["median"], r["status"][:nB], my_id)
    have_f = [b for b in range(nB) if want[b] is not None]
    assert r["n_frames"] == len(have_f)
    assert r["f_batch"].tolist() == have_f
    assert r["f_gidx"].tolist() == [int(r["b_gidx"][b]) for b in have_f]
    fo = r["frame_of"][:nB].tolist()
    assert fo == [have_f.index(b) if want[b] is not None else -1 for b in range(nB)]
    pos = 0
    out = r["out"]
    for f, b in enumerate(have_f):
        w = want[b]
        assert int(r["frame_off"][f]) == pos and int(r["frame_len"][f]) == len(w)
        end = pos + ((len(w) + 3) & ~3)
        if end <= r["cap"]:
            assert out[pos:pos + len(w)].tobytes() == w, f"frame {f} (proposal {b})"
            assert not out[pos + len(w):end].any(), "pad bytes"
        pos = end
    assert r["n_bytes"] == pos
    return want, have_f
