"""Shared pieces of the journal tests (include/gpx_journal.h): the five ACCEPT rounds whose log flags the oracle decides,
directed frame sets, and - for the GPU file - the _dev call on buffers inside guard bands."""
import numpy as np

from gigapaxos_amd import Engine, hri_create, S_OK, wire as W
from tests import journal_model as M

GROUPS, K, WINDOW, ME, CREATOR = 300, 3, 8, 101, 100
SLOTS = 12
ROUNDS = [(0, 100), (0, 100), (1, 102), (0, 100), (1, 102)]    # the ballot of each round's ACCEPTs
ROUND_OK = [2400, 2400, 2400, 3600, 2400]                      # records answered GPX_S_OK
ROUND_LOGGED = [2400, 0, 2400, 0, 0]                           # ... of which must be logged
GUARD = 4096
SENTINEL = 0xA5


def rounds_engine(lib):
    """300 groups of three, window 8, on node 101, created as the coordinator 100 left them; names bound for the decode"""
    e = Engine(lib, ME, GROUPS, kmax=K, window=WINDOW, max_batch=1 << 14)
    mem = np.tile(np.arange(CREATOR, CREATOR + K, dtype=np.int32), (GROUPS, 1))
    assert (e.create_groups(np.arange(GROUPS), mem, K, hri_create(GROUPS, K, CREATOR)) == S_OK).all()
    we = W.WireEngine(e)
    assert (we.bind(round_names(), np.arange(GROUPS)) == S_OK).all()
    return e, we


def round_names():
    return [b"svc-%d" % g for g in range(GROUPS)]


def round_records(seed=7):
    """ACCEPTs for slots 1 .. 12 of every group, shuffled: the same 3,600 (group, slot) in every round"""
    g = np.repeat(np.arange(GROUPS, dtype=np.int32), SLOTS)
    s = np.tile(np.arange(1, SLOTS + 1, dtype=np.int32), GROUPS)
    p = np.random.default_rng(seed).permutation(g.size)
    return g[p], s[p]


def round_frames(g, s, bnum, bcoord):
    """the ACCEPT frames of one round (AcceptPacket.toBytes, gigapaxos_amd/wire.py), values of 0 .. 36 bytes"""
    names = round_names()
    return [W.accept(names[int(a)], 0, 1000 + i, int(b), bnum, bcoord, 0, bcoord, value=bytes([65 + i % 26]) * (i % 37))
            for i, (a, b) in enumerate(zip(g, s))]


def oracle_round(eo, wo, frames):
    """one round on the oracle: decode, accept -> (the decoded ACCEPT columns, r_flags, status)"""
    d = wo.decode(frames)
    n = d.counts["n_accepts"]
    assert n == len(frames) and d.counts["n_bad_frames"] == 0
    A = {k: v[:n] for k, v in d.accepts.items()}
    (_, _, _, r_flags, status), _ = eo.accept(A["gidx"], A["bnum"], A["bcoord"], A["slot"], A["median_cp"], A["flags"])
    return A, r_flags, status


def logged(r_flags, status):
    return (status == M.S_OK) & ((r_flags & M.R_TOLOG) != 0)


# ---- directed frame sets ---------------------------------------------------------------------------------------------
def frames_of_lengths(lens, seed=1, padded=False):
    """(block, frame_off, frame_len or None): frames of the given lengths filled with bytes 1 .. 250.  padded: the pack
    calls' form - 4-byte aligned starts, 0xFF pad bytes that must never be copied - else contiguous"""
    rng = np.random.default_rng(seed)
    parts, off, pos = [], [], 0
    for ln in lens:
        off.append(pos)
        parts.append(rng.integers(1, 251, int(ln)).astype(np.uint8))
        pos += int(ln)
        if padded and pos % 4:
            parts.append(np.full(4 - pos % 4, 0xFF, np.uint8))
            pos += 4 - pos % 4
    block = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    if padded:
        return block, np.array(off, np.int64), np.array(lens, np.int32)
    return block, np.array(off + [pos], np.int64), None


def all_logged_columns(n):
    """record columns under which every record is logged"""
    i = np.arange(n, dtype=np.int32)
    return dict(gidx=i * 3 + 1, slot=i - 7, bnum=i % 5, bcoord=100 + i % 3,
                r_flags=np.where(i % 2 == 1, M.R_TOLOG | M.R_STORED, M.R_TOLOG).astype(np.uint8), status=np.zeros(n, np.uint8))


def phase_lengths():
    """2,000 lengths: 0 .. 40 in turn, then random in [0, 300]: an entry starts at every offset modulo 16 and a prefix
    straddles a 16-byte chunk in each of its three ways"""
    rng = np.random.default_rng(3)
    return [i % 41 if i < 410 else int(rng.integers(0, 301)) for i in range(2000)]


def selection_case():
    """every status x flag bits x frame validity -> (block, frame_off, frame_len, rec_frame, columns)"""
    block, off, ln = frames_of_lengths([10 + i for i in range(40)], seed=4, padded=True)
    off, ln = off.copy(), ln.copy()
    off[30] = -4                                    # a negative start
    ln[31] = -1                                     # a negative length
    ln[39] = block.shape[0] - int(off[39]) + 1      # ends one byte past frames_bytes
    ln[33] = 2 ** 31 - 1 - 3                        # INT32_MAX - 3: above the largest length
    frs = [3, -1, 40, 30, 31, 39, 33, 7, 3]
    rec_frame, status, r_flags = [], [], []
    for st in (M.S_OK, M.S_WINDOW, M.S_NOGROUP):
        for fl in (0, M.R_TOLOG, M.R_STORED, M.R_TOLOG | M.R_STORED):
            for f in frs:
                rec_frame.append(f), status.append(st), r_flags.append(fl)
    n = len(status)
    i = np.arange(n, dtype=np.int32)
    cols = dict(gidx=i, slot=2 * i, bnum=3 * i, bcoord=-i, r_flags=np.array(r_flags, np.uint8), status=np.array(status, np.uint8))
    return block, off, ln, np.array(rec_frame, np.int32), cols


# ---- the _dev call inside guard bands (GPU) ----------------------------------------------------------------------------
class Guarded:
    """One device byte buffer that holds every buffer of a call, each between two bands of GUARD bytes.  The bands of an
    output hold SENTINEL; the bands around the frame block hold live, plausible bytes (a copy of the block's own bytes,
    shifted): a wrong offset reads wrong data and fails the comparison instead of leaving allocated memory."""

    def __init__(self):
        self.parts, self.pos, self.at = [], 0, {}

    def put(self, name, body, live=False, misalign=0):
        body = np.ascontiguousarray(body).view(np.uint8).reshape(-1)
        if live and body.shape[0]:
            band = np.resize(np.roll(body, 5), GUARD)
        else:
            band = np.full(GUARD, SENTINEL if not live else 0x3C, np.uint8)
        front = np.concatenate([band, band[:misalign]])
        self.parts += [front, body, band]
        self.at[name] = (self.pos + front.shape[0], body.shape[0])
        self.pos += front.shape[0] + body.shape[0] + GUARD
        pad = (-self.pos) % 16
        self.parts.append(np.full(pad, SENTINEL, np.uint8))
        self.pos += pad

    def upload(self):
        import torch
        self.image = np.concatenate(self.parts)
        self.buf = torch.from_numpy(self.image).cuda()
        torch.cuda.synchronize()
        assert self.buf.data_ptr() % 16 == 0
        return self

    def ptr(self, name):
        return self.buf.data_ptr() + self.at[name][0] if name in self.at else 0

    def download(self):
        self.after = self.buf.cpu().numpy()
        return self

    def get(self, name, dtype=np.uint8):
        o, n = self.at[name]
        return self.after[o:o + n].copy().view(dtype)

    def unchanged_outside(self, written):
        """every byte outside the named (offset, count) ranges of the outputs is what was uploaded"""
        keep = np.ones(self.image.shape[0], bool)
        for name, count in written.items():
            o, _ = self.at[name]
            keep[o:o + count] = False
        bad = np.nonzero((self.image != self.after) & keep)[0]
        assert bad.shape[0] == 0, "bytes changed outside the outputs, the first at %d of %s" % (int(bad[0]), self.at)


ROW_DT = dict(rec=np.int32, gidx=np.int32, slot=np.int32, bnum=np.int32, bcoord=np.int32, off=np.int64, len=np.int32)


def pack_dev(e, block, frame_off, cols, frame_len=None, rec_frame=None, base_offset=0, flags=0, cap_bytes=None,
             cap_entries=None, misalign=0, null_rows=(), what=""):
    """gpx_journal_pack_dev on guarded buffers, compared with the model: counts, bytes, rows, and every byte outside what
    the model says was written -> the model's answer"""
    from gigapaxos_amd import journal as J
    n = cols["status"].shape[0]
    want_all = M.pack(block, frame_off, cols["gidx"], cols["slot"], cols["bnum"], cols["bcoord"], cols["r_flags"],
                      cols["status"], frame_len, rec_frame)
    count_only = bool(flags & M.COUNT_ONLY)
    cb = want_all.counts["n_bytes"] if cap_bytes is None else cap_bytes
    ce = n if cap_entries is None else cap_entries
    want = M.pack(block, frame_off, cols["gidx"], cols["slot"], cols["bnum"], cols["bcoord"], cols["r_flags"],
                  cols["status"], frame_len, rec_frame, base_offset, flags, cb, ce)
    A = Guarded()
    A.put("frames", block, live=True, misalign=misalign)
    A.put("frame_off", frame_off.astype(np.int64), live=True)
    if frame_len is not None:
        A.put("frame_len", frame_len.astype(np.int32), live=True)
    if rec_frame is not None:
        A.put("rec_frame", rec_frame.astype(np.int32), live=True)
    for k in ("gidx", "slot", "bnum", "bcoord"):
        A.put(k, cols[k].astype(np.int32), live=True)
    for k in ("r_flags", "status"):
        A.put(k, cols[k].astype(np.uint8), live=True)
    if not count_only:
        A.put("out", np.full(cb, SENTINEL, np.uint8))
        for k, dt in ROW_DT.items():
            if k not in null_rows:
                A.put("e_" + k, np.full(ce * np.dtype(dt).itemsize, SENTINEL, np.uint8))
    A.put("counts", np.full(32, SENTINEL, np.uint8))
    A.upload()
    n_frames = frame_off.shape[0] - (1 if frame_len is None else 0)
    J.journal_pack_dev(e, n, A.ptr("frames"), block.shape[0], n_frames, A.ptr("frame_off"), A.ptr("frame_len"),
                       A.ptr("rec_frame"), [A.ptr(k) for k in ("gidx", "slot", "bnum", "bcoord")], A.ptr("r_flags"),
                       A.ptr("status"), base_offset, flags, A.ptr("out"), cb, ce, [A.ptr("e_" + k) for k in ROW_DT],
                       A.ptr("counts"))
    e.sync()
    A.download()
    counts = J.JournalCounts.from_buffer_copy(A.get("counts").tobytes())
    assert M.counts_of(counts) == want.counts, (what, M.counts_of(counts), want.counts)
    written = {"counts": 32}
    if not count_only:
        assert A.get("out")[:counts.bytes_done].tobytes() == want.bytes, what + ": journal bytes"
        written["out"] = counts.bytes_done
        for k, dt in ROW_DT.items():
            if k not in null_rows:
                assert A.get("e_" + k, dt)[:counts.n_done].tolist() == want.rows[k].tolist(), what + ": row column " + k
                written["e_" + k] = counts.n_done * np.dtype(dt).itemsize
    A.unchanged_outside(written)
    return want
