"""numpy restatement of include/gpx_packed.h: the reading of a packed vote batch (unpack) and the packer's rule
(pack), written from the header's text and independent of the library's code.  Also the vote batches the packed
tests share."""
import numpy as np

EXC_BIT = np.uint32(0x80000000)
RESERVED = np.uint32(0x7F000000)
M32 = 0xFFFFFFFF


def _i32(x):
    return (np.asarray(x, np.int64) & M32).astype(np.uint32).view(np.int32)


def pack(cols):
    """-> (header dict, rec uint32 [n, 2], exc int32 [needed, 8]); header['n_exc'] == needed (no capacity here)."""
    gidx, bnum, bcoord, slot, acceptor, max_cp = (np.asarray(c, np.int32) for c in cols)
    n = gidx.shape[0]
    # Boyer-Moore majority candidate of the ballots, in order
    cand, cnt = (0, 0), 0
    for b in zip(bnum.tolist(), bcoord.tolist()):
        if cnt == 0:
            cand, cnt = b, 1
        elif b == cand:
            cnt += 1
        else:
            cnt -= 1
    same = (bnum == cand[0]) & (bcoord == cand[1])
    base = [0, 0, 0]
    if same.any():
        f = int(np.argmax(same))
        base = [(int(c[f]) - 128) & M32 for c in (slot, max_cp, acceptor)]
    d = [(c.astype(np.int64) - b) & M32 for c, b in zip((slot, max_cp, acceptor), base)]
    fits = same & (d[0] < 256) & (d[1] < 256) & (d[2] < 256)
    rec = np.zeros((n, 2), np.uint32)
    rec[:, 0] = gidx.view(np.uint32)
    rec[:, 1] = (d[0] | (d[1] << 8) | (d[2] << 16)).astype(np.uint32) * fits
    ex = np.nonzero(~fits)[0]
    rec[ex, 1] = EXC_BIT | np.arange(ex.shape[0], dtype=np.uint32)
    exc = np.zeros((ex.shape[0], 8), np.int32)
    for k, c in enumerate((bnum, bcoord, slot, acceptor, max_cp)):
        exc[:, k] = c[ex]
    hdr = dict(n=n, n_exc=int(ex.shape[0]), bnum=int(cand[0]), bcoord=int(cand[1]),
               base_slot=int(_i32(base[0])), base_cp=int(_i32(base[1])), base_acceptor=int(_i32(base[2])))
    return hdr, rec, exc


def unpack(hdr, rec, exc):
    """-> the six int32 columns (gidx, bnum, bcoord, slot, acceptor, max_cp) in record order."""
    rec = np.asarray(rec, np.uint32).reshape(-1, 2)
    exc = np.asarray(exc, np.int32).reshape(-1, 8)
    n, n_exc = hdr["n"], hdr["n_exc"]
    assert rec.shape[0] == n and exc.shape[0] >= n_exc
    g, w = rec[:, 0], rec[:, 1]
    is_exc = (w & EXC_BIT) != 0
    r = (w & ~EXC_BIT).astype(np.int64)
    bad = np.where(is_exc, r >= n_exc, (w & RESERVED) != 0)
    rr = np.where(is_exc & ~bad, r, 0)
    row = exc[rr] if n_exc > 0 else np.zeros((n, 8), np.int32)
    w64 = w.astype(np.int64)
    delta = [_i32(np.full(n, hdr["bnum"])), _i32(np.full(n, hdr["bcoord"])),
             _i32((hdr["base_slot"] & M32) + (w64 & 255)),
             _i32((hdr["base_acceptor"] & M32) + ((w64 >> 16) & 255)),
             _i32((hdr["base_cp"] & M32) + ((w64 >> 8) & 255))]
    cols = [np.where(bad, np.int32(-1), g.view(np.int32)).astype(np.int32)]
    for k in range(5):
        cols.append(np.where(bad, 0, np.where(is_exc, row[:, k], delta[k])).astype(np.int32))
    return tuple(cols)


# ---- the shapes of batch every packed test goes through ----------------------------------------------------------
def wrap_batch(n, rng, around):
    """Slots and checkpoints within +-50 of `around` (Integer.MAX_VALUE / MIN_VALUE: the batch straddles the wrap)."""
    return (rng.integers(0, 1000, n).astype(np.int32), np.zeros(n, np.int32), np.full(n, 100, np.int32),
            _i32(around + rng.integers(-50, 50, n)), rng.choice([100, 101, 102], n).astype(np.int32),
            _i32(around - 1 + rng.integers(-50, 50, n)))


def far_nodes_batch(n, rng):
    """Node ids 2^20 apart: about one vote in six comes from a node outside the byte around the first vote's."""
    far = (rng.random(n) < 1 / 6) * rng.integers(1, 3, n)
    far[:1] = 0
    return (rng.integers(0, 1000, n).astype(np.int32), np.zeros(n, np.int32), np.full(n, 100, np.int32),
            np.full(n, 7, np.int32), ((1 << 20) * far + 5).astype(np.int32), np.full(n, 6, np.int32))


def odd_first_batch(n):
    """An odd FIRST vote (other ballot, far slot) in front of n - 1 ordinary ones."""
    g = np.arange(n, dtype=np.int32)
    cols = [g, np.zeros(n, np.int32), np.full(n, 100, np.int32), np.full(n, 5, np.int32),
            (100 + g % 3).astype(np.int32), np.full(n, 4, np.int32)]
    if n:
        cols[1][0], cols[2][0], cols[3][0] = 9, 101, 1 << 30
    return tuple(cols)


def own_slot_batch(n):
    """Every group at its own slot (slot = 10 * gidx): deltas over 255 become exceptions."""
    g = np.arange(n, dtype=np.int32)
    return (g, np.zeros(n, np.int32), np.full(n, 100, np.int32), (10 * g).astype(np.int32),
            (100 + g % 3).astype(np.int32), (10 * g - 1).astype(np.int32))


def malformed(rec, n_exc, rng, count):
    """A copy of `rec` with `count` records broken (reserved bits / row index >= n_exc alternately); -> (rec, indices)."""
    rec = np.array(rec, np.uint32).reshape(-1, 2).copy()
    idx = np.sort(rng.choice(rec.shape[0], size=count, replace=False))
    for j, i in enumerate(idx):
        if j % 2 == 0:
            rec[i, 1] = (rec[i, 1] & ~EXC_BIT) | np.uint32(1 << (24 + j % 7))
        else:
            rec[i, 1] = EXC_BIT | np.uint32(n_exc + j)
    return rec, idx
