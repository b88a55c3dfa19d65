"""Columns at chosen addresses inside guarded arenas: the drivers of tests/test_placement_gpu.py (engine against
oracle) and tests/test_placement_model.py (the same arenas over numpy bytes, oracle against oracle, on the CPU).

Every kernel that reads a caller's column with 16-byte loads has a second form for columns that are not 16-byte aligned
and a third for the last few records of a batch; which one runs is decided by the low bits of the caller's pointers
and by n mod 4 or n mod 8.  Torch allocations are aligned to 256 bytes and have nothing next to them that a test looks
at, so here ONE byte buffer per call holds every input and output column of the call, each at a byte offset modulo 16
that the PLACEMENT names, each between two guard bands of GUARD bytes:

  output columns  the bands (and the columns, before the call) hold SENTINEL.  After the call every byte outside the n
                  entries of an output column is what it was: a store that runs past a column damages a sentinel, or,
                  under `packed`, the head of the next output, which the comparison with the oracle sees.
  input columns   the bands hold live POISON: records that are valid for this call and change its answer if applied.
                  The P records behind a column start with one for the group of record n - 1, the band in front ends
                  with one for the group of record 0 (what an unguarded gidx[i + 1] / gidx[i - 1] takes for the same
                  run); in a batch that is grouped by group the poison keeps the column non-decreasing, so that it would
                  be applied and not refused.  After the call every input column and both its bands are byte-identical
                  to what was uploaded.

The bands are as wide as they are so that a kernel which reads or writes a few vectors too far stays inside the test's
own allocation: a defect makes a comparison fail.  Nothing here sits at the end of an allocation or of a page."""
import ctypes as C

import numpy as np

from gigapaxos_amd._abi import Decisions, ExecRuns
from tests.lifetime_common import DevEngine

GUARD = 4096
P = 16
SENTINEL = 0xA5

# name -> byte offsets modulo 16 of (int32 inputs, byte inputs, int32 outputs, byte outputs and status); `packed`: the
# columns back to back, 4 n bytes each, the byte columns directly behind, guards around the whole run only
PLACEMENTS = {
    "aligned": (0, 0, 0, 0),
    "all+4": (4, 1, 4, 1),
    "in+8/out+12": (8, 2, 12, 3),
    "in+12/out+4": (12, 3, 4, 5),
    "packed": None,
    "only-gidx": (0, 0, 0, 0),      # ... and gidx at +4
    "only-bytes": (0, 1, 0, 1),
    "only-outputs": (0, 0, 4, 7),
}
NAMES = list(PLACEMENTS)
MOVES_INPUT = {"all+4", "in+8/out+12", "in+12/out+4", "packed", "only-gidx", "only-bytes"}   # (packed: whenever n % 4)
MOVES_INT_INPUT = {"all+4", "in+8/out+12", "in+12/out+4", "only-gidx"}                        # at every n

# entry point -> (C function, input columns, output columns); a column: (name, bytes per entry); the count word has
# one entry.  The C call takes n, the inputs in this order, then the outputs in this order.
OPS = {
    "propose": ("propose_batch", [("gidx", 4), ("is_stop", 1)],
                [("slot", 4), ("bnum", 4), ("bcoord", 4), ("median_cp", 4), ("status", 1)]),
    "accept": ("accept_batch", [("gidx", 4), ("bnum", 4), ("bcoord", 4), ("slot", 4), ("median_cp", 4), ("a_flags", 1)],
               [("r_bnum", 4), ("r_bcoord", 4), ("r_maxcp", 4), ("r_flags", 1), ("status", 1), ("x_gidx", 4), ("x_first", 4),
                ("x_count", 4), ("n_runs", 4)]),
    "commit": ("commit_batch", [("gidx", 4), ("bnum", 4), ("bcoord", 4), ("slot", 4), ("median_cp", 4), ("c_kind", 1)],
               [("status", 1), ("x_gidx", 4), ("x_first", 4), ("x_count", 4), ("n_runs", 4)]),
    "accept_reply": ("accept_reply_batch",
                     [("gidx", 4), ("bnum", 4), ("bcoord", 4), ("slot", 4), ("acceptor", 4), ("max_cp", 4)],
                     [("d_gidx", 4), ("d_slot", 4), ("d_bnum", 4), ("d_bcoord", 4), ("d_median_cp", 4), ("d_kind", 1),
                      ("n_out", 4), ("status", 1)]),
}
COUNT_WORDS = {"n_runs", "n_out"}
ENTRY_POINTS = tuple(OPS)


# ---- the poison ----------------------------------------------------------------------------------------------------------
def is_grouped(g):
    return g.shape[0] > 0 and bool((np.diff(g.astype(np.int64)) >= 0).all())


def poison(op, cols, gmax=None):
    """(front, behind): per input column of `cols` (gidx first; None: a NULL column) P records for the band in front of
    the column and P for the band behind it.

    A batch grouped by group (non-decreasing gidx; judged over the last and over the first 2 P records on their own, so
    that the acceptors' ascending runs count at both ends) gets non-decreasing poison: behind, the group of record n - 1 and -
    where the caller names the table's last group, gmax - the groups after it, two records each; in front the same
    mirrored, ending with the group of record 0.  Any other batch gets the groups of records n - 1, n - 8, n - 15, ...
    behind and of ..., 14, 7, 0 in front.  A poison record copies the record it is derived from and then differs the
    way a later message of the same exchange would: an accept reply comes from the next member (a vote that has not
    been cast: with one vote per group in the batch it completes the majority), an ACCEPT / COMMIT is for the next
    slot(s) of its group, a proposal is a further request for the group."""
    g = cols[0]
    n = g.shape[0]
    j = np.arange(P)
    if n == 0:
        z = [None if c is None else np.zeros(P, c.dtype) for c in cols]
        return z, [None if c is None else x.copy() for c, x in zip(cols, z)]
    # grouped is judged at either end of the batch on its own (the acceptors' ascending runs: the last run goes on)
    if is_grouped(g[-2 * P:]):
        src_b, gb = np.full(P, n - 1), np.full(P, g[n - 1], np.int64)
        if gmax is not None and 0 <= g[n - 1] <= gmax:
            gb = np.minimum(gb + (j + 1) // 2, gmax)
    else:
        src_b = (n - 1 - 7 * j) % n
        gb = g[src_b].astype(np.int64)
    if is_grouped(g[:2 * P]):
        src_f, gf = np.zeros(P, np.int64), np.full(P, g[0], np.int64)
        if gmax is not None and 0 <= g[0] <= gmax:
            gf = np.maximum(gf - (P - j) // 2, 0)
    else:
        src_f = (7 * (P - 1 - j)) % n
        gf = g[src_f].astype(np.int64)
    out = []
    for src, grp, order in ((src_f, gf, j[::-1]), (src_b, gb, j)):   # `order`: nearest to the column first
        band = [None if c is None else c[src].copy() for c in cols]
        band[0] = grp.astype(np.int32)
        seen = {}
        for i in order:
            k = seen.get(int(grp[i]), 0)
            seen[int(grp[i])] = k + 1
            same = int(grp[i]) == int(g[src[i]])
            if op in ("accept", "commit"):
                band[3][i] = (int(band[3][i]) + k + (1 if same else 0) + 2 ** 31) % 2 ** 32 - 2 ** 31   # (Java int)
            elif op == "accept_reply":
                band[4][i] = 100 + (int(band[4][i]) - 100 + 1 + k) % 3
        out.append(band)
    return out[0], out[1]


def extended(cols, front, behind, with_front=False):
    """The n + P records a call would see if it ran past its last record (with_front: if it began P records early)."""
    parts = [front, cols] if with_front else [cols, behind]
    return [None if cols[i] is None else np.concatenate([p[i] for p in parts]) for i in range(len(cols))]


# ---- the arena -----------------------------------------------------------------------------------------------------------
class Column:
    def __init__(self, name, width, n, out, body=None, front=None, behind=None):
        self.name, self.width, self.n, self.out = name, width, n, out
        self.body, self.front, self.behind = body, front, behind
        self.off = None   # byte offset of entry 0 in the arena (None: NULL)

    @property
    def nbytes(self):
        return self.n * self.width

    def dtype(self):
        return np.int32 if self.width == 4 else np.uint8


def _band(col, nbytes, front):
    """Guard bytes next to `col`: sentinels for an output; for an input its P poison records against the column and the
    outermost of them repeated to the band's far end."""
    if col.out:
        return np.full(nbytes, SENTINEL, np.uint8)
    cnt = nbytes // col.width
    assert cnt * col.width == nbytes and cnt >= P
    rec = col.front if front else col.behind
    fill = np.full(cnt - P, rec[0] if front else rec[-1], col.dtype())
    a = np.concatenate([fill, rec] if front else [rec, fill]).astype(col.dtype())
    return a.view(np.uint8)


def _body(col):
    if col.out:
        return np.full(col.nbytes, SENTINEL, np.uint8)
    return np.ascontiguousarray(col.body, col.dtype()).view(np.uint8)


def offsets_of(placement, col, status_at=None):
    o = PLACEMENTS[placement]
    if col.name == "status" and status_at is not None:
        return status_at
    if placement == "only-gidx" and col.name == "gidx":
        return 4
    return o[(2 if col.out else 0) + (1 if col.width == 1 else 0)]


def lay_out(placement, columns, status_at=None):
    """Lays `columns` (inputs first) out under `placement`; sets every column's `off` and returns the arena's initial
    image (uint8).  The image starts and every band ends on a 16-byte boundary of the arena."""
    chunks, pos = [], 0

    def put(a):
        nonlocal pos
        chunks.append(a)
        pos += a.shape[0]

    def pad16(col):
        if pos % 16:
            k = 16 - pos % 16
            put(_band(col, k, False)[:k] if col.out else np.zeros(k, np.uint8))
    live = [c for c in columns if c is not None]
    if placement == "packed":
        for out in (False, True):
            run = [c for c in live if c.out == out]
            run = [c for c in run if c.width == 4] + [c for c in run if c.width == 1]
            if not run:
                continue
            put(_band(run[0], GUARD, True))
            for c in run:
                c.off = pos
                put(_body(c))
            # the band behind continues the LAST column; an int32 band starts where the int32 columns end (4-aligned)
            put(_band(run[-1], GUARD, False))
            pad16(run[-1])
    else:
        for c in live:
            off = offsets_of(placement, c, status_at)
            assert off % c.width == 0 and pos % 16 == 0
            put(_band(c, GUARD + off, True))
            c.off = pos
            assert c.off % 16 == off
            put(_body(c))
            put(_band(c, GUARD, False))
            pad16(c)
    return np.concatenate(chunks)


def verify(image, after, columns, what):
    """Every byte outside the output columns' n entries is what was uploaded: sentinels intact, inputs and poison
    untouched."""
    assert image.shape == after.shape
    keep = np.ones(image.shape[0], bool)
    for c in columns:
        if c is not None and c.out:
            keep[c.off:c.off + c.nbytes] = False
    bad = np.nonzero((image != after) & keep)[0]
    if bad.shape[0]:
        b = int(bad[0])
        near = min((c for c in columns if c is not None), key=lambda c: min(abs(b - c.off), abs(b - (c.off + c.nbytes))))
        side = "in front of" if b < near.off else ("behind" if b >= near.off + near.nbytes else "inside")
        raise AssertionError(f"{what}: {bad.shape[0]} byte(s) changed outside the outputs, the first {side} "
                             f"{'output' if near.out else 'input'} column {near.name} (arena byte {b}, column at "
                             f"{near.off}..{near.off + near.nbytes}): {int(image[b]):#x} -> {int(after[b]):#x}")


def aligned_bytes(nbytes):
    """A zeroed numpy byte array that starts on a 16-byte boundary."""
    raw = np.zeros(nbytes + 16, np.uint8)
    s = (-raw.ctypes.data) % 16
    return raw[s:s + nbytes]


class Placer:
    """Turns the host calls' signatures into calls on placed columns.  A subclass runs the call: _run(fn, n, image,
    columns) -> the arena's bytes after the call.  Each call takes the next placement of its entry point (that entry
    point's own call counter); `fixed` pins one, `status_at` moves the status column alone, `null_status` drops it, `gmax` lets the poison of
    grouped batches walk on to the groups behind the batch."""

    def _init_placer(self):
        self.count = {op: 0 for op in OPS}
        self.log = []          # per call: dict(op, n, placement, kernels)
        self.fixed = None
        self.status_at = None
        self.null_status = False   # accept replies without a status column, whatever the driver asks for
        self.gmax = None
        self.last = None       # (op, input columns, front, behind) of the most recent call

    def _placed(self, op, cols, null_outputs=()):
        fn, ins, outs = OPS[op]
        n = int(cols[0].shape[0])
        placement = self.fixed or NAMES[self.count[op] % len(NAMES)]
        self.count[op] += 1
        arrays = [None if c is None else np.ascontiguousarray(c, np.int32 if w == 4 else np.uint8)
                  for c, (_, w) in zip(cols, ins)]
        front, behind = poison(op, arrays, self.gmax)
        self.last = (op, arrays, front, behind)
        columns = [None if a is None else Column(nm, w, n, False, a, f, b)
                   for (nm, w), a, f, b in zip(ins, arrays, front, behind)]
        columns += [None if nm in null_outputs else Column(nm, w, 1 if nm in COUNT_WORDS else n, True) for nm, w in outs]
        image = lay_out(placement, columns, self.status_at)
        what = f"{op} call {self.count[op]} of {n} records, placement {placement}"
        after, kernels = self._run(fn, n, image, columns)
        verify(image, after, columns, what)
        self.log.append(dict(op=op, n=n, placement=placement, kernels=kernels))
        res = {}
        for c in columns[len(ins):]:
            if c is not None:
                res[c.name] = after[c.off:c.off + c.nbytes].copy().view(c.dtype())
        return n, res

    @staticmethod
    def _flags(col, n):
        return np.zeros(n, np.uint8) if col is None else col

    def propose(self, g, is_stop=None):
        n, r = self._placed("propose", [np.ascontiguousarray(g, np.int32), is_stop])
        return r["slot"], r["bnum"], r["bcoord"], r["median_cp"], r["status"]

    def accept(self, g, bnum, bcoord, slot, median, a_flags=None):
        g = np.ascontiguousarray(g, np.int32)
        n, r = self._placed("accept", [g, bnum, bcoord, slot, median, self._flags(a_flags, g.shape[0])])
        m = int(r["n_runs"][0])
        return ((r["r_bnum"], r["r_bcoord"], r["r_maxcp"], r["r_flags"], r["status"]),
                ExecRuns(r["x_gidx"][:m], r["x_first"][:m], r["x_count"][:m]))

    def commit(self, g, bnum, bcoord, slot, median, c_kind=None):
        g = np.ascontiguousarray(g, np.int32)
        n, r = self._placed("commit", [g, bnum, bcoord, slot, median, self._flags(c_kind, g.shape[0])])
        m = int(r["n_runs"][0])
        return r["status"], ExecRuns(r["x_gidx"][:m], r["x_first"][:m], r["x_count"][:m])

    def accept_reply(self, g, bnum, bcoord, slot, acceptor, max_cp, unaligned=False, status=True):
        """status None or False: a NULL status column (the answer's status is then None)."""
        g = np.ascontiguousarray(g, np.int32)
        n, r = self._placed("accept_reply", [g, bnum, bcoord, slot, acceptor, max_cp], () if status and not self.null_status else ("status",))
        m = int(r["n_out"][0])
        return Decisions(r["d_gidx"][:m], r["d_slot"][:m], r["d_bnum"][:m], r["d_bcoord"][:m], r["d_median_cp"][:m],
                         r["d_kind"][:m], r.get("status"))


# ---- the view change's entry points (gpx_election_begin, gpx_prepare_reply_batch) ------------------------------------------
# Their columns do not all have n entries: pv_off has n + 1, the five pvalue columns pv_off[n], the four list outputs
# `window` planes of n entries each (entry j of record i at [j * n + i]); pv_handle and e_handle are 64-bit.
ELECT_OPS = {
    "election_begin": ("election_begin", [("gidx", 4), ("bnum", 4)], [("e_status", 1)]),
    "prepare_reply": ("prepare_reply_batch",
                      [("gidx", 4), ("acceptor", 4), ("r_bnum", 4), ("r_bcoord", 4), ("first_slot", 4), ("pv_off", 4), ("pv_slot", 4),
                       ("pv_bnum", 4), ("pv_bcoord", 4), ("pv_handle", 8), ("pv_flags", 1)],
                      [("v_kind", 1), ("e_count", 4), ("e_median", 4), ("e_slot", 4), ("e_kind", 1), ("e_handle", 8), ("e_flags", 1),
                       ("status", 1)]),
}
ELECT_PLANES = ("e_slot", "e_kind", "e_handle", "e_flags")
ELECT_ENTRY_POINTS = tuple(ELECT_OPS)


class WideColumn(Column):
    """A column of 1-, 4- or 8-byte entries."""

    def dtype(self):
        return {1: np.uint8, 4: np.int32, 8: np.int64}[self.width]


def elect_poison(op, arrays):
    """(front, behind) for the view change's input columns.  Behind the record columns: further replies - record
    n - 1 - 7 j with the acceptor of the record after it (in most cases a member that has not answered yet: the reply
    would count) - with empty slices (pv_off goes on at pv_off[n]); in front the same from record 0 on.  Around the
    pvalue columns: the column's own entries again, one ballot number higher, other handles, the stop flag set - a slice
    read too far carries them over in place of what the group accepted."""
    n = arrays[0].shape[0]
    j = np.arange(P)
    src_b, src_f = (n - 1 - 7 * j) % n, (7 * (P - 1 - j)) % n
    front, behind = [], []
    names = [nm for nm, _ in ELECT_OPS[op][1]]
    for nm, a in zip(names, arrays):
        if nm == "pv_off":
            front.append(np.zeros(P, np.int32)), behind.append(np.full(P, a[-1], np.int32))
        elif nm.startswith("pv_"):
            m = a.shape[0]
            f, b = a[(np.arange(P) - P) % m].copy(), a[np.arange(P) % m].copy()
            for x in (f, b):
                if nm == "pv_bnum":
                    x += 1
                elif nm == "pv_handle":
                    x += 7
                elif nm == "pv_flags":
                    x |= 1
            front.append(f), behind.append(b)
        elif nm == "acceptor":
            front.append(a[(src_f + 1) % n].copy()), behind.append(a[(src_b + 1) % n].copy())
        else:
            front.append(a[src_f].copy()), behind.append(a[src_b].copy())
    return front, behind


def lay_out_wide(placement, columns):
    """lay_out for columns of several lengths and widths: an 8-byte column takes its placement's offset rounded down to
    a multiple of 8; under `packed` the 8-byte columns come first, then the 4-byte ones, then the bytes."""
    chunks, pos = [], 0

    def put(a):
        nonlocal pos
        chunks.append(a)
        pos += a.shape[0]

    def pad16(col):
        if pos % 16:
            k = 16 - pos % 16
            put(np.full(k, SENTINEL, np.uint8) if col.out else np.zeros(k, np.uint8))
    if placement == "packed":
        for out in (False, True):
            run = sorted([c for c in columns if c.out == out], key=lambda c: -c.width)
            put(_band(run[0], GUARD, True))
            for c in run:
                c.off = pos
                put(_body(c))
            put(_band(run[-1], GUARD, False))
            pad16(run[-1])
    else:
        for c in columns:
            off = offsets_of(placement, c)
            off -= off % c.width
            assert pos % 16 == 0
            put(_band(c, GUARD + off, True))
            c.off = pos
            assert c.off % 16 == off and c.off % c.width == 0
            put(_body(c))
            put(_band(c, GUARD, False))
            pad16(c)
    return np.concatenate(chunks)


def elect_counts(log):
    """{(entry point, placement): calls} of the view change's calls in a driver's log."""
    out = {(op, p): 0 for op in ELECT_OPS for p in NAMES}
    for x in log:
        if x["op"] in ELECT_OPS:
            out[(x["op"], x["placement"])] += 1
    return out


class ElectPlacer:
    """Placer's two further entry points (mixed into the placed engines below): every input column and each of the
    outputs - the four [window][n] planes among them - at its placement's offset inside one arena, between guard bands;
    after the call the planes j >= e_count[i] of every record i are exactly the sentinel."""

    def _placed_elect(self, op, arrays, W=1):
        fn, ins, outs = ELECT_OPS[op]
        n = int(arrays[0].shape[0])
        k = self.count.get(op, 0)
        placement = self.fixed or NAMES[k % len(NAMES)]
        self.count[op] = k + 1
        arrays = [np.ascontiguousarray(a, {1: np.uint8, 4: np.int32, 8: np.int64}[w]) for a, (_, w) in zip(arrays, ins)]
        front, behind = elect_poison(op, arrays)
        columns = [WideColumn(nm, w, a.shape[0], False, a, f, b) for (nm, w), a, f, b in zip(ins, arrays, front, behind)]
        columns += [WideColumn(nm, w, n * W if nm in ELECT_PLANES else n, True) for nm, w in outs]
        image = lay_out_wide(placement, columns)
        what = f"{op} call {k + 1} of {n} records, placement {placement}"
        after, kernels = self._run_elect(fn, n, image, columns)
        verify(image, after, columns, what)
        self.log.append(dict(op=op, n=n, placement=placement, kernels=kernels))
        res = {c.name: after[c.off:c.off + c.nbytes].copy().view(c.dtype()) for c in columns if c.out}
        if op == "prepare_reply":
            cnt = res["e_count"].astype(np.int64)
            assert (cnt >= 0).all() and (cnt <= W).all(), what
            untouched = np.arange(W)[:, None] >= cnt[None, :]
            for nm in ELECT_PLANES:
                raw = after[[c for c in columns if c.name == nm][0].off:][:res[nm].nbytes].reshape(W, n, -1)
                assert (raw[untouched] == SENTINEL).all(), f"{what}: {nm} written beyond e_count"
        return n, res

    def election_begin(self, gidx, bnum):
        g = np.ascontiguousarray(gidx, np.int32)
        _, r = self._placed_elect("election_begin", [g, np.array(np.broadcast_to(np.asarray(bnum, np.int32), g.shape))])
        return r["e_status"]

    def prepare_reply(self, gidx, acceptor, r_bnum, r_bcoord, first_slot, pvalues=None):
        from tests.elect_enum_common import flatten, answer
        g = np.ascontiguousarray(gidx, np.int32)
        n = g.shape[0]
        off, pv = flatten(pvalues if pvalues is not None else [[] for _ in range(n)])
        assert off[-1] > 0, "the placed call wants at least one pvalue in the batch"
        cols = [g] + [np.array(np.broadcast_to(np.asarray(x, np.int32), (n,))) for x in (acceptor, r_bnum, r_bcoord, first_slot)]
        _, r = self._placed_elect("prepare_reply", cols + [off] + list(pv), int(self.e.cfg.window))
        return answer(r, n)


class PlacedDevEngine(Placer, ElectPlacer, DevEngine):
    """A HIP engine behind the host calls' signatures, every data-path call through gpx_*_batch_dev on columns placed in
    one device byte buffer.  The count word is read after gpx_compact_last_dev, like DevEngine's; `raw` is what the call
    itself left there.  prepare stays on the host call."""

    def __init__(self, e):
        DevEngine.__init__(self, e)
        self._init_placer()

    def _run_elect(self, fn, n, image, columns):
        buf = self.t.from_numpy(image).cuda()
        base = buf.data_ptr()
        assert base % 16 == 0
        args = [C.c_void_p(base + c.off) for c in columns]
        if fn == "prepare_reply_batch":
            args.insert(6, int(columns[6].n))   # pv_total, behind pv_off: the entries of the pvalue columns
        self._begin()
        self.e.lib.check(self.e.lib.fn[fn + "_dev"](self.e.h, n, *args), fn + "_dev")
        self._finish(None)
        return buf.cpu().numpy(), self.kernels[-1]

    def _run(self, fn, n, image, columns):
        buf = self.t.from_numpy(image).cuda()
        base = buf.data_ptr()
        assert base % 16 == 0
        word = next((c for c in columns if c is not None and c.name in COUNT_WORDS), None)
        self._begin()
        self.e.call_dev(fn, n, *[0 if c is None else base + c.off for c in columns])
        self._finish(buf[word.off:word.off + 4].view(self.t.int32) if word is not None else None)
        return buf.cpu().numpy(), self.kernels[-1]


class PlacedHostEngine(Placer, ElectPlacer):
    """The same arenas over numpy bytes: a library's host-pointer calls (the oracle's) on placed columns."""

    def __init__(self, e):
        self.e, self.raw = e, None
        self._init_placer()

    def _run_elect(self, fn, n, image, columns):
        arena = aligned_bytes(image.shape[0])
        arena[:] = image
        args = [C.c_void_p(arena.ctypes.data + c.off) for c in columns]
        self.e.lib.check(self.e.lib.fn[fn](self.e.h, n, *args), fn)
        return arena, set()

    def __getattr__(self, name):
        return getattr(self.e, name)

    def _run(self, fn, n, image, columns):
        arena = aligned_bytes(image.shape[0])
        arena[:] = image
        base = arena.ctypes.data
        args = [None if c is None else C.c_void_p(base + c.off) for c in columns]
        self.e.lib.check(self.e.lib.fn[fn](self.e.h, n, *args), fn)
        return arena, set()


# ---- liveness of the poison: what the oracle answers when handed the bands as records ------------------------------------
COMPACTED = {"accept": ("x_gidx", ["x_gidx", "x_first", "x_count"], "n_runs"), "commit": ("x_gidx", ["x_gidx", "x_first", "x_count"], "n_runs"),
             "accept_reply": ("d_gidx", ["d_gidx", "d_slot", "d_bnum", "d_bcoord", "d_median_cp", "d_kind"], "n_out"),
             "propose": (None, [], None)}


def host_call(e, op, cols):
    """One host-pointer call on exact-size numpy columns -> {output column: array}."""
    fn, ins, outs = OPS[op]
    n = int(cols[0].shape[0])
    a = [None if c is None else np.ascontiguousarray(c, np.int32 if w == 4 else np.uint8) for c, (_, w) in zip(cols, ins)]
    res = {nm: np.zeros(1 if nm in COUNT_WORDS else max(n, 1), np.int32 if w == 4 else np.uint8) for nm, w in outs}
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    e.lib.check(e.lib.fn[fn](e.h, n, *[ptr(x) for x in a], *[ptr(res[nm]) for nm, _ in outs]), fn)
    return res


def signature(e, op, g, res, lo, n, groups, only=None):
    """What a call answered for its records lo .. lo+n-1 and left behind in `groups`: the per-record outputs, the compacted
    outputs, the counters and the groups' state dumps.  only: restricted to that group (its records, its compacted
    entries, its dump; no counters)."""
    key, comp, word = COMPACTED[op]
    sel = np.ones(n, bool) if only is None else g[lo:lo + n] == only
    sig = [res[nm][lo:lo + n][sel].tobytes() for nm, _ in OPS[op][2] if nm not in comp and nm not in COUNT_WORDS and nm in res]
    if word:
        m = int(res[word][0])
        rows = np.ones(m, bool) if only is None else res[key][:m] == only
        sig += [res[nm][:m][rows].tobytes() for nm in comp]
    if only is None:
        sig.append(e.counters())
    G = int(e.cfg.max_groups)
    sig.append([e.dump(int(x)).tolist() for x in ([only] if only is not None else groups) if 0 <= int(x) < G])
    return sig


def probe_groups(g, band):
    """The groups whose state a band's records would change: the band's own and those of records 0 and n - 1."""
    return np.unique(np.concatenate([band[0], g[:1], g[-1:]]))


def probe_ok(g, G):
    """Can the call stand for its entry point in the liveness check: records 0 and n - 1 name groups of the table."""
    return g.shape[0] > 0 and 0 <= g[0] < G and 0 <= g[-1] < G


PROBED = 24   # eligible calls per entry point whose signatures a Recorder keeps by default


class ProbeDone(Exception):
    def __init__(self, sig, tail_status):
        self.sig, self.tail_status = sig, tail_status   # (the status the poison records behind the batch got)


class Recorder(PlacedHostEngine):
    """PlacedHostEngine that keeps, per call that can stand for its entry point, the signatures the poison must change:
    sigs[(op, k)] = (whole call with the groups of the band behind, record 0's group, whole call with the groups of
    the band in front) for the k-th such call of op.  first_only: the first PROBED per op."""

    def __init__(self, e, first_only=True):
        PlacedHostEngine.__init__(self, e)
        self.sigs, self.first_only, self.seen_ok = {}, first_only, {op: 0 for op in OPS}

    def _placed(self, op, cols, null_outputs=()):
        n, res = PlacedHostEngine._placed(self, op, cols, null_outputs)
        _, arrays, front, behind = self.last
        g = arrays[0]
        if probe_ok(g, int(self.e.cfg.max_groups)):
            k = self.seen_ok[op]
            self.seen_ok[op] += 1
            if k < PROBED or not self.first_only:
                self.sigs[(op, k)] = (signature(self.e, op, g, res, 0, n, probe_groups(g, behind)),
                                      signature(self.e, op, g, res, 0, n, None, only=int(g[0])),
                                      signature(self.e, op, g, res, 0, n, probe_groups(g, front)))
        return n, res


class Probe:
    """A plain engine behind the host calls' signatures that hands the k-th eligible call of `op` its poison as records
    - behind the batch (side 'behind') or in front of it ('front': judged by the answer for the group of record 0;
    'front, whole call': by the whole call's) - and stops there with the signature."""

    def __init__(self, e, op, k, side, gmax=None):
        self.e, self.op, self.k, self.side, self.gmax = e, op, k, side, gmax
        self.seen_ok = 0

    def __getattr__(self, name):
        return getattr(self.e, name)

    def _call(self, op, cols, plain):
        arrays = [None if c is None else np.ascontiguousarray(c, np.int32 if w == 4 else np.uint8)
                  for c, (_, w) in zip(cols, OPS[op][1])]
        g = arrays[0]
        if op == self.op and probe_ok(g, int(self.e.cfg.max_groups)):
            self.seen_ok += 1
            if self.seen_ok - 1 == self.k:
                n = g.shape[0]
                front, behind = poison(op, arrays, self.gmax)
                ext = extended(arrays, front, behind, self.side != "behind")
                res = host_call(self.e, op, ext)
                if self.side == "front":   # the answer for the group of record 0
                    raise ProbeDone(signature(self.e, op, ext[0], res, P, n, None, only=int(g[0])), res["status"][:P])
                if self.side == "front, whole call":
                    raise ProbeDone(signature(self.e, op, ext[0], res, P, n, probe_groups(g, front)), res["status"][:P])
                raise ProbeDone(signature(self.e, op, ext[0], res, 0, n, probe_groups(g, behind)), res["status"][n:])
        return plain()

    def propose(self, g, is_stop=None):
        return self._call("propose", [np.ascontiguousarray(g, np.int32), is_stop], lambda: self.e.propose(g, is_stop))

    def accept(self, g, bnum, bcoord, slot, median, a_flags=None):
        fl = np.zeros(np.asarray(g).shape[0], np.uint8) if a_flags is None else a_flags
        return self._call("accept", [np.ascontiguousarray(g, np.int32), bnum, bcoord, slot, median, fl],
                          lambda: self.e.accept(g, bnum, bcoord, slot, median, a_flags))

    def commit(self, g, bnum, bcoord, slot, median, c_kind=None):
        fl = np.zeros(np.asarray(g).shape[0], np.uint8) if c_kind is None else c_kind
        return self._call("commit", [np.ascontiguousarray(g, np.int32), bnum, bcoord, slot, median, fl],
                          lambda: self.e.commit(g, bnum, bcoord, slot, median, c_kind))

    def accept_reply(self, g, bnum, bcoord, slot, acceptor, max_cp, unaligned=False, status=True):
        return self._call("accept_reply", [np.ascontiguousarray(g, np.int32), bnum, bcoord, slot, acceptor, max_cp],
                          lambda: self.e.accept_reply(g, bnum, bcoord, slot, acceptor, max_cp))


# ---- (a) the fuzz cells under placements -----------------------------------------------------------------------------------
# Steps of each cell of geometry_common.CELLS under PlacedDevEngine: the fewest (in tens) at which every entry point makes
# at least len(NAMES) calls, so that every (entry point, placement) pair occurs in every cell (test_placement_model.py
# asserts it with the cells' seeds: the fuzz draws the same stream whichever library answers).
PLACED_STEPS = {"partition-k3-w4": 60, "partition-k5-w8": 50, "partition-k8-w32": 60, "partition-k16-w8": 70, "tiles-k3-w8": 80,
                "tiles-k8-w4": 50, "runs-k5-w32": 70, "runs-k3-w4": 50, "big-accept-commit-k3-w8": 50, "wide-s11-w8": 60,
                "wide-s12-w4": 50}


def cell_counts(log):
    """{(entry point, placement): calls} of a driver's log."""
    out = {(op, p): 0 for op in OPS for p in NAMES}
    for x in log:
        out[(x["op"], x["placement"])] += 1
    return out


# ---- (b) tails at the kernels' own boundaries ----------------------------------------------------------------------------
MEMBERS = [100, 101, 102]
ONE_N = (1, 7, 8, 9, 2047, 2048, 2049, 2055)
ORDER_N = tuple(65_537 + r for r in (0, 6, 7, 8, 9))
RUNS_N = (4095, 4096, 4097, 8193)          # GPX_RC_ITEMS x GPX_OC_BLOCK = 4,096 records per workgroup of k_runs_check
TILE_N = tuple(8192 + r for r in (0, 1, 2, 3, 5)) + (4095,)
CASE_MAX_BATCH = 1 << 17
# kind -> (switches, groups, promise of the engine (the oracle's: without LAZY_OUTPUTS), sizes, kernels every data call ran)
LAZY = 32
PAC = 1 | 2 | 4
CASES = {
    "order": (dict(), 1100, 0, ORDER_N, dict(accept={"k_order_check", "k_scatter_ac16"}, commit={"k_order_check", "k_scatter_ac16"})),
    "one": (dict(GPX_XCHG_SLOTS=0), 4096, PAC | LAZY, ONE_N,
            dict(propose={"k_one_check", "k_propose_one"}, accept={"k_one_check", "k_ac_one"}, commit={"k_one_check", "k_ac_one"})),
    "pers": (dict(), 4096, PAC | LAZY, ONE_N, dict(propose={"k_propose_pers"}, accept={"k_ac_pers"}, commit={"k_ac_pers"})),
    "small": (dict(), 4096, 0, ONE_N, dict(accept={"k_ac_small"}, commit={"k_ac_small"})),
    "runs": (dict(GPX_XCHG_SLOTS=0, GPX_SAR_MAX_N=0), 4096, 8, RUNS_N, dict(accept_reply={"k_runs_check", "k_ar_runs"})),
    "tiles": (dict(GPX_TILE_T=4096, GPX_SAR_MAX_N=0), 2048, 0, TILE_N, dict(accept_reply={"k_scatter_tiles"})),
    "partition": (dict(GPX_AR_TILES=0, GPX_SAR_MAX_N=0), 2048, 0, TILE_N, dict(accept_reply={"k_hist", "k_scatter_ar16"})),
}
CASE_SWITCHES = ("GPX_XCHG_SLOTS", "GPX_SAR_MAX_N", "GPX_TILE_T", "GPX_TILE_NT", "GPX_AR_TILES", "GPX_TRY_RUNS", "GPX_BUCKET_SHIFT",
                 "GPX_PERS_CHUNKS")


def case_env(monkeypatch, kind):
    for v in CASE_SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for k, v in CASES[kind][0].items():
        monkeypatch.setenv(k, str(v))


def case_pair(lib_a, lib_b, kind):
    from tests.lifetime_common import make_ordered_pair
    _, G, mask, _, _ = CASES[kind]
    return make_ordered_pair(lib_a, lib_b, G, mask, mask & ~LAZY, max_batch=CASE_MAX_BATCH)


def case_engine(lib, kind, lazy=False):
    """One engine set up as case_pair's (the oracle for the liveness probes)."""
    from gigapaxos_amd import Engine, hri_create, S_OK
    _, G, mask, _, _ = CASES[kind]
    e = Engine(lib, 100, G, kmax=3, window=8, max_batch=CASE_MAX_BATCH)
    assert (e.create_groups(np.arange(G), np.tile(np.array(MEMBERS, np.int32), (G, 1)), 3, hri_create(G, 3, 100)) == S_OK).all()
    e.set_ordered_batches(mask if lazy else mask & ~LAZY)
    return e


def drive_case(kind, n, ea, eb):
    """The data calls of one directed case on engine a (placed, or a probe) and the oracle b, every answer compared.  In
    every call record 0 and record n - 1 belong to groups whose exchange the poison continues, with groups of the table
    on either side of the batch for a grouped batch's poison to walk to."""
    from gigapaxos_amd import C_HASVALUE
    from tests.lifetime_common import same_answer
    G = CASES[kind][1]
    what = f"{kind} n={n}"
    if kind == "order":
        # n records over 1,024 groups, grouped by group; the k-th record of a group is for slot 1 + k mod 8
        g = (8 + np.arange(n, dtype=np.int64) * 1024 // n).astype(np.int32)
        first = np.searchsorted(g, g)
        slot = (1 + (np.arange(n) - first) % 8).astype(np.int32)
        z, bc = np.zeros(n, np.int32), np.full(n, 100, np.int32)
        same_answer("accept", ea.accept(g, z, bc, slot, z), eb.accept(g, z, bc, slot, z), what + " ACCEPT")
        hv = np.full(n, C_HASVALUE, np.uint8)
        same_answer("commit", ea.commit(g, z, bc, slot, z, hv), eb.commit(g, z, bc, slot, z, hv), what + " COMMIT")
    elif kind in ("one", "pers", "small"):
        g = np.arange(8, 8 + n, dtype=np.int32)
        pa, pb = ea.propose(g), eb.propose(g)
        same_answer("propose", pa, pb, what + " PROPOSE")
        same_answer("accept", ea.accept(g, pb[1], pb[2], pb[0], pb[3]), eb.accept(g, pb[1], pb[2], pb[0], pb[3]), what + " ACCEPT")
        hv = np.full(n, C_HASVALUE, np.uint8)
        same_answer("commit", ea.commit(g, pb[1], pb[2], pb[0], pb[3], hv), eb.commit(g, pb[1], pb[2], pb[0], pb[3], hv),
                    what + " COMMIT")
    else:
        every = np.arange(G, dtype=np.int32)
        same_answer("propose", ea.propose(every), eb.propose(every), what + " PROPOSE")
        if kind == "runs":
            # three acceptors' replies, groups ascending in each; group 8 votes in the first run only, the last group of
            # the third run in that run only
            n1 = n2 = n // 3
            n3 = n - n1 - n2
            gi = np.concatenate([np.arange(8, 8 + n1), np.arange(9, 9 + n2), np.arange(29, 29 + n3)]).astype(np.int32)
            acc = np.repeat(np.array(MEMBERS, np.int32), [n1, n2, n3])
        else:
            # shuffled votes (duplicates among them); records 0 and n - 1 are the only votes of their groups
            rng = np.random.default_rng(n)
            gi = rng.integers(20, G - 40, n).astype(np.int32)
            acc = rng.choice(np.array(MEMBERS, np.int32), n)
            gi[0], acc[0], gi[-1], acc[-1] = 5, 100, G - 20, 102
        cols = [gi, np.zeros(n, np.int32), np.full(n, 100, np.int32), np.ones(n, np.int32), acc, np.zeros(n, np.int32)]
        da, db = ea.accept_reply(*cols), eb.accept_reply(*cols)
        assert da.as_tuple_array().tolist() == db.as_tuple_array().tolist(), what + " decisions"
        if da.status is not None:
            assert da.status.tolist() == db.status.tolist(), what + " status"
        assert db.gidx.shape[0] > 0, what
    from tests.lifetime_common import assert_same_rows
    assert_same_rows(ea, eb, G)
