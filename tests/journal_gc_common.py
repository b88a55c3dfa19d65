"""Shared pieces of the journal compaction tests (include/gpx_journal_gc.h): the group table and its GC slots, seeded
journal files with their index rows, the directed cases of tests/test_journal_gc_gpu.py (the CPU file asserts their
non-vacuity on the same seeds) and - for the GPU file - the _dev call on buffers inside guard bands."""
import numpy as np

from tests import journal_gc_model as GM
from tests import journal_model as M
from tests.journal_common import SENTINEL, Guarded

G, K, ME, CREATOR = 100, 3, 101, 100
MAX_V, MIN_V = 2 ** 31 - 1, -2 ** 31
SPECIAL_GC = (-1, 0, 5, MAX_V - 1, MIN_V)     # groups 0 .. 4 of the table
STOPPED, NEVER = 2, 7                         # group 2 (gc 5) is stopped by the GPU file; group 7 is never created


def table_gc():
    """acc_gc_slot of every group of the table: the five special ones, then seeded values on both sides of 0"""
    gc = np.random.default_rng(5).integers(-2 ** 26, 2 ** 26, G).astype(np.int64)
    gc[:len(SPECIAL_GC)] = SPECIAL_GC
    return gc


def table_exists():
    ex = np.ones(G, bool)
    ex[NEVER] = False
    return ex


def wrap(x):
    return ((np.asarray(x, np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)


class File:
    """a journal file under construction: <be32 len><bytes> entries and the index rows that name them"""

    def __init__(self, seed, in_base=0, a_gc=None):
        self.rng = np.random.default_rng(seed)
        self.in_base, self.a_gc = in_base, table_gc() if a_gc is None else a_gc
        self.parts, self.pos = [], 0
        self.gidx, self.slot, self.off, self.len = [], [], [], []

    def add(self, ln, keep, named=True, g=None):
        """one entry of ln bytes; keep decides its slot against its group's GC slot (groups that exist, not the stopped)"""
        ln = int(ln)
        body = self.rng.integers(1, 251, ln).astype(np.uint8)
        self.parts += [np.frombuffer(ln.to_bytes(4, "big"), np.uint8), body]
        at, self.pos = self.pos, self.pos + 4 + ln
        if not named:
            return
        if g is None:
            g = int(self.rng.integers(8, G))
        d = int(self.rng.integers(1, 17)) if keep else -int(self.rng.integers(0, 16))
        self.gidx.append(g), self.slot.append(int(wrap(int(self.a_gc[g]) + d))), self.off.append(self.in_base + at), self.len.append(ln)

    def done(self):
        n = len(self.len)
        i = np.arange(n, dtype=np.int32)
        return dict(data=np.concatenate(self.parts) if self.parts else np.zeros(0, np.uint8), in_bytes=self.pos, in_base=self.in_base,
                    e_gidx=np.array(self.gidx, np.int32), e_slot=np.array(self.slot, np.int32), e_off=np.array(self.off, np.int64),
                    e_len=np.array(self.len, np.int32), e_bnum=i % 7, e_bcoord=100 + i % 3, cp_slot=None)


def model(c, a_gc=None, exists=None, data=True, **kw):
    """tests/journal_gc_model.compact over a case dict"""
    return GM.compact(c["data"] if data else None, c["in_bytes"], c["in_base"], c["e_gidx"], c["e_slot"], c["e_off"], c["e_len"],
                      table_gc() if a_gc is None else a_gc, table_exists() if exists is None else exists, c["e_bnum"], c["e_bcoord"],
                      c["cp_slot"], **kw)


# ---- the directed cases --------------------------------------------------------------------------------------------------
CP_MODES = ("none", "above", "equal", "below", "wrapped")


def verdict_case(mode):
    """gc x slot around it and half the ring away, one cp_slot mode, the stopped group, group numbers that cannot be judged"""
    f = File(11, in_base=1000)
    cp = []
    dcp = dict(none=0, above=3, equal=0, below=-3, wrapped=2 ** 31)[mode]
    for q, gc in enumerate(SPECIAL_GC):
        for d in (-1, 0, 1, 2 ** 31 - 1, 2 ** 31, -4, -3, -2):
            f.add(3 + q, True, g=q)
            f.slot[-1] = int(wrap(gc + d))
            cp.append(int(wrap(gc + dcp)))
    for g in (-1, G, NEVER, MIN_V, MAX_V):
        f.add(9, False, g=8)
        f.gidx[-1] = g
        cp.append(0)
    c = f.done()
    if mode != "none":
        c["cp_slot"] = np.array(cp, np.int32)
    return c


def phase_case():
    """6,000 entries of 0 .. 40 bytes kept or dropped at random: a run head at every source phase x output phase"""
    f = File(32)
    for i in range(6000):
        f.add(i % 41 if i < 410 else int(f.rng.integers(0, 41)), bool(f.rng.integers(0, 2)))
    return f.done()


def phase_pairs(c, want):
    """{(source phase, output phase)} of the run heads of the model's answer"""
    src, pos, prev, seen = want.rows["src"], want.rows["off"], -2, set()
    for s, p in zip(src.tolist(), pos.tolist()):
        if s != prev + 1:
            seen.add((int(c["e_off"][s]) % 16, p % 16))
        prev = s
    return seen


RUN_LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 1, 190)


def runs_case():
    """runs of kept rows of the lengths that matter around the wave and the row tile, each behind dropped rows"""
    f = File(13)
    for rl in RUN_LENGTHS:
        for _ in range(rl):
            f.add(f.rng.integers(0, 50), True)
        for _ in range(1 + rl // 2):
            f.add(f.rng.integers(0, 50), False)
    return f.done()


def uniform_case(keep, n=700, seed=14, in_base=64):
    f = File(seed, in_base=in_base)
    for _ in range(n):
        f.add(f.rng.integers(0, 120), keep)
    return f.done()


def gaps_case():
    """everything kept, every 50th entry of the file named by no row"""
    f = File(15)
    for i in range(600):
        f.add(f.rng.integers(0, 60), True, named=i % 50 != 49)
    return f.done()


def swapped_case():
    """everything kept and adjacent, but rows 300 and 301 in each other's place"""
    c = uniform_case(True)
    for k in ("e_gidx", "e_slot", "e_off", "e_len", "e_bnum", "e_bcoord"):
        a = c[k].copy()
        a[[300, 301]] = a[[301, 300]]
        c[k] = a
    return c


def tile_edge_case(k, d):
    """kept bytes of 16384 k + d, dropped entries in between"""
    f = File(100 * k + d + 5)
    total, t = 16384 * k + d, 0
    while total - t > 400:
        ln = 97 + int(f.rng.integers(0, 50))
        f.add(ln, True)
        t += 4 + ln
        if f.rng.integers(0, 3) == 0:
            f.add(f.rng.integers(0, 30), False)
    rest = total - t
    f.add(rest // 2 - 4, True), f.add(rest - rest // 2 - 4, True), f.add(3, False)
    return f.done(), total


def tiny_case():
    """10,000 entries of 0 or 1 bytes, alternately kept: 5,000 runs, more than 256 in one 16 KB tile"""
    f = File(16)
    for i in range(10000):
        f.add(f.rng.integers(0, 2), bool(i & 1))
    return f.done()


def huge_case():
    f = File(17)
    for i in range(2001):
        f.add((1 << 20) + 13 if i == 1000 else f.rng.integers(0, 60), i == 1000 or f.rng.integers(0, 3) > 0)
    return f.done()


def refusal_case():
    """forty entries, nine rows spoilt -> (case, the rows a prefix test alone catches)"""
    f = File(18, in_base=500)
    for i in range(40):
        f.add(10 + i, i % 3 != 0)
    c = f.done()
    off, ln, data = c["e_off"].copy(), c["e_len"].copy(), c["data"].copy()
    off[5] = c["in_base"] - 1                       # a negative offset
    off[6] = -2 ** 63
    ln[7] = -1
    ln[8] = MAX_V - 3                               # above the largest length
    ln[39] += 1                                     # ends one byte past in_bytes
    data[int(off[20]) - c["in_base"] + 3] ^= 1      # a wrong prefix
    off[22] += 1                                    # a row that points into the middle of an entry
    off[23] = c["in_base"] + c["in_bytes"] - 3      # a prefix that would straddle the end
    off[24] = 2 ** 63 - 1
    c.update(e_off=off, e_len=ln, data=data)
    return c, (20, 22)


def caps_case():
    """1,400 entries, the first and every odd one kept -> (case, the ends of the kept entries in the output)"""
    f = File(19)
    ends = [0]
    for i in range(1400):
        ln, keep = (21 if i == 0 else int(f.rng.integers(0, 90))), (i == 0 or bool(i & 1))
        f.add(ln, keep)
        if keep:
            ends.append(ends[-1] + 4 + ln)
    return f.done(), ends


def big_case(n=70_000):
    f = File(20)
    for i in range(n):
        f.add(0 if i % 3 else 2, bool((i >> 1) & 1))
    return f.done()


def round_commits(groups=300):
    """the real round of the GPU file: the slots 1 .. k of group g that are executed before compaction, k = 4 .. 8, which
    is where the acceptor's GC slot then stands"""
    return (4 + np.arange(groups) % 5).astype(np.int32)


def round_logged(g, s, window=8):
    """which ACCEPTs of tests/journal_common.round_records an acceptor with an empty window of 8 logs: slots 1 .. 12
    arrive shuffled, and of two slots that share a ring position (1 and 9, .. 4 and 12) the one that arrives first is
    stored and logged, the other is refused with GPX_S_WINDOW"""
    seen, out = set(), np.zeros(len(g), bool)
    for i, (a, b) in enumerate(zip(g.tolist(), s.tolist())):
        if (a, b % window) not in seen:
            seen.add((a, b % window))
            out[i] = True
    return out


# ---- the _dev call inside guard bands (GPU) ----------------------------------------------------------------------------
ROW_DT = dict(src=np.int32, gidx=np.int32, slot=np.int32, bnum=np.int32, bcoord=np.int32, off=np.int64, len=np.int32)
IN_COLS = (("e_gidx", np.int32), ("e_slot", np.int32), ("e_off", np.int64), ("e_len", np.int32), ("e_bnum", np.int32),
           ("e_bcoord", np.int32), ("cp_slot", np.int32))


def gc_dev(e, c, a_gc, exists, out_base=0, flags=0, cap_bytes=None, cap_entries=None, null_cols=False, no_in=False, no_verdict=False,
           what=""):
    """gpx_journal_gc_dev on guarded buffers, compared with the model: counts, verdicts, bytes, rows, and every byte
    outside what the model says was written -> the model's answer.  `in` lies between live, plausible entries."""
    from gigapaxos_amd import journal_gc as J
    n = c["e_len"].shape[0]
    c = dict(c, e_bnum=None, e_bcoord=None) if null_cols else c
    whole = model(c, a_gc, exists, data=not no_in, flags=GM.COUNT_ONLY)      # keep_bytes describes the whole call
    count_only = bool(flags & GM.COUNT_ONLY)
    cb = whole.counts["keep_bytes"] if cap_bytes is None else cap_bytes
    ce = n if cap_entries is None else cap_entries
    want = model(c, a_gc, exists, data=not no_in, out_base=out_base, flags=flags, cap_bytes=cb, cap_entries=ce)
    A = Guarded()
    if not no_in:
        body = np.zeros((c["in_bytes"] + 15) // 16 * 16, np.uint8)     # the block ends at a 16-byte boundary
        body[:c["data"].shape[0]] = c["data"][:body.shape[0]]
        A.put("in", body, live=True)
    for k, dt in IN_COLS:
        if c[k] is not None:
            A.put(k, c[k].astype(dt), live=True)
    if not count_only:
        A.put("out", np.full(cb, SENTINEL, np.uint8))
        for k, dt in ROW_DT.items():
            if not (null_cols and k in ("src", "gidx", "slot", "bnum", "bcoord")):
                A.put("k_" + k, np.full(ce * np.dtype(dt).itemsize, SENTINEL, np.uint8))
    if not no_verdict:
        A.put("verdict", np.full(n, SENTINEL, np.uint8))
    A.put("counts", np.full(64, SENTINEL, np.uint8))
    A.upload()
    J.journal_gc_dev(e, n, A.ptr("in"), c["in_bytes"], c["in_base"], [A.ptr(k) for k, _ in IN_COLS], out_base, flags, A.ptr("out"),
                     cb, ce, A.ptr("verdict"), [A.ptr("k_" + k) for k in ROW_DT], A.ptr("counts"))
    e.sync()
    A.download()
    counts = J.JournalGcCounts.from_buffer_copy(A.get("counts").tobytes())
    assert GM.counts_of(counts) == want.counts, (what, GM.counts_of(counts), want.counts)
    written = {"counts": 64}
    if not no_verdict:
        assert A.get("verdict").tolist() == want.verdicts.tolist(), what + ": verdicts"
        written["verdict"] = n
    if not count_only:
        assert A.get("out")[:counts.bytes_done].tobytes() == want.bytes, what + ": journal bytes"
        written["out"] = counts.bytes_done
        for k, dt in ROW_DT.items():
            if "k_" + k in A.at:
                assert A.get("k_" + k, dt)[:counts.n_done].tolist() == want.rows[k].tolist(), what + ": row column " + k
                written["k_" + k] = counts.n_done * np.dtype(dt).itemsize
    A.unchanged_outside(written)
    return want


def survivors_through_pack(c, want):
    """the kept entries fed to the journal pack's model as frames (the detour of the parent commit): its bytes"""
    s = want.rows["src"].astype(np.int64)
    k = s.shape[0]
    rel = c["e_off"][s] - c["in_base"] + 4
    z = np.zeros(k, np.int32)
    return M.pack(c["data"], rel, z, z, z, z, np.full(k, M.R_TOLOG, np.uint8), np.zeros(k, np.uint8), frame_len=c["e_len"][s]).bytes
