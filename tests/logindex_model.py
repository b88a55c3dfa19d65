"""The log index (include/gpx_logindex.h) twice: `JavaIndex`, a per-group, list-based restatement of
paxosutil/LogIndex.java in Java int arithmetic, and `FlatIndex`, a numpy model of the flat table with the calls' exact
outputs.  tests/test_logindex_model.py checks the two against each other; the GPU file checks the library bit for bit
against `FlatIndex`.  `CASES` is the directed case list both run: a case is a function of a back end `B` whose methods
are the seven calls (tests/logindex_common.py runs a case on the model and on another back end at once)."""
import numpy as np

ADDED, STALE, NOGROUP, FULL, REPEAT = 0, 1, 2, 3, 4
RESET = 1
MAX_FILES = 4096
COUNT_FIELDS = ("n_rows", "n_alive", "generation", "n_done", "n_hits", "n_stale", "n_nogroup", "n_repeat")
LOOKUP_COLS = ("rec", "row", "slot", "bnum", "bcoord", "file", "off", "len")
FILE_ROWS_COLS = ("row", "gidx", "slot", "bnum", "bcoord", "off", "len", "gc")
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def i32(x):
    """a Java int"""
    x = int(x) & 0xFFFFFFFF
    return x - (1 << 32) if x >= 1 << 31 else x


def diff(a, b):
    """a - b in Java int arithmetic"""
    return i32(int(a) - int(b))


def vdiff(a, b):
    """... over numpy columns"""
    d = (np.asarray(a, np.int64) - np.asarray(b, np.int64)) & 0xFFFFFFFF
    return np.where(d >= 1 << 31, d - (1 << 32), d)


# ---- the Java, restated -------------------------------------------------------------------------------------------------
class LogIndex:
    """paxosutil/LogIndex.java for ACCEPT entries: [slot, bnum, bcoord, file, offset, length] in arrival order"""

    def __init__(self):
        self.gc_slot, self.min_logfile, self.log = -1, None, []

    def add(self, slot, bnum, bcoord, file, off, ln):                      # :192-204
        if diff(slot, self.gc_slot) <= 0:
            return False
        if self.min_logfile is None:
            self.min_logfile = file
        self.log.append([slot, bnum, bcoord, file, off, ln])
        return True

    def set_gc_slot(self, gc):                                             # :128-152
        self.gc_slot = gc
        self.log = [e for e in self.log if not diff(e[0], self.gc_slot) <= 0]
        self.min_logfile = self.log[0][3] if self.log else None

    def get_logged_accepts(self, min_slot, max_slot):                      # :213-237
        return [e for e in self.log if diff(e[0], min_slot) >= 0 and (max_slot is None or diff(e[0], max_slot) <= 0)]

    def modify(self, slot, bnum, bcoord, file, off, ln):                   # :174-186
        for e in self.log:
            if e[0] == slot and e[1] == bnum and e[2] == bcoord:
                e[3], e[4], e[5] = file, off, ln
                return True
        return False

    def get_min_logfile(self):                                             # :319-322
        return self.min_logfile if self.log else None

    def get_logfiles(self):                                                # :253-259
        return {e[3] for e in self.log}

    def is_log_msg_needed(self, slot):                                     # :331-345, the ACCEPT branch
        return not diff(slot, self.gc_slot) <= 0


class JavaIndex:
    """MessageLogDiskMap: one LogIndex per group; a new version replaces it by a fresh one"""

    def __init__(self, groups):
        self.of = [LogIndex() for _ in range(groups)]

    def reset(self, g):
        self.of[g] = LogIndex()


# ---- the flat table -----------------------------------------------------------------------------------------------------
class FlatIndex:
    def __init__(self, groups, cap_rows):
        self.G, self.cap = groups, cap_rows
        self.gidx, self.slot, self.bnum, self.bcoord, self.file, self.len = (np.zeros(cap_rows, np.int32) for _ in range(6))
        self.off = np.zeros(cap_rows, np.int64)
        self.alive = np.zeros(cap_rows, bool)
        self.n_rows, self.generation = 0, 0
        self.gc = np.full(groups, -1, np.int32)
        self.min_file = np.full(groups, -1, np.int32)

    def _counts(self, **kw):
        c = dict.fromkeys(COUNT_FIELDS, 0)
        c.update(n_rows=self.n_rows, n_alive=int(self.alive[:self.n_rows].sum()), generation=self.generation)
        c.update(kw)
        return c

    @staticmethod
    def _taken(n, n_dev):
        return n if n_dev is None else min(n, max(int(n_dev), 0))

    def _first_records(self, gidx):
        """(status per record, the first record of each group or -1)"""
        gidx = np.asarray(gidx, np.int64)
        rec = np.full(self.G, -1, np.int64)
        status = np.zeros(gidx.shape[0], np.uint8)
        for i, g in enumerate(gidx.tolist()):
            if not 0 <= g < self.G:
                status[i] = NOGROUP
            elif rec[g] >= 0:
                status[i] = REPEAT
            else:
                rec[g] = i
        return status, rec

    def add(self, gidx, slot, bnum, bcoord, off, ln, file, n_dev=None):
        m = self._taken(len(gidx), n_dev)
        status = np.zeros(m, np.uint8)
        done = 0
        for i in range(m):
            g = int(gidx[i])
            if not 0 <= g < self.G:
                status[i] = NOGROUP
            elif diff(slot[i], self.gc[g]) <= 0:
                status[i] = STALE
            elif self.n_rows >= self.cap:
                status[i] = FULL
            else:
                r = self.n_rows
                self.gidx[r], self.slot[r], self.bnum[r], self.bcoord[r] = g, slot[i], bnum[i], bcoord[i]
                self.file[r], self.off[r], self.len[r], self.alive[r] = file, off[i], ln[i], True
                if self.min_file[g] == -1:
                    self.min_file[g] = file
                self.n_rows += 1
                done += 1
        return status, self._counts(n_done=done, n_stale=int((status == STALE).sum()), n_nogroup=int((status == NOGROUP).sum()))

    def set_gc(self, gidx, gc_slot=None, flags=0):
        status, rec = self._first_records(gidx)
        n, reset = self.n_rows, bool(flags & RESET)
        named = np.nonzero(rec >= 0)[0]
        for g in named.tolist():
            self.gc[g] = -1 if reset else i32(gc_slot[rec[g]])
        rr = rec[self.gidx[:n]]
        mine = self.alive[:n] & (rr >= 0)
        die = mine.copy() if reset else mine & (vdiff(self.slot[:n], self.gc[self.gidx[:n]]) <= 0)
        self.alive[:n] &= ~die
        for g in named.tolist():
            rows = np.nonzero(self.alive[:n] & (self.gidx[:n] == g))[0]
            self.min_file[g] = self.file[rows[0]] if rows.size else -1
        return status, self._counts(n_done=int(named.size), n_stale=int(die.sum()), n_nogroup=int((status == NOGROUP).sum()),
                                    n_repeat=int((status == REPEAT).sum()))

    def lookup(self, gidx, min_slot, max_slot=None, has_max=None, cap=0):
        status, rec = self._first_records(gidx)
        n = self.n_rows
        rr = rec[self.gidx[:n]]
        q = np.maximum(rr, 0)
        hit = self.alive[:n] & (rr >= 0)
        if len(gidx):
            lo = np.asarray(min_slot, np.int64)[q]
            hit &= vdiff(self.slot[:n], lo) >= 0
            if has_max is not None:
                hm = np.asarray(has_max, np.uint8)[q] != 0
                hi = np.asarray(max_slot, np.int64)[q]
                hit &= ~hm | (vdiff(self.slot[:n], hi) <= 0)
        rows = np.nonzero(hit)[0]
        k = min(rows.size, cap)
        w = rows[:k]
        out = dict(rec=rr[w].astype(np.int32), row=w.astype(np.int32), slot=self.slot[w], bnum=self.bnum[w],
                   bcoord=self.bcoord[w], file=self.file[w], off=self.off[w], len=self.len[w])
        return out, status, self._counts(n_done=k, n_hits=int(rows.size), n_nogroup=int((status == NOGROUP).sum()),
                                         n_repeat=int((status == REPEAT).sum()))

    def file_rows(self, file, cap):
        n = self.n_rows
        rows = np.nonzero(self.alive[:n] & (self.file[:n] == file))[0]
        k = min(rows.size, cap)
        w = rows[:k]
        out = dict(row=w.astype(np.int32), gidx=self.gidx[w], slot=self.slot[w], bnum=self.bnum[w], bcoord=self.bcoord[w],
                   off=self.off[w], len=self.len[w], gc=self.gc[self.gidx[w]])
        return out, self._counts(n_done=k, n_hits=int(rows.size))

    def relocate(self, generation, o_row, k_src, new_file, k_off, k_len, n_dev=None):
        n = len(o_row)
        m = self._taken(n, n_dev)
        done = 0
        for j in range(m):
            src = j if k_src is None else int(k_src[j])
            if generation != self.generation or not 0 <= src < n:
                continue
            r = int(o_row[src])
            if not 0 <= r < self.n_rows or not self.alive[r]:
                continue
            self.file[r], self.off[r], self.len[r] = new_file, k_off[j], k_len[j]
            done += 1
        return self._counts(n_done=done, n_stale=m - done)

    def files(self, file_base, n_files):
        n = self.n_rows
        f = self.file[:n][self.alive[:n]].astype(np.int64) - file_base
        mf = self.min_file[self.min_file != -1].astype(np.int64)
        d = mf - file_base
        inside, ginside = (f >= 0) & (f < n_files), (d >= 0) & (d < n_files)
        rows = np.bincount(f[inside], minlength=n_files).astype(np.int32)[:n_files]
        groups = np.bincount(d[ginside], minlength=n_files).astype(np.int32)[:n_files]
        lo = int(mf.min()) if mf.size else -1
        return rows, groups, lo, self._counts(n_stale=int((~inside).sum() + (~ginside).sum()))

    def compact(self):
        n = self.n_rows
        w = np.nonzero(self.alive[:n])[0]
        for c in (self.gidx, self.slot, self.bnum, self.bcoord, self.file, self.off, self.len):
            c[:w.size] = c[w]
        self.alive[:] = False
        self.alive[:w.size] = True
        self.n_rows = int(w.size)
        self.generation = i32(self.generation + 1)
        return self._counts(n_done=int(w.size))

    # what the Java comparison reads
    def group_list(self, g):
        n = self.n_rows
        w = np.nonzero(self.alive[:n] & (self.gidx[:n] == g))[0]
        return [[int(self.slot[r]), int(self.bnum[r]), int(self.bcoord[r]), int(self.file[r]), int(self.off[r]),
                 int(self.len[r])] for r in w]


# ---- the directed case list ---------------------------------------------------------------------------------------------
def recs(gidx, slot, bnum=None, bcoord=None, off=None, ln=None):
    """row columns as the pack hands them out; offsets ascend by 4 + len as in a file"""
    gidx = np.asarray(gidx, np.int32)
    n = gidx.shape[0]
    i = np.arange(n, dtype=np.int64)
    ln = (i % 37 + 1).astype(np.int32) if ln is None else np.asarray(ln, np.int32)
    off = np.concatenate([[0], np.cumsum(ln.astype(np.int64) + 4)[:-1]]) + 1000 if off is None and n else off
    return dict(gidx=gidx, slot=np.asarray([i32(s) for s in np.asarray(slot).tolist()], np.int32),
                bnum=np.asarray((i % 3) if bnum is None else bnum, np.int32),
                bcoord=np.asarray((100 + i % 2) if bcoord is None else bcoord, np.int32),
                off=np.asarray(np.zeros(0) if off is None else off, np.int64), len=ln)


def add_of(B, r, file, n_dev=None):
    return B.add(r["gidx"], r["slot"], r["bnum"], r["bcoord"], r["off"], r["len"], file, n_dev)


def case_tile_edges(B):
    """a: add of 255 / 256 / 257 / 513 records with STALE, NOGROUP and ADDED interleaved at the tile edges, onto a tail at
    0, 255, 256 and 1,023; a table with room for k < addable records, then compact and the rest; n_dev smaller, equal,
    larger, zero and negative"""
    seen = set()
    B.set_gc([5, 6], [10, INT_MAX])                                        # groups 5 and 6 refuse small slots

    def mixed(n):
        i = np.arange(n)
        g = (i * 7) % B.G
        g[i % 256 == 255] = B.G                                            # the last lane of a tile: no such group
        g[i % 256 == 0] = 5                                                # the first lane: stale (slot 3 - 10 <= 0)
        g[i % 64 == 62] = -1
        seen.add(B.n_rows)
        st, c = add_of(B, recs(g, np.where(g == 5, 3, 20 + i)), file=n % 5)
        assert c["n_done"] == int((st == ADDED).sum()) and c["n_stale"] >= 1 and (n < 64 or c["n_nogroup"] >= 1)

    def fill_to(tail):
        k = tail - B.n_rows
        add_of(B, recs([1] * k, 50 + np.arange(k)), file=1)
        assert B.n_rows == tail

    mixed(255)                                                             # onto a tail at 0
    fill_to(255)
    mixed(1)                                                               # at 255: one stale record
    add_of(B, recs([2], [9]), file=1)
    mixed(256)                                                             # at 256
    mixed(257)
    fill_to(1023)
    seen.add(B.n_rows)
    assert {0, 255, 256, 1023} <= seen, seen
    # one row of room, 513 records of which most are addable
    i = np.arange(513)
    g = np.where(i % 5 == 0, 6, i % 4)
    r = recs(g, 1000 + i)
    st, c = add_of(B, r, file=7)
    assert c["n_done"] == 1 and (st == FULL).sum() > 300 and (st == STALE).sum() == 103 and B.n_rows == 1024
    first_full = int(np.nonzero(st == FULL)[0][0])
    B.set_gc(np.arange(B.G), [900] * B.G)                                  # group 6 moves backwards with the rest
    c = B.compact()
    assert c["n_rows"] == 1
    rest = {k: v[first_full:] for k, v in r.items()}
    for nd in (-3, 0, 2, rest["gidx"].shape[0], rest["gidx"].shape[0] + 9):   # negative, zero, smaller, equal, larger
        st, c = add_of(B, rest, file=8, n_dev=nd)
        assert st.shape[0] == min(max(nd, 0), rest["gidx"].shape[0])
    B.lookup(np.arange(B.G), [0] * B.G, cap=1024)


def case_gc_reset(B):
    """b: set_gc forwards, backwards and equal; a group named three times; rows of one group over four tiles; the min
    file after the first row dies, after all die and after a later add; slots across the wrap; RESET"""
    i = np.arange(900)
    g = np.where(i % 3 == 0, 9, i % 7)                                     # group 9: 300 rows over four tiles
    add_of(B, recs(g[:450], 1 + i[:450]), file=2)
    add_of(B, recs(g[450:], 1 + i[450:]), file=3)
    st, c = B.set_gc([9, 9, 200, 9, 1], [100, 400, 5, 7, 2])
    assert st.tolist() == [ADDED, REPEAT, NOGROUP, REPEAT, ADDED] and c["n_repeat"] == 2 and c["n_stale"] > 30
    B.set_gc([9], [460])                                                   # every row of file 2 dies: the min file moves
    B.set_gc([9], [50])                                                    # backwards: nothing comes back ...
    st, _ = add_of(B, recs([9, 9], [60, 40]), file=4)                      # ... but slot 60 is no longer stale
    assert st.tolist() == [ADDED, STALE]
    B.set_gc([9], [50])                                                    # equal
    B.set_gc([9], [5000])                                                  # all die: no min file
    add_of(B, recs([9], [5001]), file=5)                                   # a later add names it again
    # across Integer.MAX_VALUE / MIN_VALUE
    w = [INT_MAX - 2, INT_MAX - 1, INT_MAX, INT_MIN, INT_MIN + 1, INT_MIN + 2]
    B.set_gc([20, 21], [INT_MAX - 3, INT_MAX - 3])
    add_of(B, recs([20] * 6 + [21] * 6, w + w), file=6)
    B.set_gc([20, 21], [INT_MAX, INT_MIN])
    st, _ = add_of(B, recs([20, 20, 21, 21], [INT_MAX, INT_MIN, INT_MIN, INT_MIN + 1]), file=6)
    assert st.tolist() == [STALE, ADDED, STALE, ADDED]
    B.lookup([20, 21, 9], [INT_MAX - 5] * 3, [INT_MIN + 5] * 3, [1, 1, 0], cap=64)
    st, c = B.set_gc([1, 9, 1], None, RESET)
    assert st.tolist() == [ADDED, ADDED, REPEAT] and c["n_stale"] > 0
    st, _ = add_of(B, recs([9, 1], [1, 1]), file=7)                        # a fresh index takes slot 1 again
    assert st.tolist() == [ADDED, ADDED]
    B.files(0, 8)
    B.lookup(np.arange(B.G), [INT_MIN] * B.G, cap=1024)                    # the negative slots
    B.lookup(np.arange(B.G), [0] * B.G, cap=1024)                          # the others


def case_lookup(B):
    """c: with and without max, empty ranges, min > max, ranges across the wrap; equal slots at two ballots in list order;
    cap cuts at 0, inside a tile and at a tile edge; a repeated group; a group with no rows"""
    i = np.arange(700)
    add_of(B, recs(i % 10, 1 + i // 10), file=0)
    add_of(B, recs([3, 3, 3], [30, 30, 30], bnum=[1, 2, 2], bcoord=[100, 100, 101]), file=1)   # slot 30 again, higher ballots
    B.set_gc([11], [INT_MAX - 10])
    add_of(B, recs([11] * 8, [INT_MAX - 3 + k for k in range(8)]), file=1)
    g = [0, 1, 2, 3, 4, 5, 6, 0, 50, 11, 11, 7]
    lo = [1, 10, 80, 30, 40, 5, INT_MIN, 1, 1, INT_MAX - 1, 0, 71]
    hi = [70, 20, 90, 30, 39, 0, 0, 3, 9, INT_MIN + 1, 0, 0]
    hm = [1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0]
    out, st, c = B.lookup(g, lo, hi, hm, cap=1024)
    assert st.tolist() == [ADDED] * 7 + [REPEAT, ADDED, ADDED, REPEAT, ADDED] and c["n_hits"] == c["n_done"]
    r3 = out["rec"] == 3
    assert out["slot"][r3].tolist() == [30] * 4 and out["bnum"][r3].tolist()[1:] == [1, 2, 2]       # list order
    assert (out["rec"] == 4).sum() == 0 and (out["rec"] == 8).sum() == 0 and (out["rec"] == 9).sum() == 4
    edge = int((out["row"] < 256).sum())                                   # the hits of the table's first tile
    assert 1 < edge < c["n_hits"] - 1
    for cap in (0, 1, edge - 1, edge, edge + 1, c["n_hits"] - 1, c["n_hits"]):
        o, _, cc = B.lookup(g, lo, hi, hm, cap=cap)
        assert cc["n_hits"] == c["n_hits"] and cc["n_done"] == min(cap, c["n_hits"])
    B.lookup(g, lo, cap=1024)                                              # no max anywhere
    B.lookup([], [], cap=16)


def case_relocate(B):
    """d (the part that needs no journal): relocate by row, with a stale generation, with row indices of -1 / tail /
    INT32_MAX, with a dead row, with k_src out of range; min files do not move; the equal-slot, equal-ballot deviation"""
    i = np.arange(300)
    add_of(B, recs(i % 6, 1 + i // 6), file=0)
    add_of(B, recs([2, 2], [77, 77], bnum=[4, 4], bcoord=[100, 100]), file=0)      # the same slot at the same ballot twice
    B.set_gc([0], [10])
    rows, c = B.file_rows(0, cap=1024)
    n = c["n_done"]
    assert n == c["n_hits"] == 302 - 10
    gen = c["generation"]
    c = B.relocate(gen + 1, rows["row"], None, 9, rows["off"] - 1000, rows["len"])  # a stale generation
    assert c["n_done"] == 0 and c["n_stale"] == n
    bad = rows["row"].copy()
    bad[0], bad[1], bad[2], bad[3] = -1, B.n_rows, INT_MAX, 0              # row 0 is dead (group 0, slot 1)
    src = np.arange(n, dtype=np.int32)
    src[5], src[6], src[7] = -1, n, INT_MAX
    c = B.relocate(gen, bad, src, 9, rows["off"] - 1000, rows["len"])
    assert c["n_stale"] == 7 and c["n_done"] == n - 7
    c = B.relocate(gen, rows["row"], None, 9, rows["off"] - 1000, rows["len"], n_dev=n // 2)
    assert c["n_done"] == n // 2
    B.files(0, 16)                                                         # the rows are in file 9, the min files still 0
    B.lookup(np.arange(6), [0] * 6, cap=1024)
    B.compact()
    c = B.relocate(gen, rows["row"], None, 10, rows["off"], rows["len"])   # row indices from before the compact: void
    assert c["n_done"] == 0


def case_files(B):
    """e: ids below, inside and above the range, 1 and 4,096 bins; the smallest min file with no group, one, all"""
    _, _, lo, _ = B.files(0, 1)
    assert lo == -1
    add_of(B, recs([4] * 3, [1, 2, 3]), file=4000)
    _, _, lo, _ = B.files(0, MAX_FILES)
    assert lo == 4000
    for f in (17, 5000, 4095, 0, 4096):
        i = np.arange(B.G + 3)
        add_of(B, recs(i % B.G, 10 + f % 97 + i // B.G), file=f)
    rows, groups, lo, c = B.files(0, MAX_FILES)
    assert lo == 17 and c["n_stale"] > 0 and groups[17] == B.G - 1 and groups[4000] == 1 and rows[0] == B.G + 3
    B.files(17, 1)
    B.files(4001, 100)
    B.files(-50, 60)
    B.files(0, 0)


def case_compact(B):
    """f: no dead rows, alternating, all dead; the generation moves; lookups before and after agree except for o_row"""
    i = np.arange(600)
    add_of(B, recs(i % 8, 1 + i), file=1)
    allg = np.arange(B.G)
    a, _, _ = B.lookup(allg, [0] * B.G, cap=1024)
    c0 = B.compact()
    assert c0["n_rows"] == 600
    B.set_gc([1, 3, 5, 7], [INT_MAX - 1000] * 4)                           # every other row dies
    a, _, _ = B.lookup(allg, [0] * B.G, cap=1024)
    c1 = B.compact()
    b, _, _ = B.lookup(allg, [0] * B.G, cap=1024)
    assert c1["generation"] == c0["generation"] + 1 and c1["n_rows"] == 300
    assert all(a[k].tolist() == b[k].tolist() for k in LOOKUP_COLS if k != "row") and a["row"].tolist() != b["row"].tolist()
    B.set_gc(allg, None, RESET)
    c2 = B.compact()
    assert c2["n_rows"] == 0 and c2["n_alive"] == 0
    add_of(B, recs([1], [1]), file=2)
    B.lookup(allg, [0] * B.G, cap=8)


CASES = dict(tile_edges=case_tile_edges, gc_reset=case_gc_reset, lookup=case_lookup, relocate=case_relocate,
             files=case_files, compact=case_compact)
