"""Back ends for the directed cases of tests/logindex_model.py: `JavaChecked` runs a case on the flat model and on the
restated Java at once and compares their whole state after every call; `Both` runs it on the flat model and on the
library (`HostCalls`: the host twins, `DevCalls`: the _dev forms on buffers inside guard bands) and compares every
output bit for bit."""
import numpy as np

from tests import logindex_model as LM


def _norm(x):
    if isinstance(x, dict):
        return {k: _norm(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return [_norm(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.astype(np.int64).tolist()
    return int(x)


class Both:
    """every call on the model and on `impl`; the outputs must agree; the model's are returned"""

    def __init__(self, model, impl):
        self.m, self.impl, self.calls = model, impl, 0

    G = property(lambda s: s.m.G)
    n_rows = property(lambda s: s.m.n_rows)

    def __getattr__(self, name):
        def call(*a, **kw):
            want, got = getattr(self.m, name)(*a, **kw), getattr(self.impl, name)(*a, **kw)
            self.calls += 1
            assert _norm(want) == _norm(got), "%s, call %d: the model and the library disagree\n%r\n%r" % (
                name, self.calls, _norm(want), _norm(got))
            return want
        return call


class JavaChecked:
    """every call on the flat model and on the restated Java (one LogIndex per group, fed entry by entry as
    SQLPaxosLogger feeds it); after each the two hold the same lists, GC slots and min files.  `deviations` counts the
    entries that differ after a relocate, all of which must be duplicates of (slot, ballot) inside their group."""

    def __init__(self, groups, cap_rows):
        self.m, self.j = LM.FlatIndex(groups, cap_rows), LM.JavaIndex(groups)
        self.deviations = 0
        self.seen = dict(stale=0, backwards_gone=0, min_file_moved=0, wrap_range=0)
        self._allowed, self._removed = set(), {}

    G = property(lambda s: s.m.G)
    n_rows = property(lambda s: s.m.n_rows)

    def _same(self):
        for g in range(self.G):
            a, b = self.m.group_list(g), self.j.of[g].log
            if a != b:
                assert len(a) == len(b), g
                for x, y in zip(a, b):
                    if x != y:
                        key = tuple(x[:3])
                        assert x[:3] == y[:3] and sum(1 for z in a if tuple(z[:3]) == key) > 1, (g, x, y)
                        self._allowed.add((g, key))
            assert int(self.m.gc[g]) == self.j.of[g].gc_slot, g
            mf = self.j.of[g].get_min_logfile()
            assert int(self.m.min_file[g]) == (-1 if mf is None else mf), g
            if a and a[0][3] != int(self.m.min_file[g]):
                self.seen["min_file_moved"] += 1
        self.deviations = len(self._allowed)

    def add(self, gidx, slot, bnum, bcoord, off, ln, file, n_dev=None):
        st, c = self.m.add(gidx, slot, bnum, bcoord, off, ln, file, n_dev)
        for i, s in enumerate(st.tolist()):
            if s == LM.NOGROUP:
                continue
            if s == LM.FULL:                                               # the table's limit is not the reference's
                continue
            g = int(gidx[i])
            assert self.j.of[g].is_log_msg_needed(int(slot[i])) == (s == LM.ADDED)
            ok = self.j.of[g].add(int(slot[i]), int(bnum[i]), int(bcoord[i]), int(file), int(off[i]), int(ln[i]))
            assert ok == (s == LM.ADDED), (i, s)
            self.seen["stale"] += s == LM.STALE
        self._same()
        return st, c

    def set_gc(self, gidx, gc_slot=None, flags=0):
        st, c = self.m.set_gc(gidx, gc_slot, flags)
        for i, s in enumerate(st.tolist()):
            if s != LM.ADDED:
                continue
            g = int(gidx[i])
            x = self.j.of[g]
            if flags & LM.RESET:
                self.j.reset(g)
                self._removed.pop(g, None)
                continue
            old, new, had = x.gc_slot, LM.i32(gc_slot[i]), [e[0] for e in x.log]
            x.set_gc_slot(new)
            gone = self._removed.setdefault(g, set())
            gone.update(set(had) - {e[0] for e in x.log})
            # backwards: a slot that an earlier, larger GC slot removed would be needed again, and stays removed
            if LM.diff(new, old) < 0 and any(x.is_log_msg_needed(q) and q not in {e[0] for e in x.log} for q in gone):
                self.seen["backwards_gone"] += 1
        self._same()
        return st, c

    def lookup(self, gidx, min_slot, max_slot=None, has_max=None, cap=0):
        out, st, c = self.m.lookup(gidx, min_slot, max_slot, has_max, cap)
        if c["n_done"] == c["n_hits"]:
            for i, s in enumerate(st.tolist()):
                if s != LM.ADDED:
                    continue
                mx = None if has_max is None or not has_max[i] else LM.i32(max_slot[i])
                want = self.j.of[int(gidx[i])].get_logged_accepts(LM.i32(min_slot[i]), mx)
                w = out["rec"] == i
                got = [list(map(int, r)) for r in zip(out["slot"][w], out["bnum"][w], out["bcoord"][w], out["file"][w],
                                                      out["off"][w], out["len"][w])]
                if int(gidx[i]) not in {g for g, _ in self._allowed}:     # a group the deviation has touched: _same()
                    assert got == want, (i, got, want)
                if mx is not None and LM.i32(min_slot[i]) > mx and want:
                    self.seen["wrap_range"] += 1
        return out, st, c

    def file_rows(self, file, cap):
        return self.m.file_rows(file, cap)

    def relocate(self, generation, o_row, k_src, new_file, k_off, k_len, n_dev=None):
        n = len(o_row)
        m = n if n_dev is None else min(n, max(int(n_dev), 0))
        todo = []
        for j in range(m):                                                 # what the model will accept, before it does
            src = j if k_src is None else int(k_src[j])
            if generation != self.m.generation or not 0 <= src < n:
                continue
            r = int(o_row[src])
            if 0 <= r < self.m.n_rows and self.m.alive[r]:
                todo.append((int(self.m.gidx[r]), int(self.m.slot[r]), int(self.m.bnum[r]), int(self.m.bcoord[r]),
                             int(new_file), int(k_off[j]), int(k_len[j])))
        c = self.m.relocate(generation, o_row, k_src, new_file, k_off, k_len, n_dev)
        assert c["n_done"] == len(todo)
        for g, *e in todo:                                                 # modifyLogIndexEntry, entry by entry
            assert self.j.of[g].modify(*e)
        self._same()
        return c

    def files(self, file_base, n_files):
        rows, groups, lo, c = self.m.files(file_base, n_files)
        if not self._allowed:
            used = set().union(*[x.get_logfiles() for x in self.j.of])
            assert {file_base + f for f in np.nonzero(rows)[0].tolist()} == {f for f in used if 0 <= f - file_base < n_files}
        mins = [x.get_min_logfile() for x in self.j.of if x.get_min_logfile() is not None]
        assert lo == (min(mins) if mins else -1)
        for f in range(n_files):                                           # FileIDMap.isRemovable's question
            assert int(groups[f]) == sum(1 for x in mins if x == file_base + f)
        return rows, groups, lo, c

    def compact(self):
        c = self.m.compact()
        self._same()
        return c


def counts_dict(c):
    return {f: int(getattr(c, f)) for f in LM.COUNT_FIELDS}


class HostCalls:
    """the host-pointer twins (gigapaxos_amd/logindex.py) in the model's shapes"""

    def __init__(self, e):
        self.e = e

    def add(self, gidx, slot, bnum, bcoord, off, ln, file, n_dev=None):
        from gigapaxos_amd import logindex as L
        st, c = L.add(self.e, gidx, slot, bnum, bcoord, off, ln, file, n_dev)
        return st, counts_dict(c)

    def set_gc(self, gidx, gc_slot=None, flags=0):
        from gigapaxos_amd import logindex as L
        st, c = L.set_gc(self.e, gidx, gc_slot, flags)
        return st, counts_dict(c)

    def lookup(self, gidx, min_slot, max_slot=None, has_max=None, cap=0):
        from gigapaxos_amd import logindex as L
        out, st, c = L.lookup(self.e, gidx, min_slot, max_slot, has_max, cap)
        return out, st, counts_dict(c)

    def file_rows(self, file, cap):
        from gigapaxos_amd import logindex as L
        out, c = L.file_rows(self.e, file, cap)
        return out, counts_dict(c)

    def relocate(self, generation, o_row, k_src, new_file, k_off, k_len, n_dev=None):
        from gigapaxos_amd import logindex as L
        return counts_dict(L.relocate(self.e, generation, o_row, k_src, new_file, k_off, k_len, n_dev))

    def files(self, file_base, n_files):
        from gigapaxos_amd import logindex as L
        rows, groups, lo, c = L.files(self.e, file_base, n_files)
        return rows, groups, lo, counts_dict(c)

    def compact(self):
        from gigapaxos_amd import logindex as L
        return counts_dict(L.compact(self.e))


class DevCalls:
    """the _dev forms: every buffer of a call inside 4 KiB guard bands (tests/journal_common.Guarded); an output column
    carries a sentinel that must still stand from the last entry written to the end of its band.  How many entries that is
    comes from the counts the device itself returns; `Both` then compares counts and entries with the model's."""

    def __init__(self, e):
        self.e = e

    def _run(self, ins, outs, call):
        """ins: name -> array; outs: name -> (dtype, entries); call(ptr) queues the _dev call -> (Guarded, counts)"""
        from tests.journal_common import Guarded, SENTINEL
        A = Guarded()
        for k, v in ins.items():
            if v is not None:
                A.put(k, v, live=True)
        for k, (dt, cnt) in outs.items():
            A.put(k, np.full(cnt * np.dtype(dt).itemsize, SENTINEL, np.uint8))
        A.put("counts", np.full(32, SENTINEL, np.uint8))
        A.upload()
        call(A.ptr)
        self.e.sync()
        A.download()
        from gigapaxos_amd.logindex import LogIndexCounts
        return A, counts_dict(LogIndexCounts.from_buffer_copy(A.get("counts").tobytes()))

    @staticmethod
    def _i32(a):
        return None if a is None else np.asarray([LM.i32(x) for x in np.asarray(a).tolist()], np.int32)

    def add(self, gidx, slot, bnum, bcoord, off, ln, file, n_dev=None):
        from gigapaxos_amd import logindex as L
        n = len(gidx)
        ins = dict(gidx=self._i32(gidx), slot=self._i32(slot), bnum=self._i32(bnum), bcoord=self._i32(bcoord),
                   off=np.asarray(off, np.int64), len=self._i32(ln), n_dev=None if n_dev is None else np.array([n_dev], np.int32))
        A, c = self._run(ins, dict(status=(np.uint8, n)), lambda p: L.add_dev(
            self.e, n, p("n_dev"), [p(k) for k in ("gidx", "slot", "bnum", "bcoord", "off", "len")], file, p("status"), p("counts")))
        m = n if n_dev is None else min(n, max(int(n_dev), 0))
        A.unchanged_outside(dict(counts=32, status=m))
        return A.get("status")[:m], c

    def set_gc(self, gidx, gc_slot=None, flags=0):
        from gigapaxos_amd import logindex as L
        n = len(gidx)
        A, c = self._run(dict(gidx=self._i32(gidx), gc=self._i32(gc_slot)), dict(status=(np.uint8, n)), lambda p: L.set_gc_dev(
            self.e, n, p("gidx"), p("gc"), flags, p("status"), p("counts")))
        A.unchanged_outside(dict(counts=32, status=n))
        return A.get("status")[:n], c

    def lookup(self, gidx, min_slot, max_slot=None, has_max=None, cap=0):
        from gigapaxos_amd import logindex as L
        n = len(gidx)
        ins = dict(gidx=self._i32(gidx), lo=self._i32(min_slot), hi=self._i32(max_slot),
                   hm=None if has_max is None else np.asarray(has_max, np.uint8))
        outs = {k: (dt, cap) for k, dt in L.LOOKUP_COLS} if cap else {}
        outs["status"] = (np.uint8, n)
        A, c = self._run(ins, outs, lambda p: L.lookup_dev(
            self.e, n, p("gidx"), p("lo"), p("hi"), p("hm"), cap, [p(k) for k, _ in L.LOOKUP_COLS], p("status"), p("counts")))
        k = c["n_done"]
        assert 0 <= k <= cap
        A.unchanged_outside(dict(counts=32, status=n, **({q: k * np.dtype(dt).itemsize for q, dt in L.LOOKUP_COLS} if cap else {})))
        return ({q: (A.get(q, dt)[:k] if cap else np.zeros(0, dt)) for q, dt in L.LOOKUP_COLS}, A.get("status")[:n], c)

    def file_rows(self, file, cap):
        from gigapaxos_amd import logindex as L
        outs = {k: (dt, cap) for k, dt in L.FILE_ROWS_COLS} if cap else {}
        A, c = self._run({}, outs, lambda p: L.file_rows_dev(self.e, file, cap, [p(k) for k, _ in L.FILE_ROWS_COLS], p("counts")))
        k = c["n_done"]
        assert 0 <= k <= cap
        A.unchanged_outside(dict(counts=32, **({q: k * np.dtype(dt).itemsize for q, dt in L.FILE_ROWS_COLS} if cap else {})))
        return {q: (A.get(q, dt)[:k] if cap else np.zeros(0, dt)) for q, dt in L.FILE_ROWS_COLS}, c

    def relocate(self, generation, o_row, k_src, new_file, k_off, k_len, n_dev=None):
        from gigapaxos_amd import logindex as L
        n = len(o_row)
        ins = dict(row=self._i32(o_row), src=self._i32(k_src), off=np.asarray(k_off, np.int64), len=self._i32(k_len),
                   n_dev=None if n_dev is None else np.array([n_dev], np.int32))
        A, c = self._run(ins, {}, lambda p: L.relocate_dev(
            self.e, n, p("n_dev"), generation, p("row"), p("src"), new_file, p("off"), p("len"), p("counts")))
        A.unchanged_outside(dict(counts=32))
        return c

    def files(self, file_base, n_files):
        from gigapaxos_amd import logindex as L
        outs = dict(rows=(np.int32, n_files), groups=(np.int32, n_files), lo=(np.int32, 1))
        A, c = self._run({}, outs, lambda p: L.files_dev(self.e, file_base, n_files, p("rows"), p("groups"), p("lo"), p("counts")))
        A.unchanged_outside(dict(counts=32, rows=4 * n_files, groups=4 * n_files, lo=4))
        return A.get("rows", np.int32), A.get("groups", np.int32), int(A.get("lo", np.int32)[0]), c

    def compact(self):
        from gigapaxos_amd import logindex as L
        A, c = self._run({}, {}, lambda p: L.compact_dev(self.e, p("counts")))
        A.unchanged_outside(dict(counts=32))
        return c
