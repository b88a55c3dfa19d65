"""Delta images (include/gpx_delta.h) as a model over gpx_group_dump words.  The mark of a group is "its dump at the export
that last wrote it" (None: mark 0), changed means "the dump differs"; the cap / prefix rules and the gone rule are
restated.  A row is a function of (dump, gidx, my_id, kmax, window) and back (tests/image_model.py), so "the dump
differs" and "the rows differ" are the same statement.  Nothing here knows a signature."""

EVICT, FULL = 1, 2


class DeltaModel:
    def __init__(self, n_groups):
        self.n = int(n_groups)
        self.mark = [None] * self.n

    def export(self, dumps, nrows, entries=None, flags=0, cap=0, cap_gone=0):
        """dumps[g]: the dump of group g as a tuple, None for a dead group; nrows[g]: the rows a live group needs (1, or
        2 while it runs for coordinator).  entries None = the whole table.  Updates the marks; returns the changed, the
        written, the gone and the listed gone groups in entry order, and the eight counts."""
        live, changed, gone = 0, [], []
        for g in (range(self.n) if entries is None else entries):
            g = int(g)
            if not 0 <= g < self.n:
                continue
            d = dumps[g]
            if d is not None:
                live += 1
                if (flags & FULL) or self.mark[g] != d:
                    changed.append(g)
            elif self.mark[g] is not None:
                gone.append(g)
        written, used = [], 0
        for g in changed:                                   # the longest prefix whose rows all fit
            if used + nrows[g] > cap:
                break
            written.append(g)
            used += nrows[g]
        listed = gone[:cap_gone]
        for g in written:
            self.mark[g] = None if flags & EVICT else dumps[g]
        for g in listed:
            self.mark[g] = None
        counts = (live, len(changed), sum(nrows[g] for g in changed), len(written), used, len(gone), len(listed), 0)
        return dict(changed=changed, written=written, gone=gone, listed=listed, counts=counts)
