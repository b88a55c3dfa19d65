"""numpy restatement of include/gpx_scan.h: given the DENSE columns of a scan (what gpx_election_scan / gpx_poke_scan /
gpx_gap_scan write, here the CPU oracle's), the groups of the scanned entries and `cap`, the compact columns and the
counts the hit-compacting call must produce.  Pure numpy: no library, no GPU."""
import numpy as np

S_OK, S_NOGROUP, S_STOPPED = 0, 1, 2
RUN_NO, POKE_NONE = 0, 0
GAP_HIT_SYNC, GAP_HIT_MISSING, GAP_HIT_AHEAD = 1, 2, 4

# compact column dtypes, in argument order (o_gidx first)
DTYPES = {"election": (np.int32, np.uint8, np.int32, np.int32),
          "poke": (np.int32, np.uint8, np.int32, np.int32, np.int32, np.int32, np.uint8, np.uint32),
          "gap": (np.int32, np.int32, np.int32, np.uint64, np.uint8)}
HIT_BYTES = {k: sum(np.dtype(d).itemsize for d in v) for k, v in DTYPES.items()}   # 13, 26, 21
DENSE_BYTES = {"election": 10, "poke": 23, "gap": 18}                                # out, per scanned entry


def hit_mask(kind, dense, require=0):
    """Which scanned entries are hits: the table of include/gpx_scan.h over the dense row."""
    status = np.asarray(dense[-1])
    ok = status == S_OK
    if kind == "election":
        return ok & (np.asarray(dense[0]) != RUN_NO)
    if kind == "poke":
        return ok & (np.asarray(dense[0]) != POKE_NONE)
    first, maxc, missing, sync = (np.asarray(c) for c in dense[:4])
    m = ok.copy()                                    # a stopped group (S_STOPPED) is never a hit
    if require & GAP_HIT_SYNC:
        m &= sync != 0
    if require & GAP_HIT_MISSING:
        m &= missing != 0
    if require & GAP_HIT_AHEAD:                      # Java's maxc - first >= 0: the difference taken in int32
        m &= (maxc.astype(np.int64) - first.astype(np.int64)).astype(np.int32) >= 0
    return m


def compact(kind, dense, groups, cap, require=0):
    """-> (compact columns cut to min(n_hits, cap) entries, n_hits, n_nogroup).  `dense` = the dense call's columns in
    its argument order, status last; `groups` = the group of every scanned entry (gidx, or arange(n))."""
    groups = np.asarray(groups, np.int32)
    m = hit_mask(kind, dense, require)
    idx = np.nonzero(m)[0]                           # ascending entry index
    n_hits = int(idx.shape[0])
    idx = idx[:max(0, min(n_hits, cap))]
    cols = [groups[idx]] + [np.asarray(c)[idx] for c in dense[:-1]]
    cols = tuple(np.ascontiguousarray(c, dt) for c, dt in zip(cols, DTYPES[kind]))
    return cols, n_hits, int((np.asarray(dense[-1]) == S_NOGROUP).sum())
