"""The journal compaction of include/gpx_journal_gc.h, restated over numpy and bytes.

`gc_of` is setGCSlot's threshold (SQLPaxosLogger.java:1481-1482), `needed` is LogIndex.isLogMsgNeeded for an ACCEPT
(LogIndex.java:333), both in Java's wrapping int arithmetic; `compact` is the header: the usable test, the verdicts,
the kept entries in row order, the k_* rows, both caps, the run count and `unchanged`.  Group state comes in as two
arrays over max_groups: `a_gc` and `exists`."""
from collections import namedtuple

import numpy as np

COUNT_ONLY, SKIP_UNCHANGED = 1, 2
DROP, KEEP, KEEP_UNJUDGED, BAD = 0, 1, 2, 3
MAX_LEN = 2 ** 31 - 1 - 4
ROW_COLS = ("src", "gidx", "slot", "bnum", "bcoord", "off", "len")
COUNT_FIELDS = ("n_usable", "n_keep", "n_done", "n_bad", "n_unjudged", "n_runs_done", "unchanged", "reserved",
                "keep_bytes", "bytes_done", "named_bytes", "reserved2")

Compacted = namedtuple("Compacted", "bytes rows verdicts counts")   # rows: {column: array}; counts: dict


def i32(x):
    """Java's int: x wrapped into [-2^31, 2^31)"""
    return (int(x) + 2 ** 31) % 2 ** 32 - 2 ** 31


def gc_of(acc, cp=None):
    """slot - acceptedGCSlot < 0 ? slot : acceptedGCSlot, with slot = the caller's checkpointed slot"""
    return int(acc) if cp is None else (int(cp) if i32(int(cp) - int(acc)) < 0 else int(acc))


def needed(slot, gc):
    """!(slot - gcSlot <= 0)"""
    return i32(int(slot) - int(gc)) > 0


def compact(data, in_bytes, in_base, e_gidx, e_slot, e_off, e_len, a_gc, exists, e_bnum=None, e_bcoord=None, cp_slot=None,
            out_base=0, flags=0, cap_bytes=None, cap_entries=None):
    """gpx_journal_gc on host data.  data None: no prefix test (GPX_JG_COUNT_ONLY with in == NULL).  cap_bytes /
    cap_entries None: no cut."""
    data = None if data is None else bytes(data)
    n, G = len(e_len), len(a_gc)
    verdicts = np.zeros(n, np.uint8)
    ents = []                                       # (row, rel, len, pos, head)
    pos = named = n_bad = n_unj = 0
    prev_end = None                                 # where row i - 1 ends if it is kept
    for i in range(n):
        rel, ln = int(e_off[i]) - int(in_base), int(e_len[i])
        ok = rel >= 0 and 0 <= ln <= MAX_LEN and rel + 4 + ln <= in_bytes
        if ok and data is not None:
            ok = int.from_bytes(data[rel:rel + 4], "big", signed=True) == ln
        if not ok:
            verdicts[i], n_bad, prev_end = BAD, n_bad + 1, None
            continue
        named += 4 + ln
        g = int(e_gidx[i])
        if not 0 <= g < G or not exists[g]:
            v, n_unj = KEEP_UNJUDGED, n_unj + 1
        else:
            v = KEEP if needed(e_slot[i], gc_of(a_gc[g], None if cp_slot is None else cp_slot[i])) else DROP
        verdicts[i] = v
        if v == DROP:
            prev_end = None
            continue
        ents.append((i, rel, ln, pos, prev_end != rel))
        pos += 4 + ln
        prev_end = rel + 4 + ln
    n_keep, heads = len(ents), sum(1 for t in ents if t[4])
    unchanged = int(n_bad == 0 and n_keep == n and heads == (1 if n else 0) and (n == 0 or ents[0][1] == 0) and pos == in_bytes)
    done = []
    if not flags & COUNT_ONLY and not (flags & SKIP_UNCHANGED and unchanged):
        for e, t in enumerate(ents):
            if (cap_entries is not None and e >= cap_entries) or (cap_bytes is not None and t[3] + 4 + t[2] > cap_bytes):
                break
            done.append(t)
    out = b"".join(data[rel:rel + 4 + ln] for _, rel, ln, _, _ in done)
    rows = None
    if not flags & COUNT_ONLY:
        idx = np.array([t[0] for t in done], np.int64)
        rows = {"src": idx.astype(np.int32), "gidx": np.asarray(e_gidx, np.int32)[idx], "slot": np.asarray(e_slot, np.int32)[idx],
                "bnum": None if e_bnum is None else np.asarray(e_bnum, np.int32)[idx],
                "bcoord": None if e_bcoord is None else np.asarray(e_bcoord, np.int32)[idx],
                "off": np.array([out_base + t[3] for t in done], np.int64), "len": np.array([t[2] for t in done], np.int32)}
    counts = dict(n_usable=n - n_bad, n_keep=n_keep, n_done=len(done), n_bad=n_bad, n_unjudged=n_unj,
                  n_runs_done=sum(1 for t in done if t[4]), unchanged=unchanged, reserved=0, keep_bytes=pos,
                  bytes_done=len(out), named_bytes=named, reserved2=0)
    return Compacted(out, rows, verdicts, counts)


def counts_of(c):
    """a JournalGcCounts structure as the model's dict"""
    return {f: int(getattr(c, f)) for f in COUNT_FIELDS}


def outcome(counts):
    """compactLogfile's three outcomes (SQLPaxosLogger.java:3420-3436)"""
    return "delete" if counts["n_keep"] == 0 else "leave" if counts["unchanged"] else "replace"
