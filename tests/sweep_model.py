"""The rules of the deactivation sweep (include/gpx_sweep.h), restated in numpy: what one call answers and what it leaves
behind, from what each scanned entry IS.  The tests feed it from the CPU oracle (live and busy from
orc_group_retire(PAUSE) on a copy or from statuses taken just before, changed from orc_group_dump against its value at
the previous sweep) and compare the HIP calls with its answer."""
import numpy as np

PEEK, HOLD = 1, 2
AGE_MAX = 255


def sweep(live, busy, changed, age, min_age, flags, cap):
    """One call over n distinct entries.

    live[i]     the entry names a live group (False: dead or out of range)
    busy[i]     ... that gpx_group_retire(PAUSE) would refuse with GPX_S_BUSY
    changed[i]  the group's signature differs from the stored one (a group never seen caught up: True)
    age[i]      the stored age (0 for an entry out of range)

    -> dict: hits (entry indices written, ascending), ages (their o_age), counts (n_hits, n_nogroup, n_busy, n_paused),
       paused (entry indices paused), new_age (the stored ages after the call), stored (entries whose signature word now
       holds the current signature), cleared (entries whose signature word now holds 0)"""
    live, busy, changed = (np.asarray(a, bool) for a in (live, busy, changed))
    age = np.asarray(age, np.int64)
    assert 0 <= min_age <= AGE_MAX and cap >= 0 and not flags & ~(PEEK | HOLD)
    caught = live & ~busy
    same = age if flags & HOLD else np.minimum(age + 1, AGE_MAX)
    now = np.where(caught, np.where(changed, 0, same), 0)         # dead and busy entries: age 0
    hit = caught & (now >= min_age)
    idx = np.nonzero(hit)[0]
    k = min(idx.size, cap)
    written = idx[:k]
    peek = bool(flags & PEEK)
    paused = written[:0] if peek else written
    if peek:
        new_age = age.copy()
        stored = np.zeros(0, np.int64)
        cleared = np.zeros(0, np.int64)
    else:
        new_age = now.copy()
        new_age[paused] = 0
        stored = np.setdiff1d(np.nonzero(caught & changed)[0], paused)
        cleared = np.union1d(np.nonzero(~live)[0], paused)
    counts = (int(idx.size), int((~live).sum()), int((live & busy).sum()), int(paused.size))
    return dict(hits=written, ages=now[written].astype(np.uint8), counts=counts, paused=paused,
                new_age=new_age.astype(np.uint8), stored=stored, cleared=cleared)
