/*
 * gpx_timers.h — retransmission timers on the device: a sweep that returns only the ACCEPTs and PREPAREs that are due.
 *
 * gpx_poke_scan (include/gpx.h) says WHAT is waiting for replies; since when was the caller's business.  The reference
 * keeps that in WaitforUtility.initTime / retransmissionCount (paxosutil/WaitforUtility.java:39-40, 101-127), tested by
 * PaxosCoordinatorState.testAndSetWaitingTooLong() for the outstanding PREPARE and testAndSetWaitingTooLong(int slot)
 * for the head-of-line ACCEPT (PCS:715-739), reached from pokeLocalCoordinator -> reissueAcceptIfWaitingTooLong
 * (PISM:2268-2279, PaxosCoordinator.java:334-350) and the PREPARE resend branch of checkRunForCoordinator
 * (PISM:2169-2181).  gpx_retransmit_sweep is those tests over a whole table as one call: a node's batch timer calls
 * it with its clock, and what comes back is exactly the frames to send again.  As in the deactivation sweep
 * (gpx_sweep.h) the clock needs no store on the data path: three engine-owned words per group that only this call
 * touches are brought up to date once per sweep.
 *
 * DEVIATION FROM THE REFERENCE.  The reference stamps initTime when the proposal or waitforMyBallot is CREATED.  No
 *   data-path call of the engine takes a clock, so the engine stamps a wait at the first sweep that SEES it.  Hence:
 *   a wait that starts and ends between two sweeps is never seen; and a retransmission comes at most one sweep period
 *   later than the Java's, never at a shorter interval than its thresholds.  A host that wants the Java's instants
 *   runs a cap == 0 sweep right after the call that starts the wait.
 * Clock.  now_ms is the caller's, in milliseconds, wrapping: only differences are used.  Waits of 2^31 ms and more are
 *   not supported.  A clock that steps back makes a wait look negative: never a hit, nothing else happens.
 * Scanned entries.  Entry i < n is group gidx[i], or group i when gidx == NULL.  n above max(max_groups, max_batch)
 *   is refused with GPX_ECAPACITY.  Listed entries must be pairwise distinct (not checked, as for gpx_pause_sweep).
 * Thresholds.  cfg (HOST memory in both forms: it travels by value, like the scans' node lists) holds one table per
 *   kind: after c retransmissions a wait is due when it is longer than table[min(c, n_steps - 1)] milliseconds.
 *   gpx_rtx_backoff_table fills a table with the reference's back-off: out[c] = min(floor(timeout_ms * factor^c),
 *   INT32_MAX).  The Java compares a long wait with TIMEOUT * Math.pow(1.5, count) using `>`; for an integer wait,
 *   wait > x <=> wait > floor(x), so the integer table is exact, and 1.5^c is exactly representable for c <= 32.
 *   The reference's defaults: ACCEPT_TIMEOUT = PREPARE_TIMEOUT = FAILURE_DETECTION_TIMEOUT seconds * 1000, factor 1.5
 *   (PCS:60-64).
 * Timer words.  Three engine-owned arrays over max_groups - key (32 bits), since (32 bits), count (8 bits) - allocated
 *   zeroed by the first call (GPX_ENOMEM if that fails: the engine stays usable).  No other call reads or writes them;
 *   they are not part of a group's state: images, deltas, dumps and the pause sweep do not see them.
 * Evaluation of a scanned entry, r = the row gpx_poke_scan writes for it:
 *   r.status == GPX_S_NOGROUP   counted in n_nogroup; the three words of an in-range group become 0.
 *   r.poke == GPX_POKE_NONE     key and count become 0.
 *   otherwise                   counted in n_waiting.  k = a 32-bit mix of (r.poke, r.slot, r.bnum, r.bcoord), forced
 *                               non-zero; r.heard is NOT part of it: a reply does not restart the Java's initTime.
 *       k != key (a new wait)   key = k, since = now_ms, count = 0.  Not a hit.
 *       k == key                waited = (int32_t)((uint32_t)now_ms - (uint32_t)since), thr = the kind's table at
 *                               min(count, n_steps - 1).  A HIT iff waited > thr - strict, as PCS:717 and PCS:732 are.
 *                               A negative waited is never a hit.
 *   Only stores that change a word are made: a table at rest is read, not written.
 * Output.  Hits leave in ascending entry index.  Hit j carries o_gidx[j] = its group, the seven columns gpx_poke_scan
 *   writes for it (o_poke .. o_heard), o_count[j] = its retransmission count AFTER this one and o_waited[j].  Only the
 *   first min(n_hits, cap) entries of each column are written; nothing at or beyond that index is touched.  cap == 0
 *   with null columns counts only; with cap > 0 every column must be given.  `counts` is always written whole.
 * Re-arming.  Without GPX_RTX_PEEK exactly the hits written are re-armed: count = min(count + 1, 255), since = now_ms
 *   (incrRetransmissonCount(true)).  A hit at or beyond cap is left alone: it is a hit again on the next call.  Under
 *   GPX_RTX_PEEK no timer word changes at all - neither these nor the arming and disarming above.
 * Caveat.  A group retired and re-created with the same head-of-line slot and ballot between two sweeps continues its
 *   timer.  Harmless: a repeated ACCEPT or PREPARE is always safe.  (Two waits with one key - probability 2^-32 per
 *   comparison, and never when they differ in one field only - have the same effect.)
 * Not modelled: ranRecently (PCS:752-756), the rate limit on running for coordinator, stays with the host.
 * _dev form.  Every pointer but cfg is a DEVICE pointer (counts too; gidx nullable).  Asynchronous on the stream
 *   gpx_election_begin_dev uses: three launches ordered by the stream alone, no workgroup waits for another one.
 * Host twin.  Every pointer is host memory.  Runs the _dev form into engine-owned device memory, copies `counts`,
 *   then min(n_hits, cap) entries per column, as the twins of gpx_scan.h do: 31 bytes per due entry plus 16 cross the
 *   link (and gidx when given).  Synchronous.
 * Errors.  All argument checks come before any device work and before the handle is used:
 *   GPX_EINVAL     null handle, cfg or counts; negative n or cap; n_steps outside 1 .. GPX_RTX_MAX_STEPS; a negative
 *                  threshold among the first n_steps of either table; unknown flag bits; cap > 0 with a null column
 *   GPX_ECAPACITY  n above max(max_groups, max_batch)
 *   GPX_ENOMEM     the timer words could not be allocated
 */
#ifndef GPX_TIMERS_H
#define GPX_TIMERS_H

#include "gpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPX_RTX_MAX_STEPS 32
typedef struct gpx_rtx_cfg {            /* HOST memory in both forms */
  int32_t n_steps;                      /* 1 .. GPX_RTX_MAX_STEPS */
  int32_t accept_ms[GPX_RTX_MAX_STEPS]; /* threshold after c retransmissions; c >= n_steps uses the last entry */
  int32_t prepare_ms[GPX_RTX_MAX_STEPS];
} gpx_rtx_cfg;

typedef struct gpx_rtx_counts { /* 16 bytes, always written whole */
  int32_t n_hits;               /* due entries found; may exceed cap */
  int32_t n_nogroup;            /* scanned entries that name no live group */
  int32_t n_waiting;            /* scanned entries whose poke row is not GPX_POKE_NONE, due or not */
  int32_t n_fired;              /* entries re-armed by this call: min(n_hits, cap), 0 under GPX_RTX_PEEK */
} gpx_rtx_counts;

#define GPX_RTX_PEEK 1 /* report only: no timer word changes */

/* host helper, no engine: out[c] = min(floor(timeout_ms * factor^c), INT32_MAX) for c < n_steps.  GPX_EINVAL: null
 * out, n_steps outside 1 .. GPX_RTX_MAX_STEPS, negative timeout_ms, factor below 1 or not finite */
int gpx_rtx_backoff_table(int32_t timeout_ms, double factor, int32_t n_steps, int32_t* out);

int gpx_retransmit_sweep_dev(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t now_ms, const gpx_rtx_cfg* cfg,
                             int32_t flags, int32_t cap, int32_t* o_gidx, uint8_t* o_poke, int32_t* o_slot,
                             int32_t* o_bnum, int32_t* o_bcoord, int32_t* o_median_cp, uint8_t* o_flags,
                             uint32_t* o_heard, uint8_t* o_count, int32_t* o_waited, gpx_rtx_counts* counts);
int gpx_retransmit_sweep(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t now_ms, const gpx_rtx_cfg* cfg,
                         int32_t flags, int32_t cap, int32_t* o_gidx, uint8_t* o_poke, int32_t* o_slot,
                         int32_t* o_bnum, int32_t* o_bcoord, int32_t* o_median_cp, uint8_t* o_flags,
                         uint32_t* o_heard, uint8_t* o_count, int32_t* o_waited, gpx_rtx_counts* counts);

#ifdef __cplusplus
}
#endif
#endif /* GPX_TIMERS_H */
