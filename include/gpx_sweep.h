/*
 * gpx_sweep.h — the deactivation sweep: pause idle, caught-up groups on the device.
 *
 * PaxosManager.syncAndDeactivate walks every active instance once per DEACTIVATION_PERIOD, batches the ones that are
 * isLongIdle() and pauses each through tryPause, which succeeds only if acceptor and coordinator are caughtUp(); over
 * half capacity it force-pauses whether idle or not.  gpx_pause_sweep is that walk as one call: it finds the groups
 * that gpx_group_retire(GPX_RETIRE_PAUSE) would accept AND whose state has not changed for min_age sweeps, hands back
 * their restore rows compacted in entry order (the hit-compaction of gpx_scan.h), and pauses exactly the groups it
 * hands back.  Idleness needs no store on the data path: a group is idle if a signature of its state equals the one
 * the previous sweep saw - the batch form of lastActiveTime.  No other call reads or writes the words this keeps.
 *
 * Scanned entries.  Entry i < n is group gidx[i], or group i when gidx == NULL.  n above max(max_groups, max_batch)
 *   is refused with GPX_ECAPACITY.  Listed entries must be pairwise distinct (not checked, as for
 *   gpx_election_begin_dev).
 * Idle words.  Two engine-owned arrays over max_groups: a 32-bit signature and an 8-bit age, allocated zeroed by the
 *   first sweep (GPX_ENOMEM if that fails: the engine stays usable).
 * Evaluation of a scanned entry:
 *   dead or out of range   counted in n_nogroup; both its words become 0.
 *   live but busy          gpx_group_retire(PAUSE) would answer GPX_S_BUSY (the same test, with the same dependence
 *                          on GPX_F_ACCEPTS_FROM_DISK): counted in n_busy, its age becomes 0, never a hit.  (The sync
 *                          half of the reference's sweep is gpx_gap_scan_hits over these groups.)  A group that is
 *                          running for coordinator and has no proposals of its own is NOT busy
 *                          (PaxosCoordinatorState.caughtUp :758-761): it can be paused, its row says has_coord = 0.
 *   live and caught up     sig = a 32-bit mix of the group's state words, forced non-zero.  If sig equals the stored
 *                          signature the age becomes stored age + 1, saturating at 255 (under GPX_SWEEP_HOLD: the
 *                          stored age, unchanged); otherwise the age becomes 0 and sig is stored.  The entry is a HIT
 *                          iff age >= min_age.  min_age == 0 makes every caught-up group a hit: the reference's forced
 *                          pause, with cap as its bound.
 * Signature coverage: every word a call can change while the group stays caught up -
 *   g_flags (exists, stopped, has-coordinator, preparing, k), g_version, a_slot, a_bnum, a_bcoord, a_gc, c_bnum,
 *   c_bcoord, c_next, c_pcount, node_slots[0..k), all `window` acc_ring entries whole (with accepts from disk an
 *   accepted, uncommitted slot leaves the group caught up and is activity), and, while the group is running for
 *   coordinator, c_wait and all `window` co_ring entries whole.  Not covered, because they cannot change on a group
 *   that stays caught up: members (written by gpx_group_create only), com_ring (an entry is present only while the
 *   group is busy, and its presence bit is in the acc_ring flag word, which is covered), p_ring / p_handle (entries
 *   exist only while c_pcount != 0: busy), co_handle (changes only together with its co_ring entry).
 * Output.  Hits leave in ascending entry index.  Hit j carries o_gidx[j] = its group, o_age[j] = its age and
 *   o_rows[j] = exactly the row gpx_group_retire writes for it.  Only the first min(n_hits, cap) entries of each
 *   column are written; nothing at or beyond that index is touched.  cap == 0 with null columns counts only (and
 *   pauses nothing); with cap > 0 every column must be given.  `counts` is always written whole.
 * Pausing.  Without GPX_SWEEP_PEEK exactly the groups written are paused, each as gpx_group_retire(PAUSE) does it
 *   (the group stops existing; a bound name answers GPX_W_NOGROUP from then on), and their idle words become 0.  A
 *   hit beyond cap is left alone and keeps its age: it is a hit again on the next call - use GPX_SWEEP_HOLD for a
 *   call that continues after a cut within the same period.
 * Caveat.  A row retired by gpx_group_retire and re-created with an identical state between two sweeps continues its
 *   age.  Harmless: pausing a caught-up group is always safe, and the reference force-pauses active instances itself.
 *   (Two states with one signature - probability 2^-32 per comparison - have the same effect.)
 * _dev form.  Every pointer is a DEVICE pointer (counts too; gidx nullable).  Asynchronous on the stream
 *   gpx_election_begin_dev uses: three launches ordered by the stream alone, no workgroup waits for another one.
 * Host twin.  Every pointer is host memory.  Runs the _dev form into engine-owned device memory, copies `counts`,
 *   then min(n_hits, cap) entries per column, as the twins of gpx_scan.h do: 105 bytes per paused group plus 16 cross
 *   the link (and gidx when given).  Synchronous.
 * Errors.  All argument checks come before any device work and before the handle is used:
 *   GPX_EINVAL     null handle, negative n / cap, min_age outside 0..255, unknown flag bits, null counts, cap > 0
 *                  with a null column
 *   GPX_ECAPACITY  n above max(max_groups, max_batch)
 *   GPX_ENOMEM     the sweep's words could not be allocated
 */
#ifndef GPX_SWEEP_H
#define GPX_SWEEP_H

#include "gpx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpx_sweep_counts { /* 16 bytes, always written whole */
  int32_t n_hits;                 /* hits found; may exceed cap */
  int32_t n_nogroup;              /* scanned entries that name no live group */
  int32_t n_busy;                 /* live groups gpx_group_retire(PAUSE) would refuse with GPX_S_BUSY */
  int32_t n_paused;               /* groups this call paused: min(n_hits, cap), 0 under GPX_SWEEP_PEEK */
} gpx_sweep_counts;

#define GPX_SWEEP_PEEK 1 /* report only: no group is paused, no age or signature word changes */
#define GPX_SWEEP_HOLD 2 /* not a period: a changed group's age is reset, an unchanged one's is kept, not incremented */

int gpx_pause_sweep_dev(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t min_age, int32_t flags, int32_t cap,
                        int32_t* o_gidx, uint8_t* o_age, gpx_hri* o_rows, gpx_sweep_counts* counts);
int gpx_pause_sweep(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t min_age, int32_t flags, int32_t cap,
                    int32_t* o_gidx, uint8_t* o_age, gpx_hri* o_rows, gpx_sweep_counts* counts);

#ifdef __cplusplus
}
#endif
#endif /* GPX_SWEEP_H */
