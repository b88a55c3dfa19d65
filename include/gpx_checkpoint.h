/*
 * gpx_checkpoint.h — checkpoint transfer: jump lagging acceptors forward on the device.
 *
 * PaxosInstanceStateMachine.handleCheckpoint (PISM:1852-1879) is what a replica does with the StatePacket that answers
 * its checkpoint request (handleCheckpointRequest, PISM:2604-2640) when it has fallen behind further than its peers'
 * decision logs reach: restore the app state, PaxosAcceptor.jumpSlot (PaxosAcceptor.java:564-578) to the slot after the
 * checkpoint, then extractExecuteAndCheckpoint(null) to release what was parked above it.  gpx_checkpoint_batch is
 * the acceptor's half of that as one call: a node that comes back is behind in every group it hosts at once.
 *
 * Records.  Record i < n is one StatePacket(slotNumber = cp_slot[i]) for group gidx[i].  The packet's ballot and state
 *   never reach the acceptor (PISM:1860-1866 hand them to the logger), so they are not arguments.  Records must name
 *   pairwise distinct groups (not checked, as for gpx_pause_sweep and gpx_election_begin_dev): a host has at most one
 *   checkpoint per group in hand.  n above max(max_groups, max_batch) is refused with GPX_ECAPACITY.
 * Evaluation of a record, in this order:
 *   out of range or dead   status = GPX_S_NOGROUP, o_from = o_to = o_flags = 0; counted in n_nogroup.
 *   stopped group          status = GPX_S_STOPPED (PISM:456-460), the outputs are 0; counted in n_stopped; nothing
 *                          changes.
 *   otherwise              status = GPX_S_OK, o_from = the acceptor's slot, then:
 *   1. adopt = cp_slot >= slot: the PLAIN signed comparison of PISM:1853, not the subtraction idiom.
 *   2. if adopt: target = cp_slot + 1 (wrapping) and d = target - slot (wrapping: jumpSlot's loop is `i - slotNumber
 *      < 0`).  d > 0: every committedRequests entry whose slot lies in [slot, target) is removed; with
 *      GPX_F_ACCEPTS_FROM_DISK every acceptedProposals entry in that range too (without the flag they stay); the slot
 *      becomes target; the accepted-GC slot, the ballot and every coordinator word are untouched.  d <= 0 (the plain
 *      and the wrapping comparison disagree: a slot just past Integer.MIN_VALUE and a positive checkpoint): nothing
 *      moves, as in the Java with assertions off; reproduced, not repaired.
 *   3. always, adopted or not, extractExecuteAndCheckpoint(null): while the group is not stopped and a commit is
 *      parked at its slot, collect accepted pvalues by THAT commit's median (putAndRemoveNextExecutable's
 *      `decision == null` branch, PaxosAcceptor.java:329-338), then reconstructDecision; if that yields nothing the
 *      loop ends (the collection has happened); otherwise the slot executes exactly as for gpx_commit_batch (a stop
 *      clears the committed ring and ends the loop; under the flag the accepted entry goes).  The slots executed are ONE
 *      run (gidx, first = the slot after step 2, count).
 *   4. o_to = the slot afterwards; o_flags = GPX_CP_ADOPT if step 1 said so | GPX_CP_MOVED if the slot changed.
 * Runs leave compacted in ascending record index, x_*[0 .. n_runs); each column holds n entries; nothing at or beyond
 *   n_runs is touched.  `counts` is always written whole.
 * GPX_CP_PEEK.  Steps 1 and 2 are evaluated and nothing is stored: o_to is the slot step 2 would leave, MOVED is set
 *   iff step 2 would move it, no tail is evaluated, n_runs = 0, the run columns may be null.  This is how a host keeps
 *   the reference's order - restore() comes before jumpSlot, and nothing happens if it fails: peek, restore the app
 *   state of the ADOPT records, then apply the records whose restore succeeded.
 * Cost.  O(window) per record whatever the distance: fewer than `window` slots are walked, a longer jump tests the
 *   `window` ring entries by subtraction.
 * _dev form.  Every pointer is a DEVICE pointer (counts too).  Asynchronous on the stream gpx_election_begin_dev uses:
 *   three launches ordered by the stream alone, no workgroup waits for another one.
 * Host twin.  Every pointer is host memory.  Runs the _dev form into engine-owned device memory, copies `counts`, then
 *   n dense entries and n_runs run entries per column: 8 bytes in and 10 out per record, 12 per run, 16 of counts.
 *   Synchronous.
 * Errors.  All argument checks come before any device work and before the handle is used:
 *   GPX_EINVAL     null handle, negative n, unknown flag bits, null gidx / cp_slot / o_from / o_to / o_flags / status /
 *                  counts, a null run column without GPX_CP_PEEK
 *   GPX_ECAPACITY  n above max(max_groups, max_batch)
 *   GPX_ENOMEM     the call's scratch could not be allocated (the engine stays usable)
 *   n == 0 writes `counts` and returns GPX_OK.
 */
#ifndef GPX_CHECKPOINT_H
#define GPX_CHECKPOINT_H

#include "gpx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpx_cp_counts { /* 16 bytes, always written whole */
  int32_t n_adopted;           /* records whose checkpoint the reference would restore (GPX_CP_ADOPT) */
  int32_t n_nogroup;           /* records that name no live group */
  int32_t n_stopped;           /* records of stopped groups (PISM:456-460) */
  int32_t n_runs;              /* execution runs written */
} gpx_cp_counts;

#define GPX_CP_PEEK 1  /* call flag: report only, no state word changes, no run is written, n_runs = 0 */
#define GPX_CP_ADOPT 1 /* o_flags: cp_slot >= _slot as PISM:1853 compares - the app restore is due */
#define GPX_CP_MOVED 2 /* o_flags: _slot changed (jump and / or the execution tail) */

int gpx_checkpoint_batch_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* cp_slot, int32_t flags,
                             int32_t* o_from, int32_t* o_to, uint8_t* o_flags, uint8_t* status, int32_t* x_gidx,
                             int32_t* x_first, int32_t* x_count, gpx_cp_counts* counts);
int gpx_checkpoint_batch(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* cp_slot, int32_t flags,
                         int32_t* o_from, int32_t* o_to, uint8_t* o_flags, uint8_t* status, int32_t* x_gidx,
                         int32_t* x_first, int32_t* x_count, gpx_cp_counts* counts);

#ifdef __cplusplus
}
#endif
#endif /* GPX_CHECKPOINT_H */
