/*
 * gpx_scan.h — table scans that return only their hits, compacted on the device.
 *
 * gpx_election_scan, gpx_poke_scan and gpx_gap_scan (include/gpx.h) write one dense row per scanned entry, and every
 * row travels to the host: 10, 22 and 22 bytes per group, whatever the rows say.  The host then skips every row that
 * is not a hit.  The calls below run the same evaluation and hand back ONLY THE HITS, compacted in entry order, with
 * the count in a gpx_scan_counts: 13, 26 and 21 bytes per hit plus 16 bytes of counts.  The dense calls and their
 * results do not change; THE DENSE CALL'S ROW IS THE SPECIFICATION of everything here.
 *
 * Scanned entries.  Entry i < n is group gidx[i], or group i when gidx == NULL (allowed for all three scans).
 *   n above max(max_groups, max_batch) is refused with GPX_ECAPACITY.
 * Hit.  An entry whose dense row has
 *   election: status == GPX_S_OK and run != GPX_RUN_NO
 *   poke:     status == GPX_S_OK and poke != GPX_POKE_NONE
 *   gap:      status == GPX_S_OK and every condition selected in `require` (GPX_GAP_HIT_*, all must hold; 0 = every
 *             live, not stopped group).  A stopped group (GPX_S_STOPPED) is never a hit.
 * Output.  Hits leave in ascending entry index i: for a whole-table scan ascending gidx, the ORDER rule of gpx.h.
 *   Hit j carries o_gidx[j] = its group; the other columns hold exactly what the dense call writes at i.  Only the
 *   first min(n_hits, cap) entries of each column are written and nothing at or beyond that index is touched.
 *   cap == 0 with null columns is legal and counts only; with cap > 0 every column must be given.  `counts` is always
 *   written whole: n_hits is the number of hits FOUND (it may exceed cap), n_nogroup the scanned entries whose dense
 *   status is GPX_S_NOGROUP.
 * _dev forms.  Every pointer except the node lists is a DEVICE pointer (counts too; gidx nullable).  Asynchronous on
 *   the stream gpx_election_begin_dev uses; no state changes.  A call is three launches ordered by the stream alone:
 *   no workgroup waits for another one.
 * Host twins (the names without _dev).  Every pointer is host memory, `counts` a host struct.  They run the _dev form
 *   into engine-owned device memory, copy `counts`, then copy min(n_hits, cap) entries per column (registered blocks
 *   by DMA, pageable memory in pieces, as every host-pointer call): nothing proportional to n crosses the link except
 *   gidx when given.  Synchronous.
 * Errors.  All argument checks come before any device work and before the handle is used:
 *   GPX_EINVAL     null handle, negative n / cap / list length, null counts, cap > 0 with a null column, a null list
 *                  with a positive length
 *   GPX_ECAPACITY  a node list longer than 16; n above max(max_groups, max_batch)
 *   GPX_ENOMEM     the scan scratch (allocated by the first such call, sized once) could not be allocated: the engine
 *                  stays usable
 */
#ifndef GPX_SCAN_H
#define GPX_SCAN_H

#include "gpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPX_SCAN_TILE 1024 /* groups one workgroup scans: the tests place hits on its edges */

typedef struct gpx_scan_counts { /* 16 bytes */
  int32_t n_hits;                /* hits found; may exceed cap: only the first cap are written */
  int32_t n_nogroup;             /* scanned entries that name no live group (GPX_S_NOGROUP in the dense call) */
  int32_t reserved[2];           /* written as 0 */
} gpx_scan_counts;

/* gap scan: which conditions make a group a hit (all of the selected ones must hold; 0 = every live, not stopped
 * group) */
#define GPX_GAP_HIT_SYNC 1    /* should_sync != 0 */
#define GPX_GAP_HIT_MISSING 2 /* missing != 0 */
#define GPX_GAP_HIT_AHEAD 4   /* max_committed - first_slot >= 0 (Java wraparound compare) */

/* who must run for coordinator (gpx_election_scan): o_run = GPX_RUN_*, o_bnum / o_first = the PREPARE's ballot number
 * and firstUndecidedSlot.  The node lists are HOST arrays in both forms (they travel by value). */
int gpx_election_scan_hits_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* down_nodes,
                               int32_t n_down, const int32_t* long_dead_nodes, int32_t n_long_dead, int32_t force,
                               int32_t cap, int32_t* o_gidx, uint8_t* o_run, int32_t* o_bnum, int32_t* o_first,
                               gpx_scan_counts* counts);
/* which ACCEPT or PREPARE is still waiting for replies (gpx_poke_scan) */
int gpx_poke_scan_hits_dev(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t cap, int32_t* o_gidx,
                           uint8_t* o_poke, int32_t* o_slot, int32_t* o_bnum, int32_t* o_bcoord,
                           int32_t* o_median_cp, uint8_t* o_flags, uint32_t* o_heard, gpx_scan_counts* counts);
/* who has a decision gap (gpx_gap_scan) */
int gpx_gap_scan_hits_dev(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t threshold, int32_t sync_mode,
                          int32_t size_limit, int32_t require, int32_t cap, int32_t* o_gidx, int32_t* o_first,
                          int32_t* o_max_committed, uint64_t* o_missing, uint8_t* o_sync, gpx_scan_counts* counts);

/* host-pointer twins */
int gpx_election_scan_hits(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* down_nodes, int32_t n_down,
                           const int32_t* long_dead_nodes, int32_t n_long_dead, int32_t force, int32_t cap,
                           int32_t* o_gidx, uint8_t* o_run, int32_t* o_bnum, int32_t* o_first,
                           gpx_scan_counts* counts);
int gpx_poke_scan_hits(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t cap, int32_t* o_gidx, uint8_t* o_poke,
                       int32_t* o_slot, int32_t* o_bnum, int32_t* o_bcoord, int32_t* o_median_cp, uint8_t* o_flags,
                       uint32_t* o_heard, gpx_scan_counts* counts);
int gpx_gap_scan_hits(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t threshold, int32_t sync_mode,
                      int32_t size_limit, int32_t require, int32_t cap, int32_t* o_gidx, int32_t* o_first,
                      int32_t* o_max_committed, uint64_t* o_missing, uint8_t* o_sync, gpx_scan_counts* counts);

/*
 * gpx_election_begin_dev for the first min(counts->n_hits, cap) entries of (gidx, bnum) - a scan's o_gidx / o_bnum
 * and its counts, all in device memory, the count read ON THE DEVICE: scan -> begin with no host round trip.  The
 * effect is gpx_election_begin_dev's entry for entry; e_status holds cap entries and only the first
 * min(n_hits, cap) are written.  The entries must be pairwise distinct, as for gpx_election_begin_dev (the output of
 * a scan with gidx == NULL is distinct by construction).  GPX_EINVAL: null handle, cap < 0, a null pointer with
 * cap > 0; GPX_ECAPACITY: cap above max(max_groups, max_batch).
 */
int gpx_election_begin_hits_dev(gpx_engine* h, int32_t cap, const gpx_scan_counts* counts, const int32_t* gidx,
                                const int32_t* bnum, uint8_t* e_status);

#ifdef __cplusplus
}
#endif
#endif /* GPX_SCAN_H */
