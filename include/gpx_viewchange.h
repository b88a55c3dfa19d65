/*
 * gpx_viewchange.h — the view change in list form: prepare and prepare-reply results compacted on the device.
 *
 * gpx_prepare_batch and gpx_prepare_reply_batch (include/gpx.h) return their variable-length results as `window` dense
 * planes of n entries: 12 and 14 bytes x window per record, whatever the lists hold.  The calls below run the same
 * evaluation and hand the results back as LISTS: the acceptor's accepted pvalues as (pv_off, pv_slot, pv_bnum,
 * pv_bcoord) - column for column the pv_* input of the coordinator calls - and the coordinator's results as one 22-byte
 * row per HIT plus one 14-byte row per list entry.  The dense calls and their results do not change; THE DENSE CALL IS
 * THE SPECIFICATION of everything here (HIP library only: the CPU oracle keeps the dense calls).
 *
 * A. gpx_prepare_lists[_dev] - acceptor side
 *   State and dense columns.  The state effect and r_bnum, r_bcoord, r_gc, r_flags, status are exactly
 *     gpx_prepare_batch_dev's, for all n records, whatever cap_entries is (only the acceptor's ballot changes).
 *   Lists.  Record i's list holds the pvalues the dense call marks in p_mask[i], at pv_*[pv_off[i] .. pv_off[i+1]), in
 *     record order; inside a record in ascending SIGNED slot (PrepareReplyPacket.accepted is a TreeMap<Integer, ...>),
 *     not in ring-index order.  NACKed and dropped records have empty lists.
 *   Cut.  Record i is complete iff its list ends at or before cap_entries; recs_done is the number of leading complete
 *     records.  pv_off[0 .. recs_done] is written, pv_off[recs_done] == entries_done, and nothing at or beyond those
 *     indices is touched.  cap_entries == 0 with null pv_off / pv_slot / pv_bnum / pv_bcoord counts only.  Records at or
 *     after recs_done are answered by REPEATING THEIR PREPARE through either call: a PREPARE at a ballot that is not
 *     strictly greater changes nothing and returns the same pvalues (PaxosAcceptor.java:246-252).
 *   Chaining.  With recs_done == n, (pv_off, pv_slot, pv_bnum, pv_bcoord) are valid pv_* inputs of
 *     gpx_prepare_reply_batch_dev / gpx_prepare_reply_lists_dev as they stand, with pv_total = cap_entries or
 *     entries_done.
 *   Scratch.  8 bytes per record of max_batch, allocated by the first such call.  No planes exist anywhere.
 *
 * B. gpx_prepare_reply_lists[_dev] - coordinator side
 *   State effect.  Exactly gpx_prepare_reply_batch_dev's, for all records, whatever the caps.
 *   Hit.  A record with status != GPX_S_OK, or with v_kind GPX_V_ELECTED or GPX_V_PREEMPTED.  RECORDED and IGNORED
 *     records produce no row; the optional dense v_kind and status columns (n entries, 1 byte each, null = not wanted)
 *     carry them for a host that wants them.
 *   Order and content.  Hits leave in ascending record index; h_rec is that index, h_gidx its group, h_kind / h_status /
 *     h_median / h_count the dense v_kind[i] / status[i] / e_median[i] / e_count[i].  A hit's entries are the dense
 *     planes j = 0 .. e_count-1 in that order (ascending slot, the order spawnCommandersForProposals uses), at
 *     e_*[h_off .. h_off + h_count); h_off counts from the first entry THIS CALL writes.
 *   Cut.  Hit number q, counted from from_hit (0 here), fits iff q < cap_hits and h_off + h_count <= cap_entries.  The
 *     first hit that does not fit ends the output; nothing at or beyond hits_done / entries_done is touched.  Caps of 0
 *     with null columns count only.  h_count <= window, so cap_entries >= window (and cap_hits >= 1) GUARANTEES PROGRESS.
 *   Scratch.  The call runs the dense _dev call into engine-owned scratch - the four dense columns plus the `window`
 *     planes, (10 + 14 * window) bytes per record of max_batch, which is what a _dev caller allocates today - plus
 *     16 bytes per record for the parked hits.  One block, allocated by the first call; GPX_ENOMEM leaves the engine
 *     usable.
 *
 * C. gpx_prepare_reply_lists_more[_dev] - continuation
 *   The parked planes and per-tile words of the last gpx_prepare_reply_lists* call stay valid until the next such call
 *   on the engine (acceptor calls use a separate block and do not disturb them).  _more writes the hits from from_hit
 *   on under the same fit rule, h_off again counted from this call's first entry; the class counts are echoed;
 *   from_hit >= n_hits writes nothing.  With no such call before it: GPX_EINVAL.  gpx_prepare_reply_lists itself is
 *   "apply, then _more(0)".
 *
 * _dev forms.  Every pointer is a DEVICE pointer (counts too).  Asynchronous on the engine's stream, ordered by the
 *   stream alone: no workgroup waits for another one.
 * Host twins (the names without _dev).  Every pointer is host memory; synchronous.  They run the _dev form into
 *   engine-owned staging, copy the counts, then only what was written: nothing proportional to n x window crosses the
 *   link.  The coordinator twin runs _more rounds internally until the caller's caps are reached; h_off is relative to
 *   the caller's arrays.
 * Errors.  All argument checks come before any device work and before the handle is used:
 *   GPX_EINVAL     null handle or counts, negative n / cap / from_hit, a cap > 0 with a null column, null required
 *                  inputs (n > 0), _more with nothing parked
 *   GPX_ECAPACITY  n > max_batch
 *   GPX_ENOMEM     the scratch could not be allocated: the engine stays usable
 */
#ifndef GPX_VIEWCHANGE_H
#define GPX_VIEWCHANGE_H

#include "gpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPX_VCL_TILE 256 /* records one workgroup compacts: the tests place their edge cases on it */

typedef struct gpx_pl_counts { /* 32 bytes */
  int32_t n_entries;           /* pvalues found; may exceed cap_entries */
  int32_t recs_done;           /* leading records whose lists are complete */
  int32_t entries_done;        /* == pv_off[recs_done] */
  int32_t n_dropped;           /* status != GPX_S_OK */
  int32_t n_nack;              /* r_flags & GPX_P_NACK */
  int32_t n_tolog;             /* r_flags & GPX_P_TOLOG */
  int32_t reserved[2];         /* written as 0 */
} gpx_pl_counts;

typedef struct gpx_prl_counts { /* 32 bytes */
  int32_t n_hits;               /* hits found; may exceed the caps */
  int32_t n_entries;            /* list entries of all hits */
  int32_t from_hit;             /* the first hit this call was asked for */
  int32_t hits_done;            /* hit rows written */
  int32_t entries_done;         /* entry rows written */
  int32_t n_elected;            /* v_kind == GPX_V_ELECTED */
  int32_t n_preempted;          /* v_kind == GPX_V_PREEMPTED */
  int32_t n_dropped;            /* status != GPX_S_OK */
} gpx_prl_counts;

int gpx_prepare_lists_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* bnum, const int32_t* bcoord,
                          const int32_t* first_slot, int32_t* r_bnum, int32_t* r_bcoord, int32_t* r_gc,
                          uint8_t* r_flags, uint8_t* status, int32_t cap_entries, int32_t* pv_off, int32_t* pv_slot,
                          int32_t* pv_bnum, int32_t* pv_bcoord, gpx_pl_counts* counts);
int gpx_prepare_lists(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* bnum, const int32_t* bcoord,
                      const int32_t* first_slot, int32_t* r_bnum, int32_t* r_bcoord, int32_t* r_gc, uint8_t* r_flags,
                      uint8_t* status, int32_t cap_entries, int32_t* pv_off, int32_t* pv_slot, int32_t* pv_bnum,
                      int32_t* pv_bcoord, gpx_pl_counts* counts);

int gpx_prepare_reply_lists_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* acceptor,
                                const int32_t* r_bnum, const int32_t* r_bcoord, const int32_t* first_slot,
                                const int32_t* pv_off, int32_t pv_total, const int32_t* pv_slot, const int32_t* pv_bnum,
                                const int32_t* pv_bcoord, const int64_t* pv_handle, const uint8_t* pv_flags,
                                uint8_t* v_kind, uint8_t* status, int32_t cap_hits, int32_t cap_entries, int32_t* h_rec,
                                int32_t* h_gidx, uint8_t* h_kind, uint8_t* h_status, int32_t* h_median, int32_t* h_off,
                                int32_t* h_count, int32_t* e_slot, uint8_t* e_kind, int64_t* e_handle, uint8_t* e_flags,
                                gpx_prl_counts* counts);
/* the host twin takes no pv_total: pv_off[n] says it, as for gpx_prepare_reply_batch */
int gpx_prepare_reply_lists(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* acceptor,
                            const int32_t* r_bnum, const int32_t* r_bcoord, const int32_t* first_slot,
                            const int32_t* pv_off, const int32_t* pv_slot, const int32_t* pv_bnum,
                            const int32_t* pv_bcoord, const int64_t* pv_handle, const uint8_t* pv_flags, uint8_t* v_kind,
                            uint8_t* status, int32_t cap_hits, int32_t cap_entries, int32_t* h_rec, int32_t* h_gidx,
                            uint8_t* h_kind, uint8_t* h_status, int32_t* h_median, int32_t* h_off, int32_t* h_count,
                            int32_t* e_slot, uint8_t* e_kind, int64_t* e_handle, uint8_t* e_flags,
                            gpx_prl_counts* counts);

int gpx_prepare_reply_lists_more_dev(gpx_engine* h, int32_t from_hit, int32_t cap_hits, int32_t cap_entries,
                                     int32_t* h_rec, int32_t* h_gidx, uint8_t* h_kind, uint8_t* h_status,
                                     int32_t* h_median, int32_t* h_off, int32_t* h_count, int32_t* e_slot,
                                     uint8_t* e_kind, int64_t* e_handle, uint8_t* e_flags, gpx_prl_counts* counts);
int gpx_prepare_reply_lists_more(gpx_engine* h, int32_t from_hit, int32_t cap_hits, int32_t cap_entries, int32_t* h_rec,
                                 int32_t* h_gidx, uint8_t* h_kind, uint8_t* h_status, int32_t* h_median, int32_t* h_off,
                                 int32_t* h_count, int32_t* e_slot, uint8_t* e_kind, int64_t* e_handle, uint8_t* e_flags,
                                 gpx_prl_counts* counts);

#ifdef __cplusplus
}
#endif
#endif /* GPX_VIEWCHANGE_H */
