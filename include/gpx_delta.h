/*
 * gpx_delta.h — delta images: export only the groups that changed since the export that last wrote them, and apply
 * such a delta to a table whose groups may already exist.
 *
 * Group images (gpx_image.h) move the complete state of any group; every snapshot of a table moves every live group.
 * A table of millions of groups of which few are busy wants the other thing: a standby copy (a second engine, host
 * memory, a file) kept current at a cost that follows the number of groups that changed, and a live move by pre-copy
 * (copy everything, copy what changed meanwhile, repeat, stop the traffic for the last small round only).  The rows
 * are the rows of gpx_image.h, byte for byte; this header adds "since last time".
 *
 * Marks.  One 64-bit word per group, an array over max_groups that the engine owns.  The first delta export
 *   allocates it, zeroed (GPX_ENOMEM if it cannot; the engine stays usable); no other call reads or writes it, and
 *   it does not outlive the engine.  0 = no export has written this group; otherwise the mark is a signature of the
 *   group's state at the export that last wrote it.  The signature is a function of exactly the words of the
 *   group's rows as gpx_group_export would write them - the main row and, for a group that is running for
 *   coordinator, the continuation row, both without padding - and of nothing else.  It is therefore a function of
 *   the canonical state (gpx_group_dump): a stale word under a clear present bit never makes a group "changed", and
 *   a group that was retired and created again in the same logical state is unchanged.  (The source gidx is a word
 *   of the row: the mark of row g speaks of row g.)
 *   The signature is 64 bits wide, two independently seeded 32-bit streams over the same words, forced non-zero.
 *   THE ONE PROBABILISTIC STATEMENT OF THESE CALLS: a group whose state changed is reported unchanged only if the
 *   two signatures collide, about 2^-64 per changed group and export.  Everything else below is exact.  The hash is
 *   internal and may change between versions of the library.
 *
 * Export.  Entries, gidx == NULL, the limit on n (GPX_ECAPACITY above max(max_groups, max_batch)), pairwise distinct
 *   listed entries (not checked), compaction in ascending entry order, adjacency of a group's two rows, and "no
 *   group in part, nothing at or beyond the last written row is touched" read as in gpx_image.h.  Per entry:
 *     live, and its signature differs from its mark - or any live entry under GPX_DELTA_FULL: the group is CHANGED
 *       and needs one or two rows.  The groups written are the longest prefix of the changed entries whose rows all
 *       fit `cap`.  The mark of a group written becomes its signature; a group that did not fit keeps its mark, so
 *       the next call reports it again.
 *     in range, not live, mark non-zero: the group is GONE.  Its group index goes to o_gone, compacted in ascending
 *       entry order, while it fits cap_gone; the mark of one written becomes 0.
 *     anything else writes nothing.
 *   cap == 0 with a null o_rows and cap_gone == 0 with a null o_gone only count and change no mark.
 *   GPX_DELTA_EVICT retires exactly the groups written, as GPX_IMG_EVICT does, zeroes the deactivation sweep's idle
 *   words for them and sets their marks to 0: they are not reported gone afterwards.
 *   The rows written are byte for byte what gpx_group_export writes for the same groups in the current state.
 *   `counts` is always written whole.
 * Apply.  The rows are handled as by gpx_group_import: the checks, their order, the statuses and "a refused group
 *   writes nothing at all" are the import's, with one difference: a destination that is ALIVE IS REPLACED, not
 *   refused (no row answers GPX_S_EXISTS).  Every state word of the destination is written, the election words
 *   zeroed where the new state has none and the arrays are allocated; the wire codec's copies and the sweep's idle
 *   words are treated as by the import.  A refused row leaves a live destination exactly as it was.  status is
 *   required when n_rows > 0.
 *   Then each gone[i] that is in range and alive is retired as gpx_group_retire(GPX_RETIRE_KILL) does and its sweep
 *   idle words are zeroed, gone_status[i] = GPX_S_OK; every other entry gets GPX_S_NOGROUP and changes nothing.
 *   gone_status is required when n_gone > 0.  n_gone above max(max_groups, max_batch): GPX_ECAPACITY.
 *   Row destinations and gone entries must be pairwise distinct TOGETHER (not checked).
 *   flags: GPX_IMG_VIEWCHANGE only, as for the import (pass it when the export's n_rows_done > n_done).
 *   The marks of the engine a delta is applied to are not touched: marks describe what an engine has EXPORTED.
 * _dev forms.  Every pointer is a DEVICE pointer (counts, status, gone_status too; gidx nullable); o_rows / rows
 *   16-byte aligned, o_gone / gone 4-byte aligned, else GPX_EINVAL.  Asynchronous on the stream the image calls use:
 *   launches ordered by the stream alone, no workgroup waits for another one.
 * Host twins.  Every pointer is host memory; synchronous; through the engine-owned staging of the image calls (at
 *   most 64 MiB), a larger request in consecutive chunks whose result equals one call.
 * Errors.  All argument checks come before any device work and before the handle is used:
 *   GPX_EINVAL     null handle, negative n / cap / cap_gone / n_rows / n_gone, unknown flag bits, null counts, a
 *                  positive cap / cap_gone / n_rows / n_gone with its buffer (or status column) null, a misaligned
 *                  _dev buffer
 *   GPX_ECAPACITY  n / n_rows / n_gone above the limit
 *   GPX_ENOMEM     marks, scratch or staging could not be allocated (the engine stays usable)
 */
#ifndef GPX_DELTA_H
#define GPX_DELTA_H

#include "gpx_image.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpx_delta_counts { /* 32 bytes, always written whole */
  int32_t n_live;                 /* scanned entries that name a live group */
  int32_t n_changed;              /* of those, groups whose state differs from their mark */
  int32_t n_rows;                 /* rows all changed groups need; may exceed cap */
  int32_t n_done;                 /* groups written */
  int32_t n_rows_done;            /* rows written */
  int32_t n_gone;                 /* scanned entries that are dead but still carry a mark */
  int32_t n_gone_done;            /* of those, written to o_gone */
  int32_t reserved;               /* 0 */
} gpx_delta_counts;

#define GPX_DELTA_EVICT 1 /* retire the groups written, as GPX_IMG_EVICT does */
#define GPX_DELTA_FULL 2  /* treat every scanned live group as changed: a baseline */

int gpx_group_export_delta_dev(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t flags, int32_t cap, void* o_rows,
                               int32_t cap_gone, int32_t* o_gone, gpx_delta_counts* counts);
int gpx_group_export_delta(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t flags, int32_t cap, void* o_rows,
                           int32_t cap_gone, int32_t* o_gone, gpx_delta_counts* counts);

int gpx_group_apply_delta_dev(gpx_engine* h, int32_t n_rows, const void* rows, const int32_t* gidx, int32_t flags,
                              uint8_t* status, int32_t n_gone, const int32_t* gone, uint8_t* gone_status);
int gpx_group_apply_delta(gpx_engine* h, int32_t n_rows, const void* rows, const int32_t* gidx, int32_t flags,
                          uint8_t* status, int32_t n_gone, const int32_t* gone, uint8_t* gone_status);

#ifdef __cplusplus
}
#endif
#endif /* GPX_DELTA_H */
