/*
 * gpx_logindex.h — the log index on the device: where every logged ACCEPT lies, by group.
 *
 * gpx_journal_pack (gpx_journal.h) writes a batch of the journal and hands out LogIndex.add's arguments as rows;
 * gpx_journal_gc (gpx_journal_gc.h) compacts a file from such rows.  This header KEEPS the rows: the reference's
 * MessageLogDiskMap (SQLPaxosLogger.java:367-490) with one paxosutil/LogIndex per group, as ONE flat table in device
 * memory keyed by gidx.  It is fed by the pack's row columns (add), garbage collected by batches of checkpoint slots
 * (set_gc), queried by batches of slot ranges (lookup), hands gpx_journal_gc_dev its input (file_rows), takes that
 * call's output back (relocate) and answers the file-deletion questions (files).  Only ACCEPT entries are in scope:
 * ACCEPT is the only log message with a byte form (gpx_journal.h).
 *
 * The reference (the specification).  A group's LogIndex is gcSlot (initially -1), minLogfile (initially null) and an
 * ArrayList of entries (slot, bnum, bcoord, file, offset, length) in arrival order.
 *   add (LogIndex.java:192-204)          refused iff slot - gcSlot <= 0 in wrapping int arithmetic; otherwise minLogfile
 *                                        becomes the entry's file if it was null, and the entry is appended.
 *   setGCSlot / GC (:128-152)            gcSlot = gc unconditionally - it may move backwards, and removed entries stay
 *                                        removed; entries with slot - gc <= 0 are removed, the order is kept; minLogfile
 *                                        becomes the first remaining entry's file, or null.  Called from
 *                                        SQLPaxosLogger.java:1481 and :2717.
 *   getLoggedAccepts (:213-237)          the entries with slot - min >= 0 and (max == null or slot - max <= 0), in list
 *                                        order; getLoggedFromMessageLog (SQLPaxosLogger.java:3639-3760) then puts them
 *                                        in a map by slot, so for equal slots the later list entry wins: the caller
 *                                        does that.
 *   modify (:174-186)                    replaces file, offset and length of the first entry with the same (slot, bnum,
 *                                        bcoord, type); does not touch minLogfile.  modifyLogIndexEntry,
 *                                        SQLPaxosLogger.java:480-489 and :3443-3458.
 *   getMinLogfile (:319-322)             null for an empty list.     getLogfiles (:253-259).
 *   isLogMsgNeeded (:331-345)            the ACCEPT branch is slot - gcSlot > 0.
 *   FileIDMap.isRemovable over getMinLogfile, SQLPaxosLogger.java:3174-3207; the roll-forward point, :2725-2744.
 *   A new version: getOrCreateIfNotExistsOrLower replaces the group's index by a fresh one (GPX_LI_RESET).
 *
 * Files are int32 ids that the caller assigns in creation order, -1 for null.  The reference's Filename.compareTo
 * orders by creation, so comparing files is comparing ids.
 *
 * State.  Engine-owned, allocated by gpx_logindex_open(h, cap_rows), cap_rows in [1, 2^31 - 512].  Without open every
 *   other call answers GPX_EINVAL; a second open answers GPX_EINVAL; an allocation failure answers GPX_ENOMEM and leaves
 *   the engine usable (and the index not open).
 *   ONE flat table of up to cap_rows rows in append order: gidx, slot, bnum, bcoord, file, off (int64), len and a
 *   liveness mark; a second block of the same columns for compact.  Per group of max_groups: the GC slot (initially
 *   -1), the min file (initially -1) and one arming word with its companion.  The table's tail, the alive count and the
 *   generation live in device memory.  A per-group list of fixed capacity would be the wrong shape - a group holds
 *   everything since its last checkpoint, CHECKPOINT_INTERVAL = 400 slots by default - and a flat table in log order is
 *   what the pack already produces: within a group the table's order IS LogIndex's list order.
 *   The index is keyed by gidx in [0, max_groups) and does not look at whether the group exists: the reference's index
 *   outlives the instance too.  IT IS NOT GROUP STATE: images, deltas, dumps, snapshots and the sweeps neither see nor
 *   touch it, and no call of this header reads or writes a group.
 * Forms.  Every call has a _dev form - all pointers device memory, the counts too; queued on the engine's back-end
 *   stream behind every call made before it, with no host round trip; no workgroup waits for another one - and a
 *   synchronous host-pointer twin that copies the columns in and copies back the counts and only what was written.
 * Counts.  One struct of eight int32, 32 bytes, ALWAYS WRITTEN WHOLE.  n_rows: the table's tail after the call.
 *   n_alive: the alive rows after the call.  generation: the index's generation after the call.  A call that has no
 *   meaning for one of the other fields writes 0 there.
 * Status bytes.  GPX_LI_ADDED (0; for set_gc and lookup: the record applies), GPX_LI_STALE, GPX_LI_NOGROUP,
 *   GPX_LI_FULL, GPX_LI_REPEAT.  `status` may be NULL in every call.
 *
 * 1. add.  The row columns are gpx_journal_pack_dev's e_* outputs as they stand; `file` (>= 0) is the file the batch
 *   went to.  n_dev may be NULL; otherwise it is a device (twin: host) int32 and the call takes min(n, max(*n_dev, 0))
 *   records: pointing it at the pack's counts.n_done chains pack -> add with no copy to the host.  Per record taken:
 *     GPX_LI_NOGROUP  gidx outside [0, max_groups) (n_nogroup)
 *     GPX_LI_STALE    (int32)(slot - gc[g]) <= 0; nothing changes (n_stale)
 *     GPX_LI_ADDED    appended, in record order; sets the group's min file to `file` iff it was -1
 *     GPX_LI_FULL     the table has no room; nothing changes
 *   The added records are a prefix of the addable ones; n_done is their number.  A FULL record changes nothing, so
 *   after a compact the caller repeats from the first FULL record.  Records beyond the ones taken get no status.
 * 2. set_gc.  The FIRST record that names a group applies; later records of the same group get GPX_LI_REPEAT, count in
 *   n_repeat and do nothing - the caller sends them in its next call, which is setGCSlot twice.  For an applied record
 *   gc[g] = gc_slot, smaller or not; every alive row of g with (int32)(slot - gc_slot) <= 0 dies (n_stale counts
 *   them); the group's min file becomes the file of its first alive row in table order, or -1.  n_done: the applied
 *   records.  GPX_LI_RESET is a call-wide flag: every alive row of the named groups dies, gc = -1 and the min file is
 *   -1 - the fresh LogIndex of a new version; gc_slot may then be NULL.
 * 3. lookup.  getLoggedAccepts for a batch: the hits are the alive rows of a queried group inside its range, tested by
 *   the two wrapping comparisons above; has_max[i] == 0 (or has_max == NULL) means maxSlot == null.  Hits are compacted
 *   in TABLE order, which within a group is list order; o_rec is the querying record, o_row the table row.  n_hits
 *   counts all hits, the first min(n_hits, cap) are written (n_done) and nothing at or beyond that.  The call changes
 *   no index state, so a cut call is repeated with a larger cap; cap == 0 with null outputs counts only.  A group
 *   queried twice follows the REPEAT rule of set_gc.
 * 4. file_rows.  The alive rows whose file is `file`, in table order, under the same cap rule.  The six e_* columns are
 *   gpx_journal_gc_dev's row inputs as they stand; e_gc is each row's group's index GC slot: hand it over as cp_slot.
 *   WHY THAT KEEPS EVERY ROW.  A row is alive iff it passed add's test against the GC slot of its time and every set_gc
 *   since, and set_gc's last word is gc[g]: (int32)(slot - gc[g]) > 0 holds for every alive row.  gpx_journal_gc judges
 *   a row of an existing group against min(cp_slot, acceptedGCSlot) in wrapping order: that is cp_slot = gc[g] itself,
 *   or a slot behind it, and slot - threshold = (slot - gc[g]) + (gc[g] - threshold) stays positive while the slots in
 *   play span less than 2^31 - the window every wrapping comparison of the reference assumes.  A row of a group that
 *   does not exist is GPX_JG_KEEP_UNJUDGED.  So every usable row is kept, the file loses exactly the bytes that no
 *   alive row names, and k_src is the identity over the usable rows.
 * 5. relocate.  modifyLogIndexEntry for a compacted or merged file.  o_row holds n entries (file_rows' output).  For
 *   j < min(n, max(*n_dev, 0)) - n_dev as in add: point it at gpx_journal_gc's counts.n_done - the table row
 *   o_row[k_src ? k_src[j] : j] takes (new_file, k_off[j], k_len[j]) iff `generation` equals the index's generation,
 *   k_src[j] is inside [0, n), the row index is inside the table and the row is alive (n_done); otherwise the record
 *   counts in n_stale and nothing is written.  Every index is checked before it is used: garbage is refused, never
 *   followed.  Min files do not change, as in modify.  Two records that name one row are the caller's error (one wins).
 * 6. files.  n_files in [0, 4096].  o_rows[f]: the alive rows of file file_base + f (getLogfiles).  o_groups[f]: the
 *   groups whose min file it is - what FileIDMap.isRemovable asks: no group's min file at or before the file.
 *   *o_min_file: the smallest min file over all groups, or -1 - getMinLogfile(), the roll-forward point.  n_stale
 *   counts the alive rows and the min files outside the id range.  Every output may be NULL.
 * 7. compact.  Moves the alive rows, in order, into the other block, swaps the blocks and sets n_rows = n_alive.  It
 *   increments the generation: row indices handed out before it are void, which is why relocate takes the generation.
 *
 * Deviations.
 *   relocate goes by row identity, the reference by the first entry with equal (slot, ballot).  The two differ only
 *     for a group that logged the same slot at the same ballot twice: there the reference rewrites one entry twice and
 *     leaves the other pointing into a file that no longer exists.
 *   The file-name string becomes a caller-assigned id.
 *   Out of scope: lastActive / isPausable, the DiskMap paging of indexes, PREPARE and DECISION entries and the version
 *     number.  The caller calls set_gc with GPX_LI_RESET when a version changes.
 * Errors.  All argument checks come before any device work:
 *   GPX_EINVAL     null handle or counts; an index that is not open (open: one that is, or cap_rows out of range);
 *                  negative n, cap or n_files, n_files > 4096, file < 0 (add, relocate's new_file); unknown flag bits;
 *                  with n > 0 a null input column (gc_slot only without GPX_LI_RESET; max_slot only with has_max);
 *                  with cap > 0 a null output column
 *   GPX_ECAPACITY  n above max_batch
 *   GPX_ENOMEM     open could not allocate; a host twin could not stage
 */
#ifndef GPX_LOGINDEX_H
#define GPX_LOGINDEX_H

#include "gpx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpx_logindex_counts { /* 32 bytes, always written whole; device memory for the _dev calls */
  int32_t n_rows;                    /* the table's tail after the call */
  int32_t n_alive;                   /* alive rows after the call */
  int32_t generation;                /* the index's generation after the call */
  int32_t n_done;                    /* add: appended; set_gc: applied; lookup, file_rows: written; relocate: rewritten */
  int32_t n_hits;                    /* lookup, file_rows: all hits, written or not */
  int32_t n_stale;                   /* add: refused as stale; set_gc: rows that died; relocate: refused; files: outside */
  int32_t n_nogroup;                 /* records whose gidx is outside [0, max_groups) */
  int32_t n_repeat;                  /* set_gc, lookup: records of a group an earlier record names */
} gpx_logindex_counts;

#define GPX_LI_ADDED 0
#define GPX_LI_STALE 1
#define GPX_LI_NOGROUP 2
#define GPX_LI_FULL 3
#define GPX_LI_REPEAT 4

#define GPX_LI_RESET 1        /* set_gc: the named groups start over */
#define GPX_LI_MAX_FILES 4096 /* files: the largest n_files */

int gpx_logindex_open(gpx_engine* h, int32_t cap_rows);

int gpx_logindex_add_dev(gpx_engine* h, int32_t n, const int32_t* n_dev, const int32_t* e_gidx, const int32_t* e_slot,
                         const int32_t* e_bnum, const int32_t* e_bcoord, const int64_t* e_off, const int32_t* e_len,
                         int32_t file, uint8_t* status, gpx_logindex_counts* counts);
int gpx_logindex_add(gpx_engine* h, int32_t n, const int32_t* n_dev, const int32_t* e_gidx, const int32_t* e_slot,
                     const int32_t* e_bnum, const int32_t* e_bcoord, const int64_t* e_off, const int32_t* e_len,
                     int32_t file, uint8_t* status, gpx_logindex_counts* counts);

int gpx_logindex_set_gc_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* gc_slot, int32_t flags,
                            uint8_t* status, gpx_logindex_counts* counts);
int gpx_logindex_set_gc(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* gc_slot, int32_t flags,
                        uint8_t* status, gpx_logindex_counts* counts);

int gpx_logindex_lookup_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* min_slot,
                            const int32_t* max_slot, const uint8_t* has_max, int32_t cap, int32_t* o_rec, int32_t* o_row,
                            int32_t* o_slot, int32_t* o_bnum, int32_t* o_bcoord, int32_t* o_file, int64_t* o_off,
                            int32_t* o_len, uint8_t* status, gpx_logindex_counts* counts);
int gpx_logindex_lookup(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* min_slot, const int32_t* max_slot,
                        const uint8_t* has_max, int32_t cap, int32_t* o_rec, int32_t* o_row, int32_t* o_slot,
                        int32_t* o_bnum, int32_t* o_bcoord, int32_t* o_file, int64_t* o_off, int32_t* o_len,
                        uint8_t* status, gpx_logindex_counts* counts);

int gpx_logindex_file_rows_dev(gpx_engine* h, int32_t file, int32_t cap, int32_t* o_row, int32_t* e_gidx, int32_t* e_slot,
                               int32_t* e_bnum, int32_t* e_bcoord, int64_t* e_off, int32_t* e_len, int32_t* e_gc,
                               gpx_logindex_counts* counts);
int gpx_logindex_file_rows(gpx_engine* h, int32_t file, int32_t cap, int32_t* o_row, int32_t* e_gidx, int32_t* e_slot,
                           int32_t* e_bnum, int32_t* e_bcoord, int64_t* e_off, int32_t* e_len, int32_t* e_gc,
                           gpx_logindex_counts* counts);

int gpx_logindex_relocate_dev(gpx_engine* h, int32_t n, const int32_t* n_dev, int32_t generation, const int32_t* o_row,
                              const int32_t* k_src, int32_t new_file, const int64_t* k_off, const int32_t* k_len,
                              gpx_logindex_counts* counts);
int gpx_logindex_relocate(gpx_engine* h, int32_t n, const int32_t* n_dev, int32_t generation, const int32_t* o_row,
                          const int32_t* k_src, int32_t new_file, const int64_t* k_off, const int32_t* k_len,
                          gpx_logindex_counts* counts);

int gpx_logindex_files_dev(gpx_engine* h, int32_t file_base, int32_t n_files, int32_t* o_rows, int32_t* o_groups,
                           int32_t* o_min_file, gpx_logindex_counts* counts);
int gpx_logindex_files(gpx_engine* h, int32_t file_base, int32_t n_files, int32_t* o_rows, int32_t* o_groups,
                       int32_t* o_min_file, gpx_logindex_counts* counts);

int gpx_logindex_compact_dev(gpx_engine* h, gpx_logindex_counts* counts);
int gpx_logindex_compact(gpx_engine* h, gpx_logindex_counts* counts);

#ifdef __cplusplus
}
#endif
#endif /* GPX_LOGINDEX_H */
