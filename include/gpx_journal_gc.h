/*
 * gpx_journal_gc.h — journal compaction: drop the logged ACCEPTs that garbage collection no longer needs, on the device.
 *
 * gpx_journal_pack (gpx_journal.h) writes the journal; this call shrinks it.  The reference's half of that is
 * SQLPaxosLogger.garbageCollectJournal -> compactLogfiles -> compactLogfile (SQLPaxosLogger.java:3154-3170, 3282-3343,
 * 3347-3440) and mergeLogfiles (:3476 ff.): a loop that reads every entry of a file, parses it back into a packet, looks
 * up its group's LogIndex and asks LogIndex.isLogMsgNeeded (paxosutil/LogIndex.java:331-345) whether the entry is still
 * needed, against the threshold setGCSlot stored (SQLPaxosLogger.java:1480-1482).  Here the caller holds the index rows
 * gpx_journal_pack handed out, the acceptor's acceptedGCSlot of every group lives in device memory, and one call decides
 * all rows, writes the surviving entries contiguously with their new index rows, and - without touching a file byte -
 * tells the caller which of compactLogfile's three outcomes applies.
 *
 * Rows.  Row i < n is one LogIndex entry of an ACCEPT: e_gidx, e_slot, e_bnum, e_bcoord, e_off, e_len as
 *   gpx_journal_pack wrote them.  Its entry is in[e_off[i] - in_base .. + 4 + e_len[i]): the length prefix and the
 *   bytes.  `in` may hold one file (in_base = the file offset of its first byte) or several laid end to end, which is
 *   mergeLogfiles; the output is one file either way.  Bytes of `in` that no row names are not copied.
 * Usable.  A row is refused when e_off[i] - in_base is negative, when e_len[i] is outside [0, INT32_MAX - 4], when the
 *   range [e_off[i] - in_base, + 4 + e_len[i]) does not lie inside [0, in_bytes), or - with in != NULL - when the
 *   big-endian length prefix at the offset differs from e_len[i] (getJournaledMessage's own test, SQLPaxosLogger.java:
 *   3077-3096).  A refused row is GPX_JG_BAD, counts in n_bad and contributes no entry.  Every index and range is
 *   tested before any byte is read, and the prefix before any byte of the body.  A CALLER MUST NOT REPLACE A FILE WHEN
 *   n_bad > 0: the rows and the bytes disagree, and what the output lacks may be an entry that is still needed.
 * Threshold.  With acc = the acceptor's acceptedGCSlot of group g = e_gidx[i] as it is now,
 *     gc = cp_slot ? ((int32)(cp_slot[i] - acc) < 0 ? cp_slot[i] : acc) : acc
 *   which is setGCSlot, SQLPaxosLogger.java:1481-1482 (gcSlot = min(checkpointed slot, acceptedGCSlot)) in wrapping
 *   arithmetic.  cp_slot is per row: the caller's last checkpointed slot of that row's group.  NULL means the acceptor's
 *   GC slot alone; that is right when the caller checkpoints every group at least as far as it lets the acceptor's GC
 *   slot move - an application whose checkpoint precedes the ACCEPT that carries the new median checkpointed slot, the
 *   order of PaxosInstanceStateMachine's handlers - or keeps no checkpoints of its own.
 *   One deviation: the reference freezes acceptedGCSlot at the last checkpoint (deleteOutdatedMessages hands it to
 *   setGCSlot then, :1473-1482); this call reads the current one, which is never smaller.  So an entry may go one checkpoint earlier than
 *   in the Java; it goes only when it is both at or below the caller's own checkpoint (cp_slot) and at or below what a
 *   majority has executed (the median checkpointed slot the acceptor's GC slot follows).
 * Needed.  A row is kept iff (int32)(e_slot[i] - gc) > 0 (LogIndex.java:333: the slot alone decides for an ACCEPT, as in
 *   the reference).  A row whose e_gidx is outside [0, max_groups), or whose group does not exist, is kept: it is
 *   GPX_JG_KEEP_UNJUDGED and counts in n_unjudged - what cannot be judged is never dropped.  A stopped group is judged
 *   like any other.
 * Output.  Kept entries leave in row order, byte for byte as they stand in `in`, prefix included, contiguous: pos(0) = 0,
 *   pos(e + 1) = pos(e) + 4 + len(e).  k_off[e] = out_base + pos(e), k_len[e] = the entry's length, k_src[e] = its row,
 *   k_gidx / k_slot / k_bnum / k_bcoord copies of the row's fields.  Each k_* column except k_off and k_len may be
 *   NULL; e_bnum and e_bcoord may be NULL when their outputs are.
 * Verdicts.  verdict[i] is row i's GPX_JG_* verdict, dense, written under GPX_JG_COUNT_ONLY too; it may be NULL.
 * Capacity.  As gpx_journal_pack: kept entry e is done iff e < cap_entries and pos(e) + 4 + len(e) <= cap_bytes; the done
 *   entries are a prefix.  Nothing at or beyond out + bytes_done is written, nothing beyond row n_done of any k_*
 *   column.  n_keep and keep_bytes always describe the whole call; a cut call is continued with the columns advanced
 *   past k_src[n_done - 1] and out_base moved on by bytes_done.  `out` must be 16-byte aligned.
 * unchanged = 1 iff n_bad == 0, every row is kept, row 0 starts at in_base, every row starts where its predecessor ends
 *   and keep_bytes == in_bytes: the output would be the input.
 * The three outcomes of compactLogfile, in this order:
 *   n_keep == 0   delete the file (SQLPaxosLogger.java:3427-3431)
 *   unchanged     leave it (:3432-3436); with GPX_JG_SKIP_UNCHANGED nothing was written
 *   otherwise     write out[0, bytes_done) to a new file, rename it over the old one, and update the index from k_src /
 *                 k_off (:3420-3426, modifyLogIndexEntry :3443-3458) - unless n_bad > 0, see above.
 * Reads of `in`.  `in` must be 16-byte aligned when non-NULL.  Only aligned words (4 or 16 bytes) that hold at least one
 *   byte of an entry whose range checked out are read, and nothing at or beyond in + round_up(in_bytes, 16): the caller's
 *   block ends at a 16-byte boundary at or behind in_bytes.
 * Ordering.  The call reads group state and writes none.  It is queued on the engine's back-end stream, behind every
 *   call made on the engine before it, as the sweep and checkpoint _dev calls are.
 * Out of scope.  The PREPARE branch of isLogMsgNeeded (LogIndex.java:336-343): PREPARE has no byte form, ACCEPT is the
 *   only log message with one (gpx_journal.h).  File age (LOGFILE_AGE_THRESHOLD), FileIDMap.isRemovable,
 *   LAZY_COMPACTION, the rename, modifyLogIndexEntry itself and the LogIndex map keyed by name: the host does these from
 *   what the call returns.  gpx::FileLogger (gigapaxos_amd/host/) keeps its own loop.
 * Forms.  _dev: every pointer is device memory (counts too), the call is queued and returns; scratch (per-tile words and
 *   16 bytes per row) is allocated by the first call.  gpx_journal_gc: host pointers, synchronous, in two passes.  Pass 1
 *   sends the rows alone and gets counts and verdicts back; the length prefixes of the rows whose range checked out are
 *   compared on the host, so n_bad, n_usable and the verdicts equal the _dev form's.  If nothing is kept, if
 *   GPX_JG_COUNT_ONLY is set or GPX_JG_SKIP_UNCHANGED applies, the call ends there: no file byte crosses the link.  Pass
 *   2 goes over the rows in chunks whose kept entries lie inside a window of at most 64 MiB of `in` (or are one row), and
 *   only that window is copied in.  n_runs_done of this form counts a run once per chunk it is part of.
 * Errors.  All argument checks come before any device work:
 *   GPX_EINVAL     null handle or counts; negative n, in_bytes, cap_bytes or cap_entries; unknown flag bits; an `in` or
 *                  `out` that is not 16-byte aligned; with n > 0 a null e_gidx, e_slot, e_off or e_len, a null e_bnum
 *                  (e_bcoord) with a non-null k_bnum (k_bcoord); without GPX_JG_COUNT_ONLY and n > 0 a null `in`, out,
 *                  k_off or k_len
 *   GPX_ECAPACITY  n above max_batch
 *   GPX_ENOMEM     the scratch could not be allocated (the engine stays usable)
 */
#ifndef GPX_JOURNAL_GC_H
#define GPX_JOURNAL_GC_H

#include "gpx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpx_journal_gc_counts { /* 64 bytes, always written whole; device memory for the _dev call */
  int32_t n_usable;                    /* rows whose range (and, with `in`, length prefix) checks out */
  int32_t n_keep;                      /* usable rows that are still needed (unjudged ones included) */
  int32_t n_done;                      /* kept entries written: a prefix of them */
  int32_t n_bad;                       /* rows refused: no entry */
  int32_t n_unjudged;                  /* usable rows kept because their group could not be judged */
  int32_t n_runs_done;                 /* source runs the copy moved (diagnostic) */
  int32_t unchanged;                   /* 1: the kept entries are the whole input, in place */
  int32_t reserved;                    /* 0 */
  int64_t keep_bytes;                  /* bytes all n_keep entries need */
  int64_t bytes_done;                  /* bytes written */
  int64_t named_bytes;                 /* sum of 4 + len over the usable rows: compare with the file size */
  int64_t reserved2;                   /* 0 */
} gpx_journal_gc_counts;

#define GPX_JG_COUNT_ONLY 1     /* verdicts and counts only; `in`, out and the k_* columns may be NULL */
#define GPX_JG_SKIP_UNCHANGED 2 /* when counts.unchanged comes out 1, write nothing (n_done = 0, bytes_done = 0) */

#define GPX_JG_DROP 0
#define GPX_JG_KEEP 1
#define GPX_JG_KEEP_UNJUDGED 2
#define GPX_JG_BAD 3

int gpx_journal_gc_dev(gpx_engine* h, int32_t n, const uint8_t* in, int64_t in_bytes, int64_t in_base,
                       const int32_t* e_gidx, const int32_t* e_slot, const int64_t* e_off, const int32_t* e_len,
                       const int32_t* e_bnum, const int32_t* e_bcoord, const int32_t* cp_slot, int64_t out_base,
                       int32_t flags, uint8_t* out, int64_t cap_bytes, int32_t cap_entries, uint8_t* verdict,
                       int32_t* k_src, int32_t* k_gidx, int32_t* k_slot, int32_t* k_bnum, int32_t* k_bcoord,
                       int64_t* k_off, int32_t* k_len, gpx_journal_gc_counts* counts);
int gpx_journal_gc(gpx_engine* h, int32_t n, const uint8_t* in, int64_t in_bytes, int64_t in_base,
                   const int32_t* e_gidx, const int32_t* e_slot, const int64_t* e_off, const int32_t* e_len,
                   const int32_t* e_bnum, const int32_t* e_bcoord, const int32_t* cp_slot, int64_t out_base,
                   int32_t flags, uint8_t* out, int64_t cap_bytes, int32_t cap_entries, uint8_t* verdict, int32_t* k_src,
                   int32_t* k_gidx, int32_t* k_slot, int32_t* k_bnum, int32_t* k_bcoord, int64_t* k_off, int32_t* k_len,
                   gpx_journal_gc_counts* counts);

#ifdef __cplusplus
}
#endif
#endif /* GPX_JOURNAL_GC_H */
