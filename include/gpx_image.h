/*
 * gpx_image.h — group images: bulk export and import of the FULL state of groups on the device.
 *
 * A gpx_hri row (gpx_group_retire / gpx_group_create / gpx_pause_sweep) describes a caught-up group only.  A group
 * image is the complete protocol state of one group - accepted and committed slots, outstanding proposals, a view
 * change in progress - as fixed-stride rows of little-endian 32-bit words, so that a busy group can leave its table
 * row and continue somewhere else: a bigger table, a second engine, another shard.  The rows are CANONICAL: any two
 * engines that hold the same logical state (the same gpx_group_dump) produce identical bytes.
 *
 * Row.  gpx_image_stride(kmax, window) bytes, a multiple of 64; padding is zero.
 *   MAIN row (kind GPX_IMAGE_MAIN), word offsets:
 *     0 format (GPX_IMAGE_FORMAT)   1 kind   2 flags (GPX_IMG_F_*, k in bits 8-15)   3 my_id
 *     4 kmax | window << 16         5 source gidx        6 version
 *     7 a_slot  8 a_bnum  9 a_bcoord  10 a_gc            11 c_bnum  12 c_bcoord  13 c_next  14 c_pcount
 *     15 reserved, 0
 *     16                  members[kmax]
 *     16 + kmax           node_slots[kmax]
 *     16 + 2 kmax         p_ring[window]      bits 0-15 responded mask, GPX_IMG_P_PRESENT, GPX_IMG_P_STOP
 *     16 + 2 kmax + W     acc_ring[window]    {slot, bnum, bcoord, flags}: flags bits 0-7 = this entry's GPX_IMG_R_*,
 *                                             bits 8-15 = the GPX_IMG_R_* of com_ring's entry at the same index
 *     16 + 2 kmax + 5 W   com_ring[window]    {slot, bnum, bcoord, median}
 *   (kmax and window share word 4 as two 16-bit halves: the header is 16 words, GPX_IMAGE_HEADER_WORDS.)
 *   CONTINUATION row (kind GPX_IMAGE_CONT): written only for a group that is running for coordinator
 *   (GPX_IMG_F_PREPARING); it immediately follows its main row, whose GPX_IMG_F_CONTINUED is set.
 *     0 format   1 kind   5 source gidx   6 c_wait   (every other header word 0)
 *     16          co_ring[window]     {slot, bnum, bcoord, GPX_IMG_CO_PRESENT | GPX_PV_*}
 *     16 + 4 W    co_handle[window]   {lo, hi}
 *     16 + 6 W    p_handle[window]    {lo, hi}
 *   It always fits the stride: 16 + 8 W <= 16 + 2 kmax + 9 W.  kmax 3, window 8: 384 bytes per group, 768 for a
 *   group that is running for coordinator.
 *   A ring entry sits at index slot & (window - 1), as in the engine.
 * Canonical.  Every word the group's state does not define is zero: a ring entry whose present bit is clear (and
 *   flag bits other than the ones named here), every coordinator word (c_*, node_slots, p_ring) of a group without a
 *   coordinator, members / node_slots at or beyond k, handles of entries that do not exist.  Nothing a kernel reads is
 *   lost by this (group images).  c_pcount is the number of present p_ring entries; the entry at index x
 *   is the proposal of the one slot s with s & (window - 1) == x and 1 <= c_next - s <= window, and while the group
 *   is running for coordinator the proposals are the slots c_next - c_pcount .. c_next - 1.
 *
 * Export.  Entry i < n is group gidx[i], or group i when gidx == NULL; n above max(max_groups, max_batch) is refused
 *   with GPX_ECAPACITY; listed entries must be pairwise distinct (not checked).  A dead or out-of-range entry writes
 *   nothing; a live one needs one or two rows.  Rows leave compacted in ascending entry index, a group's two rows
 *   adjacent.  `cap` counts rows: the groups written are the longest prefix of the live entries whose rows all fit, no
 *   group is written in part, nothing at or beyond the last written row is touched.  cap == 0 with a null o_rows only
 *   counts.  `counts` is always written whole.
 *   flags 0 copies and changes no state.  GPX_IMG_EVICT also retires exactly the groups written, as
 *   gpx_group_retire(GPX_RETIRE_KILL) does (a bound name answers GPX_W_NOGROUP from then on), and zeroes the
 *   deactivation sweep's idle words for them.
 * Import.  Row j goes to group gidx[j], or with gidx == NULL to the row's source gidx (restoring a snapshot into an
 *   engine of the same shape).  Only main rows use gidx[j]; the entry of a continuation row is ignored.  Destinations
 *   must be pairwise distinct (not checked).  n_rows above 2 * max(max_groups, max_batch): GPX_ECAPACITY.
 *   status[j] (required; a continuation row receives its main row's):
 *     GPX_S_OK
 *     GPX_S_IMAGE    the row is not an image this engine can take: wrong format; wrong kind where a main row is
 *                    expected; window, kmax or my_id different from the engine's; k outside 1..kmax; unknown or
 *                    inconsistent flag bits; a non-zero reserved word; GPX_IMG_F_CONTINUED without a following
 *                    continuation row of the same source gidx; a continuation row without a preceding continued
 *                    main row; a present ring entry whose slot does not belong at its index; a continuation row
 *                    while the engine's election arrays are not allocated; c_pcount outside 0..window, different
 *                    from the number of present p_ring entries, or - while the group is running for coordinator -
 *                    proposals that are not the slots c_next - c_pcount .. c_next - 1; any word that is not
 *                    canonical (above): a non-zero word under a clear present bit, an unknown bit in a ring's flag
 *                    word, a coordinator word of a group without a coordinator, members / node_slots at or beyond
 *                    k, a handle without its entry
 *     GPX_S_NOGROUP  destination out of range
 *     GPX_S_EXISTS   destination alive
 *   (in this order: what is wrong with the row itself comes first).  A refused group writes nothing at all.  The
 *   import uses no word of a row as an address or index but the destination, after its range check; the words that
 *   other calls later use as a bound or an index - k, the ring slots, c_pcount - are the ones checked above, so a
 *   row that is taken cannot make a later call write out of bounds.  Only canonical rows are taken, so an export
 *   of an imported group returns the bytes that were imported.  A successful import writes every state word of the
 *   group - the election words (c_wait, co_ring, co_handle, p_handle) from the continuation row, or zero if there
 *   is none and the election arrays are allocated - and the wire codec's copies of (exists, version), as
 *   gpx_group_create does; the sweep's idle words of the destination become 0.  Name bindings are the caller's
 *   business, as with gpx_group_create.
 *   GPX_IMG_VIEWCHANGE makes the call allocate the election arrays first, zeroed, exactly as the first
 *   gpx_election_begin does.  The caller knows to pass it from the export's counts: n_rows > n_live.
 * _dev forms.  Every pointer is a DEVICE pointer (counts and status too; gidx nullable); o_rows / rows 16-byte
 *   aligned, else GPX_EINVAL.  Asynchronous on the stream gpx_pause_sweep_dev uses: launches ordered by the stream
 *   alone, no workgroup waits for another one.
 * Host twins.  Every pointer is host memory; synchronous.  They run the _dev form through engine-owned device staging
 *   of at most 64 MiB; a larger request runs as consecutive chunks with a result identical to one call.
 * Errors.  All argument checks come before any device work and before the handle is used:
 *   GPX_EINVAL     null handle, negative n / cap / n_rows, unknown flag bits, null counts / status, cap > 0 with a
 *                  null buffer, n_rows > 0 with null rows, a misaligned _dev buffer
 *   GPX_ECAPACITY  n / n_rows above the limit
 *   GPX_ENOMEM     scratch or staging could not be allocated (the engine stays usable)
 */
#ifndef GPX_IMAGE_H
#define GPX_IMAGE_H

#include "gpx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPX_IMAGE_FORMAT 1
#define GPX_IMAGE_MAIN 1
#define GPX_IMAGE_CONT 2
#define GPX_IMAGE_HEADER_WORDS 16
#define GPX_IMAGE_TILE_ENTRIES 256 /* entries (export) or rows (import) one workgroup handles: where its edge cases lie */

/* header word 2 */
#define GPX_IMG_F_EXISTS 1
#define GPX_IMG_F_STOPPED 2
#define GPX_IMG_F_HASCOORD 4   /* the group has a coordinator here */
#define GPX_IMG_F_PREPARING 8  /* ... which is running for coordinator (not active) */
#define GPX_IMG_F_CONTINUED 16 /* a continuation row follows */
#define GPX_IMG_F_K_SHIFT 8    /* members of the group, bits 8-15 */
/* ring words */
#define GPX_IMG_P_PRESENT 0x10000 /* p_ring entry */
#define GPX_IMG_P_STOP 0x20000
#define GPX_IMG_R_PRESENT 1 /* acc_ring / com_ring flag byte */
#define GPX_IMG_R_STOP 2
#define GPX_IMG_R_HASVALUE 4 /* com_ring's byte only */
#define GPX_IMG_CO_PRESENT 0x100 /* co_ring flag word, beside GPX_PV_STOP / GPX_PV_NOOP */

#define GPX_IMG_EVICT 1      /* export: retire the groups written */
#define GPX_IMG_VIEWCHANGE 2 /* import: allocate the election arrays first */

#define GPX_S_IMAGE 10 /* import: the row is not an image this engine can take */

typedef struct gpx_image_counts { /* 16 bytes, always written whole */
  int32_t n_live;                 /* scanned entries that name a live group */
  int32_t n_rows;                 /* rows all live entries need; may exceed cap */
  int32_t n_done;                 /* groups written */
  int32_t n_rows_done;            /* rows written */
} gpx_image_counts;

/* bytes per row, a multiple of 64; -1 for kmax outside 1..GPX_KMAX_LIMIT or a window that is no power of two in
 * 4..64.  Pure host function: needs no engine and no device. */
int64_t gpx_image_stride(int32_t kmax, int32_t window);

int gpx_group_export_dev(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t flags, int32_t cap, void* o_rows,
                         gpx_image_counts* counts);
int gpx_group_export(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t flags, int32_t cap, void* o_rows,
                     gpx_image_counts* counts);

int gpx_group_import_dev(gpx_engine* h, int32_t n_rows, const void* rows, const int32_t* gidx, int32_t flags,
                         uint8_t* status);
int gpx_group_import(gpx_engine* h, int32_t n_rows, const void* rows, const int32_t* gidx, int32_t flags,
                     uint8_t* status);

#ifdef __cplusplus
}
#endif
#endif /* GPX_IMAGE_H */
