/*
 * gpx_packed_out.h — proposals and decisions as packed records in ONE caller buffer.
 *
 * The asynchronous calls of include/gpx.h hand their outputs back as plain columns: 17 bytes per proposal (four int32
 * columns and a status byte), 21 per decision (five int32 columns and a kind byte).  Through host pointers the step
 * is bound by the link, and in the steady state those columns repeat even more than the votes of
 * include/gpx_packed.h do: one ballot for the whole call, slots and checkpoints within a byte of one entry.  A PACKED
 * OUTPUT is one buffer that starts with a 32-byte header and holds the call's outputs in one of two forms: RECORDS
 * (4 bytes per proposal, 8 per decision, plus a 32-byte row for every entry that does not fit) or COLUMNS (the plain
 * columns, when more than one entry in four would need a row).  The plain columns remain the default form of every
 * call; nothing here changes them.
 *
 * THE UNPACKED BUFFER IS, BY DEFINITION, THE PLAIN OUTPUT COLUMNS OF include/gpx.h IN OUTPUT ORDER: everything gpx.h
 * says about those columns (order, n_out, ordering contract) holds for it.
 *
 * With R(x) = x rounded up to a multiple of 32 (every area below starts on a 32-byte boundary of the buffer; the
 * bytes between the end of an area's data and that boundary are ZERO):
 *
 * RECORDS, decisions (kind GPX_PO_DECISIONS)
 *   byte 32:           rec[n][2] uint32 = (gidx, w)
 *   byte 32 + R(8 n):  rows[n_exc][8] int32
 *   w bit 31 clear: bits 0-7 dslot, 8-15 dcp, 16-17 d_kind, bits 18-30 zero (reserved).  The entry is
 *       (gidx, base_slot + dslot, bnum, bcoord, base_cp + dcp, d_kind)
 *     with the ballot and the bases from the header; the sums are taken in uint32 and read back as int32 (Java's
 *     wraparound, DESIGN.md 2: outputs that straddle Integer.MAX_VALUE pack without rows).
 *   w bit 31 set: bits 0-30 are a row index r < n_exc; row r = bnum, bcoord, slot, median_cp, kind, 0, 0, 0 and the
 *     entry is (gidx, slot, bnum, bcoord, median_cp, kind).
 * RECORDS, proposals (kind GPX_PO_PROPOSALS): dense, entry i belongs to record i of the call
 *   byte 32:           rec[n] uint32 = w
 *   byte 32 + R(4 n):  rows[n_exc][8] int32
 *   w bit 31 clear: bits 0-7 dslot, 8-15 dcp, 16-23 status, bits 24-30 zero (reserved).  The entry is
 *       (base_slot + dslot, bnum, bcoord, base_cp + dcp, status).
 *   w bit 31 set: bits 0-30 are a row index r < n_exc; row r = slot, bnum, bcoord, median_cp, status, 0, 0, 0.
 * COLUMNS: the plain columns, each S = R(4 n) bytes after the one before it, the first at byte 32
 *   decisions: d_gidx, d_slot, d_bnum, d_bcoord, d_median_cp, then the d_kind bytes at 32 + 5 S
 *   proposals: slot, bnum, bcoord, median_cp, then the status bytes at 32 + 4 S
 *   (the byte column takes R(n) bytes; n_exc is 0 and the header's ballot and bases are those of the rule below)
 *
 * THE PACKING RULE is deterministic: a host model predicts every byte of a packed buffer.
 *   - among the first min(n, 64) entries, take the ballot (bnum, bcoord) that occurs most often; on a tie the one
 *     whose first occurrence is earliest.  The REFERENCE ENTRY is that ballot's first occurrence.
 *   - the header's ballot is that ballot; base_slot = the reference's slot - 128, base_cp = its median_cp - 128, in
 *     uint32 arithmetic: the byte covers -128 .. +127 around the reference.
 *   - entry i needs a row iff its ballot differs from the header's, or (uint32)(slot - base_slot) or
 *     (uint32)(median_cp - base_cp) exceeds 255.  Rows are numbered in entry order and never shared.
 *   - needed <= n / 4: the form is RECORDS with n_exc = needed.  Otherwise COLUMNS.
 *   - n == 0: RECORDS, every header field zero except kind.
 * d_kind is GPX_D_DECISION or GPX_D_PREEMPTED (include/gpx.h): two bits.  The host packer refuses a kind above 3.
 */
#ifndef GPX_PACKED_OUT_H
#define GPX_PACKED_OUT_H

#include "gpx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpx_packed_out_hdr { /* 32 bytes at byte 0 of the buffer, native (little-endian) order */
  int32_t form;                     /* GPX_PO_RECORDS | GPX_PO_COLUMNS */
  int32_t kind;                     /* GPX_PO_DECISIONS | GPX_PO_PROPOSALS */
  int32_t n;                        /* entries: *n_out for decisions, the call's n for proposals */
  int32_t n_exc;                    /* rows; 0 in the columns form */
  int32_t bnum, bcoord, base_slot, base_cp;
} gpx_packed_out_hdr;

#define GPX_PO_RECORDS 1
#define GPX_PO_COLUMNS 2
#define GPX_PO_DECISIONS 1
#define GPX_PO_PROPOSALS 2
#define GPX_PO_EXC_BIT 0x80000000u      /* w: the record names a row */
#define GPX_PO_DEC_RESERVED 0x7FFC0000u /* w of a decision's delta record: must be zero */
#define GPX_PO_PROP_RESERVED 0x7F000000u /* w of a proposal's delta record: must be zero */
#define GPX_PO_EXC_DIV 4 /* RECORDS carries at most n / 4 rows: 8 + 32 / 4 = 16 bytes per decision at the most */
#define GPX_PO_REF_WINDOW 64 /* the entries the reference ballot is chosen among */

#define GPX_PO_R(x) (((size_t)(x) + 31) & ~(size_t)31)
/* bytes a buffer for up to `cap` entries must have: enough for both kinds and both forms (RECORDS never exceeds
 * 16 bytes per entry + 64, so a packed buffer is never larger than the columns it replaces) */
#define GPX_PACKED_OUT_BYTES(cap) (32 + 5 * GPX_PO_R(4 * (size_t)(cap)) + GPX_PO_R(cap))

/* ---- host helpers: no device call, no engine ----------------------------------------------------------- */
/* The bytes the buffer actually uses, from its header: nothing at or beyond that offset is written by any packer.
 * GPX_EINVAL for a header that is not one (null, unknown form or kind, negative counts, rows in the columns form). */
int64_t gpx_packed_out_size(const void* buf);

/* columns -> buffer by the rule above.  Return the rows NEEDED (>= 0; above n / 4 the buffer holds the columns
 * form), GPX_EINVAL (null pointers with n > 0, n < 0, a d_kind above 3), or GPX_ECAPACITY when
 * out_bytes < GPX_PACKED_OUT_BYTES(n).  `out` may sit at any 4-byte alignment. */
int gpx_decisions_pack(int32_t n, const int32_t* d_gidx, const int32_t* d_slot, const int32_t* d_bnum,
                       const int32_t* d_bcoord, const int32_t* d_median_cp, const uint8_t* d_kind, void* out,
                       size_t out_bytes);
int gpx_proposals_pack(int32_t n, const int32_t* slot, const int32_t* bnum, const int32_t* bcoord,
                       const int32_t* median_cp, const uint8_t* status, void* out, size_t out_bytes);
/* buffer (either form) + its byte length -> the plain columns, each with room for `cap` entries, and the count.
 * GPX_EINVAL when the buffer is not self-consistent - unknown form, a kind other than the call's, reserved bits
 * set, a row index >= n_exc, a size beyond `bytes` - and GPX_ECAPACITY when it holds more than `cap` entries; the
 * buffer is checked whole before the first entry is written: partial garbage is never returned. */
int gpx_decisions_unpack(const void* buf, size_t bytes, int32_t cap, int32_t* d_gidx, int32_t* d_slot,
                         int32_t* d_bnum, int32_t* d_bcoord, int32_t* d_median_cp, uint8_t* d_kind, int32_t* n_out);
int gpx_proposals_unpack(const void* buf, size_t bytes, int32_t cap, int32_t* slot, int32_t* bnum, int32_t* bcoord,
                         int32_t* median_cp, uint8_t* status, int32_t* n_out);

/* ---- engine calls ------------------------------------------------------------------------------------------ */
/*
 * gpx_decisions_pack_dev / gpx_proposals_pack_dev: the pack kernels alone, on the engine's stream.  Every pointer is
 * a DEVICE pointer and 16-byte aligned (else GPX_EINVAL); out_dev holds GPX_PACKED_OUT_BYTES(cap) bytes (cap = n for
 * proposals).  For decisions the entry count is *n_out_dev, read ON THE DEVICE (what gpx_accept_reply_batch_dev left
 * there; a value outside 0 .. cap is clamped); the columns hold cap entries.  cap / n above max_batch: GPX_ECAPACITY.
 * The buffer is byte for byte what the host packer makes of the same columns.
 */
int gpx_decisions_pack_dev(gpx_engine* h, const int32_t* n_out_dev, int32_t cap, const int32_t* d_gidx,
                           const int32_t* d_slot, const int32_t* d_bnum, const int32_t* d_bcoord,
                           const int32_t* d_median_cp, const uint8_t* d_kind, void* out_dev);
int gpx_proposals_pack_dev(gpx_engine* h, int32_t n, const int32_t* slot, const int32_t* bnum, const int32_t* bcoord,
                           const int32_t* median_cp, const uint8_t* status, void* out_dev);

/*
 * gpx_propose_packed_out_async: the twin of gpx_propose_batch_async; the five output columns come back as one packed
 * buffer (kind GPX_PO_PROPOSALS) in `out`.
 * gpx_accept_reply_packed_io_async: packed votes in (include/gpx_packed.h; pv as for gpx_accept_reply_packed_async),
 * packed decisions out (kind GPX_PO_DECISIONS; the header's n is the call's n_out).  `status` (per vote) may be NULL
 * and is otherwise the plain byte column.
 * `out` is HOST memory of out_bytes bytes, valid and untouched until gpx_engine_wait(ticket) returns; exactly
 * gpx_packed_out_size(out) bytes of it are written.  Inside a block the engine knows to be pinned (gpx_host_register,
 * gpx_host_alloc) and 16-byte aligned, the device writes it through the mapping with the length read on the device;
 * any other memory is filled by gpx_engine_wait (header first, then the rest).
 *   GPX_EINVAL     null handle / out / ticket, what the plain twin refuses
 *   GPX_ECAPACITY  out_bytes < GPX_PACKED_OUT_BYTES(n), before anything is queued; what the plain twin refuses
 * Tickets, depth, GPX_EBUSY and failures are those of the plain asynchronous calls.
 */
struct gpx_packed_votes;
int gpx_propose_packed_out_async(gpx_engine* h, int32_t n, const int32_t* gidx, const uint8_t* is_stop, void* out,
                                 size_t out_bytes, gpx_ticket* ticket);
int gpx_accept_reply_packed_io_async(gpx_engine* h, const struct gpx_packed_votes* pv, void* out, size_t out_bytes,
                                     uint8_t* status, gpx_ticket* ticket);

#ifdef __cplusplus
}
#endif
#endif /* GPX_PACKED_OUT_H */
