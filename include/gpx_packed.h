/*
 * gpx_packed.h — accept-reply votes as packed 8-byte records.
 *
 * The accept-reply call of include/gpx.h takes six int32 columns, 24 bytes per vote (16 in the common-ballot form
 * of gpx_accept_reply_batch_async).  Through host pointers that call is bound by the link, not by its kernels
 * (DESIGN.md 5), and in the steady state PISM.handleBatchedAcceptReply sees, nearly every one of those bytes repeats:
 * one ballot for the whole batch, slots and checkpoints a few units apart, a handful of acceptor ids (the reference's
 * own frame spends 12 bytes per slot on it, BatchedAcceptReply.java:113-147).  A PACKED batch is one 8-byte record per
 * vote - the group, and three byte deltas against values that go once per call - plus a 32-byte exception row for
 * every vote that does not fit.  The plain columns remain the default form; nothing here changes them.
 *
 * THE UNPACKED BATCH IS, BY DEFINITION, THE SIX COLUMNS IN RECORD ORDER: everything include/gpx.h says about a vote
 * batch (ordering contract, output order, n_out, output capacity of n entries per column) holds for a packed call as
 * it does for the plain call on those columns.
 *
 * Record i is two 32-bit words in native (little-endian) order: rec[2i] = gidx, rec[2i + 1] = w.
 *   w bit 31 clear: bits 0-7 dslot, 8-15 dcp, 16-23 dacc, bits 24-30 zero (reserved).  The vote is
 *       (gidx, bnum, bcoord, base_slot + dslot, base_acceptor + dacc, base_cp + dcp)
 *     with bnum, bcoord and the bases from the header.  Every sum is taken in uint32 and read back as int32 -
 *     Java's wraparound, as everywhere in this engine: a batch whose slots straddle Integer.MAX_VALUE
 *     packs without exceptions.
 *   w bit 31 set: bits 0-30 are an exception row index r < n_exc.  The vote is
 *       (gidx, exc[r][0] = bnum, exc[r][1] = bcoord, exc[r][2] = slot, exc[r][3] = acceptor, exc[r][4] = max_cp);
 *     exc[r][5..7] are zero.  Several records may name one row.
 *   A record with a reserved bit set, or with r >= n_exc, is MALFORMED: it unpacks to (gidx = -1, 0, 0, 0, 0, 0), and
 *     the engine drops that vote with GPX_S_NOGROUP exactly as it drops any group index out of range.  Its neighbours
 *     are unaffected.
 */
#ifndef GPX_PACKED_H
#define GPX_PACKED_H

#include "gpx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpx_packed_votes {
  int32_t n;            /* votes */
  int32_t n_exc;        /* exception rows */
  int32_t bnum, bcoord; /* the ballot of every vote that has no exception row */
  int32_t base_slot, base_cp, base_acceptor;
  int32_t reserved;     /* 0 */
  const uint32_t* rec;  /* [n][2]   8-byte records, native (little-endian) order */
  const int32_t* exc;   /* [n_exc][8] 32-byte rows: bnum, bcoord, slot, acceptor, max_cp, 0, 0, 0 */
} gpx_packed_votes;

#define GPX_PACKED_EXC_BIT 0x80000000u /* w: the record names an exception row */
#define GPX_PACKED_RESERVED 0x7F000000u /* w of a delta record: must be zero */
/* a call may carry at most n / GPX_PACKED_EXC_DIV exception rows: at one in four the packed form moves
 * 8 + 32 / 4 = 16 bytes per vote, as much as the common-ballot columns; beyond that it is the larger form */
#define GPX_PACKED_EXC_DIV 4

/* ---- host helpers: no device call, no engine ----------------------------------------------------------- */
/*
 * Packs six columns of n votes.  The rule is deterministic:
 *   - the header's ballot is the Boyer-Moore majority candidate of (bnum[i], bcoord[i]) over the call: start with
 *     no candidate and a count of 0; for every vote in order, a count of 0 makes the vote's ballot the candidate
 *     with count 1, an equal ballot adds 1, a different one takes 1 away.  (A ballot that more than half of the
 *     votes carry always ends as the candidate, wherever the odd ones sit: an odd FIRST vote does not turn every
 *     other vote into an exception.)
 *   - base_slot, base_cp, base_acceptor = slot, max_cp, acceptor of the FIRST vote that carries the candidate
 *     ballot, minus 128 in uint32 arithmetic: the byte covers -128 .. +127 around that vote.
 *   - vote i gets an exception row iff its ballot differs from the header's, or one of
 *     (uint32)(slot[i] - base_slot), (uint32)(max_cp[i] - base_cp), (uint32)(acceptor[i] - base_acceptor)
 *     is above 255.  Exception rows are numbered in record order and never shared.
 *   - n == 0: ballot and bases are 0.
 * rec_out takes n records (2 n words), exc_out up to exc_cap rows (8 exc_cap words; may be NULL when exc_cap == 0).
 * *out is filled in with rec = rec_out, exc = exc_out.
 * Returns the number of exception rows the batch NEEDS (>= 0), or GPX_EINVAL.  A return value above exc_cap means
 * the packing is incomplete: nothing was written past the capacity, out->n_exc == exc_cap, and the records of the
 * rows that did not fit name rows >= n_exc (malformed: they would be dropped) - pack again with room, or submit
 * the plain columns.  The value also tells, before submitting, whether the engine will take the batch
 * (GPX_PACKED_EXC_DIV).
 */
int gpx_votes_pack(int32_t n, const int32_t* gidx, const int32_t* bnum, const int32_t* bcoord, const int32_t* slot,
                   const int32_t* acceptor, const int32_t* max_cp, uint32_t* rec_out, int32_t* exc_out,
                   int32_t exc_cap, gpx_packed_votes* out);
/* The definition at the top of this file, on the host: pv->n entries into each column.  GPX_OK or GPX_EINVAL. */
int gpx_votes_unpack(const gpx_packed_votes* pv, int32_t* gidx, int32_t* bnum, int32_t* bcoord, int32_t* slot,
                     int32_t* acceptor, int32_t* max_cp);

/* ---- engine calls ------------------------------------------------------------------------------------------ */
/*
 * Common to the three calls: pv itself is a HOST struct, read before the call returns.
 *   GPX_EINVAL     null handle / pv, n < 0, n_exc < 0, rec == NULL with n > 0, exc == NULL with n_exc > 0
 *   GPX_ECAPACITY  n > max_batch, or n_exc > n / GPX_PACKED_EXC_DIV (use the plain call for such a batch)
 *
 * gpx_votes_unpack_dev: the unpack kernel alone, on the engine's stream.  pv->rec, pv->exc and the six columns are
 * DEVICE pointers, each 16-byte aligned (else GPX_EINVAL); the columns take pv->n entries.
 *
 * gpx_accept_reply_packed_dev: gpx_accept_reply_batch_dev on the unpacked batch.  pv->rec / pv->exc are device
 * pointers (16-byte aligned); the six columns live in scratch the engine owns (24 bytes x max_batch, allocated on
 * first use).  Outputs, n_out and status exactly as gpx_accept_reply_batch_dev leaves them.
 *
 * gpx_accept_reply_packed_async: the twin of gpx_accept_reply_batch_async.  pv->rec / pv->exc are HOST pointers (any
 * alignment; registered or gpx_host_alloc memory goes in as one DMA, pageable memory in pieces, like every other
 * input) and must stay valid and untouched until gpx_engine_wait(ticket) returns, like the output buffers.
 * 8 bytes per vote + 32 per exception row cross the link.  Tickets, depth, GPX_EBUSY and results are those of
 * gpx_accept_reply_batch_async on the unpacked columns.
 */
int gpx_votes_unpack_dev(gpx_engine* h, const gpx_packed_votes* pv, int32_t* gidx, int32_t* bnum, int32_t* bcoord,
                         int32_t* slot, int32_t* acceptor, int32_t* max_cp);
int gpx_accept_reply_packed_dev(gpx_engine* h, const gpx_packed_votes* pv, int32_t* d_gidx, int32_t* d_slot,
                                int32_t* d_bnum, int32_t* d_bcoord, int32_t* d_median_cp, uint8_t* d_kind,
                                int32_t* n_out, uint8_t* status);
int gpx_accept_reply_packed_async(gpx_engine* h, const gpx_packed_votes* pv, int32_t* d_gidx, int32_t* d_slot,
                                  int32_t* d_bnum, int32_t* d_bcoord, int32_t* d_median_cp, uint8_t* d_kind,
                                  int32_t* n_out, uint8_t* status, gpx_ticket* ticket);

#ifdef __cplusplus
}
#endif
#endif /* GPX_PACKED_H */
