/*
 * gpx_journal.h — journal batches: the ACCEPTs an acceptor must log, packed with their index rows on the device.
 *
 * An acceptor may not answer an ACCEPT before the ACCEPT is in its log: the reply leaves only after the log batch
 * (AbstractPaxosLogger.java:691-715).  Which ACCEPTs those are is `toLog` (PaxosInstanceStateMachine.java:1146-1149),
 * GPX_R_TOLOG in r_flags of gpx_accept_batch[_dev].  The reference's journal is a loop over every record,
 * SQLPaxosLogger.journal() (SQLPaxosLogger.java:965-1079): one ByteBuffer.allocate(4 + len), one putInt and one
 * appendToLogFile per packet, then messageLog.add(msg, curLogfile, curLogfileSize, bytes.length) (:1022-1025,
 * :403-422); in this repository it is FileLogger::logBatch (gigapaxos_amd/host/gpx_host.cpp).  gpx_journal_pack is that
 * loop as one call over frames that are already in HBM: what comes back goes to the file with one write.
 * The reference's defaults take exactly this path: ENABLE_JOURNALING=true, PAUSABLE_INDEX_JOURNAL=true,
 * DB_INDEX_JOURNAL=false, JOURNAL_COMPRESSION=false, BYTEIFICATION=true (PaxosConfig.java:240, 654, 667, 944, 594),
 * and an ACCEPT is the only log message with a byte form (SQLPaxosLogger.java:1084-1096).
 *
 * Records.  Record i < n is ACCEPT i of ONE gpx_accept_batch call: gidx, slot, bnum, bcoord are that call's inputs
 *   (the ACCEPT's own ballot: what LogIndex.add stores, SQLPaxosLogger.java:411-418), r_flags and status its outputs.
 *   Its frame is f = rec_frame ? rec_frame[i] : i.
 * Frame bytes, two forms, so that both sources work without a conversion:
 *   frame_len == NULL   frame_off has n_frames + 1 entries, frame f is frames[frame_off[f] .. frame_off[f + 1]):
 *                       gpx_wire_decode's form.
 *   frame_len != NULL   frame f is frames[frame_off[f] .. frame_off[f] + frame_len[f]): what the pack calls produce
 *                       (gpx_wire_pack_accepts_dev: 4-byte aligned starts, pad bytes between frames).
 * Selection.  Record i must be logged iff status[i] == GPX_S_OK && (r_flags[i] & GPX_R_TOLOG).  GPX_S_OK with the
 *   flag clear is a NACK or a repeated ACCEPT: a reply without a log entry.  A selected record whose frame cannot be
 *   used contributes no entry and counts in n_bad: f outside [0, n_frames); a negative start or length; a length above
 *   INT32_MAX - 4; a range that does not lie inside [0, frames_bytes).  Every index and range is tested before any
 *   byte of a frame is read: garbage is refused, never followed.
 * Entry bytes.  Entries leave in record order, the order of journal()'s loop (:985) and of FileLogger::logBatch.
 *   Entry e is be32(len) followed by the len bytes of the frame as received; entries are contiguous, no padding:
 *   pos(0) = 0, pos(e + 1) = pos(e) + 4 + len(e).  out[0 .. bytes_done) is byte for byte what FileLogger::logBatch
 *   builds for the same frames.
 * Index rows, LogIndex.add(slot, bnum, bcoord, ACCEPT, file, offset, length):
 *   e_off[e] = base_offset + pos(e), base_offset = the caller's curLogfileSize; the offset points at the length prefix
 *   and e_len[e] = len excludes it (getJournaledMessage, SQLPaxosLogger.java:3077-3096: seek(offset), readInt() ==
 *   length, read length bytes).  e_rec[e] = i, e_gidx / e_slot / e_bnum / e_bcoord the record's own; each of these
 *   five columns may be NULL.
 * Capacity.  Entry e is done iff e < cap_entries and pos(e) + 4 + len(e) <= cap_bytes; the done entries are a prefix.
 *   Rows and bytes are written for done entries only: nothing at or beyond out + bytes_done (the last partial 16-byte
 *   chunk takes narrower stores), nothing beyond row n_done of any e_* column.  n_entries and n_bytes always describe
 *   the whole call; the caller continues a cut call with the columns advanced past e_rec[n_done - 1].
 * GPX_JR_COUNT_ONLY.  Only *counts is written (n_done = 0, bytes_done = 0); out and the e_* columns may be NULL.
 * What the bytes are.  An entry is the frame AS RECEIVED.  The Java logs AcceptPacket.toBytes() of the parsed object
 *   (AcceptPacket.java:95-135): the ByteBuffer constructors (AcceptPacket.java:86-90, RequestPacket.java:956) do not
 *   keep the received array in byteifiedSelf, so toBytes rebuilds the bytes from the fields (RequestPacket.toBytes,
 *   RequestPacket.java:819-941, then slot, ballot, recovery, medianCheckpointedSlot, 0, sender).  The two are equal
 *   when byteification is on with integer node ids (BYTEIFICATION && IntegerMap.allInt(): otherwise toBytes is the
 *   JSON string) and the Java has changed no field of the packet between parsing and logging: no setEntryReplica /
 *   debug info / response value added, no request latched into or taken out of its batch.  Strings are decoded and
 *   encoded with the same single-byte CHARSET and keep their bytes.  tests/wire_model.py reads both directions.
 * Out of scope: DECISION and PREPARE log messages (no byte form); compression; the file itself - write, fsync, the
 *   roll at MAX_LOG_FILE_SIZE (journal() rolls only after a whole batch, :1038: a batch never splits); the LogIndex map
 *   keyed by name; the hold on the replies until the write is durable.
 * Forms.  _dev: every pointer is device memory (counts too), the call is queued on the engine's back-end stream and
 *   returns; scratch (per-tile words and 20 bytes per record) is allocated by the first call.  gpx_journal_pack: host
 *   pointers, synchronous; frames and columns are copied in, the counts and the first n_done rows and bytes_done bytes
 *   come back; a call whose frame windows exceed 64 MiB goes through in chunks of records.
 * Errors.  All argument checks come before any device work:
 *   GPX_EINVAL     null handle or counts; negative n, n_frames, frames_bytes, cap_bytes or cap_entries; unknown flag
 *                  bits; with n > 0 a null frame_off, r_flags or status, null frames with frames_bytes > 0; without
 *                  GPX_JR_COUNT_ONLY and n > 0 a null gidx, slot, bnum, bcoord, out, e_off or e_len, or an `out` that
 *                  is not 16-byte aligned
 *   GPX_ECAPACITY  n above max_batch
 *   GPX_ENOMEM     the scratch could not be allocated (the engine stays usable)
 */
#ifndef GPX_JOURNAL_H
#define GPX_JOURNAL_H

#include "gpx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpx_journal_counts { /* 32 bytes, always written whole; device memory for the _dev call */
  int32_t n_entries;                /* records that must be logged and have a usable frame (may exceed n_done) */
  int32_t n_done;                   /* entries written: a prefix of them */
  int32_t n_bad;                    /* records marked to log whose frame is unusable: no entry */
  int32_t reserved;                 /* 0 */
  int64_t n_bytes;                  /* bytes all n_entries need */
  int64_t bytes_done;               /* bytes written = where entry n_done would start */
} gpx_journal_counts;

#define GPX_JR_COUNT_ONLY 1 /* counts only: nothing else is written, out and the e_* columns may be NULL */

int gpx_journal_pack_dev(gpx_engine* h, int32_t n, const uint8_t* frames, int64_t frames_bytes, int32_t n_frames,
                         const int64_t* frame_off, const int32_t* frame_len, const int32_t* rec_frame,
                         const int32_t* gidx, const int32_t* slot, const int32_t* bnum, const int32_t* bcoord,
                         const uint8_t* r_flags, const uint8_t* status, int64_t base_offset, int32_t flags, uint8_t* out,
                         int64_t cap_bytes, int32_t cap_entries, int32_t* e_rec, int32_t* e_gidx, int32_t* e_slot,
                         int32_t* e_bnum, int32_t* e_bcoord, int64_t* e_off, int32_t* e_len, gpx_journal_counts* counts);
int gpx_journal_pack(gpx_engine* h, int32_t n, const uint8_t* frames, int64_t frames_bytes, int32_t n_frames,
                     const int64_t* frame_off, const int32_t* frame_len, const int32_t* rec_frame, const int32_t* gidx,
                     const int32_t* slot, const int32_t* bnum, const int32_t* bcoord, const uint8_t* r_flags,
                     const uint8_t* status, int64_t base_offset, int32_t flags, uint8_t* out, int64_t cap_bytes,
                     int32_t cap_entries, int32_t* e_rec, int32_t* e_gidx, int32_t* e_slot, int32_t* e_bnum,
                     int32_t* e_bcoord, int64_t* e_off, int32_t* e_len, gpx_journal_counts* counts);

/* Host helper, no engine: walks <be32 len><len bytes>* as recovery does and stops at the first entry that is torn -
 * fewer than 4 bytes left, a negative length, or a body past the end.  *good_bytes = the position of the first byte
 * that is not part of a whole entry, *n_entries = all whole entries; rows (e_off[e] = base_offset + position of the
 * prefix, e_len[e] = len) are written for the first `cap` of them.  GPX_EINVAL: negative bytes or cap, null buf with
 * bytes > 0, null n_entries or good_bytes, cap > 0 with a null e_off or e_len. */
int gpx_journal_walk(const uint8_t* buf, int64_t bytes, int64_t base_offset, int32_t cap, int64_t* e_off,
                     int32_t* e_len, int32_t* n_entries, int64_t* good_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GPX_JOURNAL_H */
