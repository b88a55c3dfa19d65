/*
 * gpx_jni.c — the JNI shim between gigapaxos's Java host and the C-ABI of include/gpx.h /
 * include/gpx_wire.h / include/gpx_packed.h.
 *
 * Compiled only where a JDK exists (none in the build image or on the GPU box: `java -version` is
 * "command not found" on both), hence the guard:
 *
 *   gcc -shared -fPIC -DGPX_HAVE_JNI -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -Iinclude \
 *       gigapaxos_amd/jni/gpx_jni.c -Lgigapaxos_amd/csrc -lgpx_hip \
 *       -Wl,-rpath,'$ORIGIN/../csrc' -o gigapaxos_amd/jni/libgpx_jni.so
 *
 * Without GPX_HAVE_JNI the file compiles to an empty translation unit plus a self-check of the
 * argument counts against the header (tests/test_abi_symbols.py builds it that way), so the shim
 * cannot silently drift from include/gpx.h.
 *
 * Java side: edu.umass.cs.gigapaxos.gpx.GpxEngine.  Every column is a direct
 * ByteBuffer in native byte order, owned by the caller and valid only for the call - the contract
 * of include/gpx.h.  One submitting thread per engine at a time (ConsumerTask.java:163-174).
 * Reference seam each entry replaces: PaxosManager.handlePaxosPacket -> PaxosInstanceStateMachine.
 * handlePaxosMessage (PaxosManager.java:1126-1204, PaxosInstanceStateMachine.java:411-583).
 */
#include <stdint.h>

#include "../../include/gpx.h"
#include "../../include/gpx_wire.h"
#include "../../include/gpx_packed.h"
#include "../../include/gpx_scan.h"
#include "../../include/gpx_sweep.h"
#include "../../include/gpx_timers.h"
#include "../../include/gpx_journal.h"
#include "../../include/gpx_journal_gc.h"
#include "../../include/gpx_logindex.h"
#include "../../include/gpx_image.h"
#include "../../include/gpx_delta.h"
#include "../../include/gpx_checkpoint.h"
#include "../../include/gpx_viewchange.h"

#ifdef GPX_HAVE_JNI
#include <jni.h>

#define H(h) ((gpx_engine*)(intptr_t)(h))
#define B(b) ((b) ? (*env)->GetDirectBufferAddress(env, (b)) : 0)
#define JFN(ret, name) JNIEXPORT ret JNICALL Java_edu_umass_cs_gigapaxos_gpx_GpxEngine_##name

JFN(jlong, create)(JNIEnv* env, jclass c, jint myId, jint maxGroups, jint kmax, jint window, jint maxBatch,
                   jint device) {
  (void)env, (void)c;
  gpx_config cfg = {myId, maxGroups, kmax, window, maxBatch, device, GPX_F_ACCEPTS_FROM_DISK, 0};
  gpx_engine* h = 0;
  /* a handle (never negative as a jlong: a user-space pointer) or the negative GPX_E* code; the text is in
   * lastError() */
  const int rc = gpx_engine_create(&cfg, &h);
  return rc == GPX_OK ? (jlong)(intptr_t)h : (jlong)rc;
}
JFN(jint, destroy)(JNIEnv* env, jclass c, jlong h) {
  (void)env, (void)c;
  return gpx_engine_destroy(H(h));
}
JFN(jstring, lastError)(JNIEnv* env, jclass c) {
  (void)c;
  return (*env)->NewStringUTF(env, gpx_last_error());
}
/* pins a direct ByteBuffer for DMA once, after allocation (gpx_host_register) */
JFN(jint, hostRegister)(JNIEnv* env, jclass c, jlong h, jobject buf) {
  (void)c;
  if (!buf) return GPX_EINVAL;
  void* p = (*env)->GetDirectBufferAddress(env, buf); /* NULL for a heap (non-direct) buffer */
  const jlong cap = (*env)->GetDirectBufferCapacity(env, buf); /* -1 for one */
  if (!p || cap <= 0) return GPX_EINVAL;
  return gpx_host_register(H(h), p, (size_t)cap);
}
/* a direct ByteBuffer over memory allocated for the DMA engines (gpx_host_alloc = hipHostMalloc): the batch columns of
 * a host that wants the link's full rate without pinning JVM memory afterwards; hostFree(buffer) gives it back */
JFN(jobject, hostAlloc)(JNIEnv* env, jclass c, jlong h, jlong bytes) {
  (void)c;
  void* p = NULL;
  if (bytes <= 0 || gpx_host_alloc(H(h), (size_t)bytes, &p) != GPX_OK) return NULL;
  jobject buf = (*env)->NewDirectByteBuffer(env, p, bytes);
  if (!buf) (void)gpx_host_free(H(h), p); /* (no direct-buffer support, or out of memory: the block must not stay until destroy) */
  return buf;
}
JFN(jint, hostFree)(JNIEnv* env, jclass c, jlong h, jobject buf) {
  (void)c;
  if (!buf) return GPX_EINVAL;
  return gpx_host_free(H(h), (*env)->GetDirectBufferAddress(env, buf));
}
/* PaxosManager.createPaxosInstance(Map, ...) batch create (PaxosManager.java:664-691) */
JFN(jint, groupCreate)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject members, jobject k,
                       jobject hriRows, jobject status) {
  (void)c;
  return gpx_group_create(H(h), n, B(gidx), B(members), B(k), B(hriRows), B(status));
}
/* PISM.tryPause / PaxosManager.kill (PISM:2004-2035, PaxosManager.java:2162) */
JFN(jint, groupRetire)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jint mode, jobject hriRows,
                       jobject status) {
  (void)c;
  return gpx_group_retire(H(h), n, B(gidx), mode, B(hriRows), B(status));
}
/* RequestBatcher.process -> PM.proposeBatched -> PCS.propose (RequestBatcher.java:79-81, PCS:233-263) */
JFN(jint, proposeBatch)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject isStop, jobject slot,
                        jobject bnum, jobject bcoord, jobject medianCp, jobject status) {
  (void)c;
  return gpx_propose_batch(H(h), n, B(gidx), B(isStop), B(slot), B(bnum), B(bcoord), B(medianCp), B(status));
}
/* PISM.handleAccept (PISM:1080-1166) */
JFN(jint, acceptBatch)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject bnum, jobject bcoord,
                       jobject slot, jobject medianCp, jobject aFlags, jobject rBnum, jobject rBcoord,
                       jobject rMaxCp, jobject rFlags, jobject status, jobject xGidx, jobject xFirst,
                       jobject xCount, jobject nRuns) {
  (void)c;
  return gpx_accept_batch(H(h), n, B(gidx), B(bnum), B(bcoord), B(slot), B(medianCp), B(aFlags), B(rBnum),
                          B(rBcoord), B(rMaxCp), B(rFlags), B(status), B(xGidx), B(xFirst), B(xCount),
                          B(nRuns));
}
/* PISM.handleBatchedAcceptReply / handleAcceptReply (PISM:1248-1419): one call per
 * PaxosPacketBatcher dequeue */
JFN(jint, acceptReplyBatch)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject bnum,
                            jobject bcoord, jobject slot, jobject acceptor, jobject maxCp, jobject dGidx,
                            jobject dSlot, jobject dBnum, jobject dBcoord, jobject dMedian, jobject dKind,
                            jobject nOut, jobject status) {
  (void)c;
  return gpx_accept_reply_batch(H(h), n, B(gidx), B(bnum), B(bcoord), B(slot), B(acceptor), B(maxCp),
                                B(dGidx), B(dSlot), B(dBnum), B(dBcoord), B(dMedian), B(dKind), B(nOut),
                                B(status));
}
/* The asynchronous twins (include/gpx.h): the call returns once its copies and kernels are queued; every
 * buffer stays untouched until engineWait(ticket) returns.  A ticket comes back through a one-element direct
 * LongBuffer. */
JFN(jint, proposeBatchAsync)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject isStop, jobject slot,
                             jobject bnum, jobject bcoord, jobject medianCp, jobject status, jobject ticket) {
  (void)c;
  return gpx_propose_batch_async(H(h), n, B(gidx), B(isStop), B(slot), B(bnum), B(bcoord), B(medianCp), B(status),
                                 (gpx_ticket*)B(ticket));
}
/* bnum == null && bcoord == null: every vote carries (commonBnum, commonBcoord) */
JFN(jint, acceptReplyBatchAsync)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject bnum,
                                 jobject bcoord, jint commonBnum, jint commonBcoord, jobject slot,
                                 jobject acceptor, jobject maxCp, jobject dGidx, jobject dSlot, jobject dBnum,
                                 jobject dBcoord, jobject dMedian, jobject dKind, jobject nOut, jobject status,
                                 jobject ticket) {
  (void)c;
  return gpx_accept_reply_batch_async(H(h), n, B(gidx), B(bnum), B(bcoord), commonBnum, commonBcoord, B(slot),
                                      B(acceptor), B(maxCp), B(dGidx), B(dSlot), B(dBnum), B(dBcoord), B(dMedian),
                                      B(dKind), B(nOut), B(status), (gpx_ticket*)B(ticket));
}
/* The votes as packed 8-byte records (include/gpx_packed.h): `records` holds n (gidx, w) pairs and `exceptions` nExc
 * rows of eight ints, both written in ByteOrder.nativeOrder() while the host drains its NIO buffers; `exceptions` may be
 * null when nExc == 0.  Both stay untouched until engineWait(ticket), like the outputs. */
JFN(jint, acceptReplyPackedAsync)(JNIEnv* env, jclass c, jlong h, jint n, jint nExc, jint bnum, jint bcoord,
                                  jint baseSlot, jint baseCp, jint baseAcceptor, jobject records, jobject exceptions,
                                  jobject dGidx, jobject dSlot, jobject dBnum, jobject dBcoord, jobject dMedian,
                                  jobject dKind, jobject nOut, jobject status, jobject ticket) {
  (void)c;
  const gpx_packed_votes pv = {n, nExc, bnum, bcoord, baseSlot, baseCp, baseAcceptor, 0,
                               (const uint32_t*)B(records), (const int32_t*)B(exceptions)};
  return gpx_accept_reply_packed_async(H(h), &pv, B(dGidx), B(dSlot), B(dBnum), B(dBcoord), B(dMedian), B(dKind),
                                       B(nOut), B(status), (gpx_ticket*)B(ticket));
}
JFN(jint, acceptBatchAsync)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject bnum, jobject bcoord,
                            jobject slot, jobject medianCp, jobject aFlags, jobject rBnum, jobject rBcoord,
                            jobject rMaxCp, jobject rFlags, jobject status, jobject xGidx, jobject xFirst,
                            jobject xCount, jobject nRuns, jobject ticket) {
  (void)c;
  return gpx_accept_batch_async(H(h), n, B(gidx), B(bnum), B(bcoord), B(slot), B(medianCp), B(aFlags), B(rBnum),
                                B(rBcoord), B(rMaxCp), B(rFlags), B(status), B(xGidx), B(xFirst), B(xCount),
                                B(nRuns), (gpx_ticket*)B(ticket));
}
JFN(jint, commitBatchAsync)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject bnum, jobject bcoord,
                            jobject slot, jobject medianCp, jobject cKind, jobject status, jobject xGidx,
                            jobject xFirst, jobject xCount, jobject nRuns, jobject ticket) {
  (void)c;
  return gpx_commit_batch_async(H(h), n, B(gidx), B(bnum), B(bcoord), B(slot), B(medianCp), B(cKind), B(status),
                                B(xGidx), B(xFirst), B(xCount), B(nRuns), (gpx_ticket*)B(ticket));
}
JFN(jint, engineWait)(JNIEnv* env, jclass c, jlong h, jlong ticket) {
  (void)env, (void)c;
  return gpx_engine_wait(H(h), (gpx_ticket)ticket);
}
JFN(jint, setOrderedBatches)(JNIEnv* env, jclass c, jlong h, jint mask) {
  (void)env, (void)c;
  return gpx_engine_set_ordered_batches(H(h), mask);
}
/* PISM.handleBatchedCommit / handleCommittedRequest (PISM:1432-1528) */
JFN(jint, commitBatch)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject bnum, jobject bcoord,
                       jobject slot, jobject medianCp, jobject cKind, jobject status, jobject xGidx,
                       jobject xFirst, jobject xCount, jobject nRuns) {
  (void)c;
  return gpx_commit_batch(H(h), n, B(gidx), B(bnum), B(bcoord), B(slot), B(medianCp), B(cKind), B(status),
                          B(xGidx), B(xFirst), B(xCount), B(nRuns));
}
/* PISM.handlePrepare (PISM:900-1006) */
JFN(jint, prepareBatch)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject bnum, jobject bcoord,
                        jobject firstSlot, jobject rBnum, jobject rBcoord, jobject rGc, jobject rFlags,
                        jobject pMask, jobject pSlot, jobject pBnum, jobject pBcoord, jobject status) {
  (void)c;
  return gpx_prepare_batch(H(h), n, B(gidx), B(bnum), B(bcoord), B(firstSlot), B(rBnum), B(rBcoord), B(rGc),
                           B(rFlags), B(pMask), B(pSlot), B(pBnum), B(pBcoord), B(status));
}
/* PISM.checkRunForCoordinator's decision over all groups (PISM:2090-2176) */
JFN(jint, electionScan)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject down, jint nDown,
                        jobject longDead, jint nLongDead, jint force, jobject run, jobject pBnum,
                        jobject pFirst, jobject status) {
  (void)c;
  return gpx_election_scan(H(h), n, B(gidx), B(down), nDown, B(longDead), nLongDead, force, B(run),
                           B(pBnum), B(pFirst), B(status));
}
/* PISM.tryMakeCoordinator -> PaxosCoordinator.makeCoordinator (PISM:2178-2183) */
JFN(jint, electionBegin)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject bnum,
                         jobject eStatus) {
  (void)c;
  return gpx_election_begin(H(h), n, B(gidx), B(bnum), B(eStatus));
}
/* PISM.handlePrepareReply (PISM:1008-1068) */
JFN(jint, prepareReplyBatch)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject acceptor,
                             jobject rBnum, jobject rBcoord, jobject firstSlot, jobject pvOff,
                             jobject pvSlot, jobject pvBnum, jobject pvBcoord, jobject pvHandle,
                             jobject pvFlags, jobject vKind, jobject eCount, jobject eMedian,
                             jobject eSlot, jobject eKind, jobject eHandle, jobject eFlags,
                             jobject status) {
  (void)c;
  return gpx_prepare_reply_batch(H(h), n, B(gidx), B(acceptor), B(rBnum), B(rBcoord), B(firstSlot),
                                 B(pvOff), B(pvSlot), B(pvBnum), B(pvBcoord), B(pvHandle), B(pvFlags),
                                 B(vKind), B(eCount), B(eMedian), B(eSlot), B(eKind), B(eHandle),
                                 B(eFlags), B(status));
}
/* getMissingCommittedSlots / shouldSync (PaxosAcceptor.java:405-438, PISM:2341-2364) */
JFN(jint, gapScan)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jint threshold, jint syncMode,
                   jint sizeLimit, jobject firstSlot, jobject maxCommitted, jobject missing,
                   jobject shouldSync, jobject status) {
  (void)c;
  return gpx_gap_scan(H(h), n, B(gidx), threshold, syncMode, sizeLimit, B(firstSlot), B(maxCommitted),
                      B(missing), B(shouldSync), B(status));
}
/* the scans that return only their hits (include/gpx_scan.h): counts = a direct buffer of 16 bytes */
JFN(jint, electionScanHits)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject down, jint nDown,
                            jobject longDead, jint nLongDead, jint force, jint cap, jobject oGidx, jobject oRun,
                            jobject oBnum, jobject oFirst, jobject counts) {
  (void)c;
  return gpx_election_scan_hits(H(h), n, B(gidx), B(down), nDown, B(longDead), nLongDead, force, cap, B(oGidx),
                                B(oRun), B(oBnum), B(oFirst), (gpx_scan_counts*)B(counts));
}
JFN(jint, pokeScanHits)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jint cap, jobject oGidx, jobject oPoke,
                        jobject oSlot, jobject oBnum, jobject oBcoord, jobject oMedianCp, jobject oFlags,
                        jobject oHeard, jobject counts) {
  (void)c;
  return gpx_poke_scan_hits(H(h), n, B(gidx), cap, B(oGidx), B(oPoke), B(oSlot), B(oBnum), B(oBcoord), B(oMedianCp),
                            B(oFlags), B(oHeard), (gpx_scan_counts*)B(counts));
}
JFN(jint, gapScanHits)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jint threshold, jint syncMode,
                       jint sizeLimit, jint require, jint cap, jobject oGidx, jobject oFirst, jobject oMaxCommitted,
                       jobject oMissing, jobject oSync, jobject counts) {
  (void)c;
  return gpx_gap_scan_hits(H(h), n, B(gidx), threshold, syncMode, sizeLimit, require, cap, B(oGidx), B(oFirst),
                           B(oMaxCommitted), B(oMissing), B(oSync), (gpx_scan_counts*)B(counts));
}
/* the deactivation sweep (include/gpx_sweep.h): oRows = a direct buffer of cap rows of 100 bytes, counts = one of
 * 16 bytes */
JFN(jint, pauseSweep)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jint minAge, jint flags, jint cap,
                      jobject oGidx, jobject oAge, jobject oRows, jobject counts) {
  (void)c;
  return gpx_pause_sweep(H(h), n, B(gidx), minAge, flags, cap, B(oGidx), B(oAge), (gpx_hri*)B(oRows),
                         (gpx_sweep_counts*)B(counts));
}
/* the retransmission sweep (include/gpx_timers.h): cfg = a direct buffer of 260 bytes (the step count, then the two
 * tables of 32 thresholds), the ten output columns direct buffers of cap entries, counts = one of 16 bytes */
JFN(jint, retransmitSweep)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jint nowMs, jobject cfg, jint flags,
                           jint cap, jobject oGidx, jobject oPoke, jobject oSlot, jobject oBnum, jobject oBcoord,
                           jobject oMedianCp, jobject oFlags, jobject oHeard, jobject oCount, jobject oWaited,
                           jobject counts) {
  (void)c;
  return gpx_retransmit_sweep(H(h), n, B(gidx), nowMs, (const gpx_rtx_cfg*)B(cfg), flags, cap, B(oGidx), B(oPoke),
                              B(oSlot), B(oBnum), B(oBcoord), B(oMedianCp), B(oFlags), B(oHeard), B(oCount), B(oWaited),
                              (gpx_rtx_counts*)B(counts));
}
/* journal batches (include/gpx_journal.h): frames = a direct buffer of framesBytes bytes, the columns direct buffers of n
 * entries (frameLen and recFrame may be null), out = a direct buffer of capBytes bytes at a 16-byte boundary, the seven
 * row columns direct buffers of capEntries entries (the first five may be null), counts = one of 32 bytes.  The caller
 * writes out[0, bytesDone) to the log file with one write and keeps the call's replies until that write is durable */
JFN(jint, journalPack)(JNIEnv* env, jclass c, jlong h, jint n, jobject frames, jlong framesBytes, jint nFrames,
                       jobject frameOff, jobject frameLen, jobject recFrame, jobject gidx, jobject slot, jobject bnum,
                       jobject bcoord, jobject rFlags, jobject status, jlong baseOffset, jint flags, jobject out,
                       jlong capBytes, jint capEntries, jobject eRec, jobject eGidx, jobject eSlot, jobject eBnum,
                       jobject eBcoord, jobject eOff, jobject eLen, jobject counts) {
  (void)c;
  return gpx_journal_pack(H(h), n, B(frames), framesBytes, nFrames, B(frameOff), B(frameLen), B(recFrame), B(gidx),
                          B(slot), B(bnum), B(bcoord), B(rFlags), B(status), baseOffset, flags, B(out), capBytes,
                          capEntries, B(eRec), B(eGidx), B(eSlot), B(eBnum), B(eBcoord), B(eOff), B(eLen),
                          (gpx_journal_counts*)B(counts));
}
/* journal compaction (include/gpx_journal_gc.h): in = a direct buffer of inBytes bytes at a 16-byte boundary whose
 * capacity is a multiple of 16 (may be null with GPX_JG_COUNT_ONLY), the seven input columns direct buffers of n entries
 * (eBnum, eBcoord and cpSlot may be null), out = a direct buffer of capBytes bytes at a 16-byte boundary, verdict = one of
 * n bytes or null, the seven k columns direct buffers of capEntries entries (the first five may be null), counts = one
 * of 64 bytes.  nKeep == 0: delete the file; unchanged: leave it; else, and only with nBad == 0, write out[0, bytesDone)
 * and rename */
JFN(jint, journalGc)(JNIEnv* env, jclass c, jlong h, jint n, jobject in, jlong inBytes, jlong inBase, jobject eGidx,
                     jobject eSlot, jobject eOff, jobject eLen, jobject eBnum, jobject eBcoord, jobject cpSlot,
                     jlong outBase, jint flags, jobject out, jlong capBytes, jint capEntries, jobject verdict,
                     jobject kSrc, jobject kGidx, jobject kSlot, jobject kBnum, jobject kBcoord, jobject kOff,
                     jobject kLen, jobject counts) {
  (void)c;
  return gpx_journal_gc(H(h), n, B(in), inBytes, inBase, B(eGidx), B(eSlot), B(eOff), B(eLen), B(eBnum), B(eBcoord),
                        B(cpSlot), outBase, flags, B(out), capBytes, capEntries, B(verdict), B(kSrc), B(kGidx), B(kSlot),
                        B(kBnum), B(kBcoord), B(kOff), B(kLen), (gpx_journal_gc_counts*)B(counts));
}
/* the log index (include/gpx_logindex.h): every column a direct buffer, counts = one of 32 bytes, status = one byte per
 * record (may be null), nDev = one 32-bit count or null; files are ids the caller assigns in creation order */
JFN(jint, logindexOpen)(JNIEnv* env, jclass c, jlong h, jint capRows) {
  (void)env, (void)c;
  return gpx_logindex_open(H(h), capRows);
}
JFN(jint, logindexAdd)(JNIEnv* env, jclass c, jlong h, jint n, jobject nDev, jobject eGidx, jobject eSlot, jobject eBnum,
                       jobject eBcoord, jobject eOff, jobject eLen, jint file, jobject status, jobject counts) {
  (void)c;
  return gpx_logindex_add(H(h), n, B(nDev), B(eGidx), B(eSlot), B(eBnum), B(eBcoord), B(eOff), B(eLen), file, B(status),
                          (gpx_logindex_counts*)B(counts));
}
JFN(jint, logindexSetGc)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject gcSlot, jint flags, jobject status,
                         jobject counts) {
  (void)c;
  return gpx_logindex_set_gc(H(h), n, B(gidx), B(gcSlot), flags, B(status), (gpx_logindex_counts*)B(counts));
}
JFN(jint, logindexLookup)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject minSlot, jobject maxSlot,
                          jobject hasMax, jint cap, jobject oRec, jobject oRow, jobject oSlot, jobject oBnum,
                          jobject oBcoord, jobject oFile, jobject oOff, jobject oLen, jobject status, jobject counts) {
  (void)c;
  return gpx_logindex_lookup(H(h), n, B(gidx), B(minSlot), B(maxSlot), B(hasMax), cap, B(oRec), B(oRow), B(oSlot),
                             B(oBnum), B(oBcoord), B(oFile), B(oOff), B(oLen), B(status),
                             (gpx_logindex_counts*)B(counts));
}
JFN(jint, logindexFileRows)(JNIEnv* env, jclass c, jlong h, jint file, jint cap, jobject oRow, jobject eGidx,
                            jobject eSlot, jobject eBnum, jobject eBcoord, jobject eOff, jobject eLen, jobject eGc,
                            jobject counts) {
  (void)c;
  return gpx_logindex_file_rows(H(h), file, cap, B(oRow), B(eGidx), B(eSlot), B(eBnum), B(eBcoord), B(eOff), B(eLen),
                                B(eGc), (gpx_logindex_counts*)B(counts));
}
JFN(jint, logindexRelocate)(JNIEnv* env, jclass c, jlong h, jint n, jobject nDev, jint generation, jobject oRow,
                            jobject kSrc, jint newFile, jobject kOff, jobject kLen, jobject counts) {
  (void)c;
  return gpx_logindex_relocate(H(h), n, B(nDev), generation, B(oRow), B(kSrc), newFile, B(kOff), B(kLen),
                               (gpx_logindex_counts*)B(counts));
}
JFN(jint, logindexFiles)(JNIEnv* env, jclass c, jlong h, jint fileBase, jint nFiles, jobject oRows, jobject oGroups,
                         jobject oMinFile, jobject counts) {
  (void)c;
  return gpx_logindex_files(H(h), fileBase, nFiles, B(oRows), B(oGroups), B(oMinFile), (gpx_logindex_counts*)B(counts));
}
JFN(jint, logindexCompact)(JNIEnv* env, jclass c, jlong h, jobject counts) {
  (void)c;
  return gpx_logindex_compact(H(h), (gpx_logindex_counts*)B(counts));
}
/* group images (include/gpx_image.h): oRows / rows = a direct buffer of rows of gpx_image_stride bytes, counts = one
 * of 16 bytes, status = one byte per row */
JFN(jint, groupExport)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jint flags, jint cap, jobject oRows,
                       jobject counts) {
  (void)c;
  return gpx_group_export(H(h), n, B(gidx), flags, cap, B(oRows), (gpx_image_counts*)B(counts));
}
JFN(jint, groupImport)(JNIEnv* env, jclass c, jlong h, jint nRows, jobject rows, jobject gidx, jint flags,
                       jobject status) {
  (void)c;
  return gpx_group_import(H(h), nRows, B(rows), B(gidx), flags, B(status));
}
/* delta images (include/gpx_delta.h): rows as above, oGone / gone = direct buffers of 32-bit group numbers, counts =
 * one of 32 bytes, status / goneStatus = one byte per row / per gone entry */
JFN(jint, exportDelta)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jint flags, jint cap, jobject oRows,
                       jint capGone, jobject oGone, jobject counts) {
  (void)c;
  return gpx_group_export_delta(H(h), n, B(gidx), flags, cap, B(oRows), capGone, B(oGone), (gpx_delta_counts*)B(counts));
}
JFN(jint, applyDelta)(JNIEnv* env, jclass c, jlong h, jint nRows, jobject rows, jobject gidx, jint flags, jobject status,
                      jint nGone, jobject gone, jobject goneStatus) {
  (void)c;
  return gpx_group_apply_delta(H(h), nRows, B(rows), B(gidx), flags, B(status), nGone, B(gone), B(goneStatus));
}
/* checkpoint transfer (include/gpx_checkpoint.h): every column a direct buffer of n entries, counts = one of 16 bytes;
 * under GPX_CP_PEEK the three run columns may be null */
JFN(jint, checkpointBatch)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject cpSlot, jint flags,
                           jobject oFrom, jobject oTo, jobject oFlags, jobject status, jobject xGidx, jobject xFirst,
                           jobject xCount, jobject counts) {
  (void)c;
  return gpx_checkpoint_batch(H(h), n, B(gidx), B(cpSlot), flags, B(oFrom), B(oTo), B(oFlags), B(status), B(xGidx),
                              B(xFirst), B(xCount), (gpx_cp_counts*)B(counts));
}
/* the view change in list form (include/gpx_viewchange.h): the dense columns direct buffers of n entries, pvOff one of
 * n + 1, the pv columns of capEntries entries, counts = one of 32 bytes; vKind / status of prepareReplyLists may be null.
 * prepareLists' (pvOff, pvSlot, pvBnum, pvBcoord) are prepareReplyLists' pv inputs as they stand (plus a handle column) */
JFN(jint, prepareLists)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject bnum, jobject bcoord,
                        jobject firstSlot, jobject rBnum, jobject rBcoord, jobject rGc, jobject rFlags, jobject status,
                        jint capEntries, jobject pvOff, jobject pvSlot, jobject pvBnum, jobject pvBcoord, jobject counts) {
  (void)c;
  return gpx_prepare_lists(H(h), n, B(gidx), B(bnum), B(bcoord), B(firstSlot), B(rBnum), B(rBcoord), B(rGc), B(rFlags),
                           B(status), capEntries, B(pvOff), B(pvSlot), B(pvBnum), B(pvBcoord), (gpx_pl_counts*)B(counts));
}
JFN(jint, prepareReplyLists)(JNIEnv* env, jclass c, jlong h, jint n, jobject gidx, jobject acceptor, jobject rBnum,
                             jobject rBcoord, jobject firstSlot, jobject pvOff, jobject pvSlot, jobject pvBnum,
                             jobject pvBcoord, jobject pvHandle, jobject pvFlags, jobject vKind, jobject status,
                             jint capHits, jint capEntries, jobject hRec, jobject hGidx, jobject hKind, jobject hStatus,
                             jobject hMedian, jobject hOff, jobject hCount, jobject eSlot, jobject eKind, jobject eHandle,
                             jobject eFlags, jobject counts) {
  (void)c;
  return gpx_prepare_reply_lists(H(h), n, B(gidx), B(acceptor), B(rBnum), B(rBcoord), B(firstSlot), B(pvOff), B(pvSlot),
                                 B(pvBnum), B(pvBcoord), B(pvHandle), B(pvFlags), B(vKind), B(status), capHits, capEntries,
                                 B(hRec), B(hGidx), B(hKind), B(hStatus), B(hMedian), B(hOff), B(hCount), B(eSlot),
                                 B(eKind), B(eHandle), B(eFlags), (gpx_prl_counts*)B(counts));
}
JFN(jint, prepareReplyListsMore)(JNIEnv* env, jclass c, jlong h, jint fromHit, jint capHits, jint capEntries, jobject hRec,
                                 jobject hGidx, jobject hKind, jobject hStatus, jobject hMedian, jobject hOff,
                                 jobject hCount, jobject eSlot, jobject eKind, jobject eHandle, jobject eFlags,
                                 jobject counts) {
  (void)c;
  return gpx_prepare_reply_lists_more(H(h), fromHit, capHits, capEntries, B(hRec), B(hGidx), B(hKind), B(hStatus),
                                      B(hMedian), B(hOff), B(hCount), B(eSlot), B(eKind), B(eHandle), B(eFlags),
                                      (gpx_prl_counts*)B(counts));
}
#endif /* GPX_HAVE_JNI */

/* header drift check, compiled with or without a JDK: the shim's calls above must match these
 * prototypes (a mismatch in include/gpx.h breaks this translation unit) */
typedef int (*gpx_jni_check_ar)(gpx_engine*, int32_t, const int32_t*, const int32_t*, const int32_t*,
                                const int32_t*, const int32_t*, const int32_t*, int32_t*, int32_t*,
                                int32_t*, int32_t*, int32_t*, uint8_t*, int32_t*, uint8_t*);
static gpx_jni_check_ar gpx_jni_check_ar_ = gpx_accept_reply_batch;
typedef int (*gpx_jni_check_pk)(gpx_engine*, const gpx_packed_votes*, int32_t*, int32_t*, int32_t*, int32_t*, int32_t*,
                                uint8_t*, int32_t*, uint8_t*, gpx_ticket*);
static gpx_jni_check_pk gpx_jni_check_pk_ = gpx_accept_reply_packed_async;
void* gpx_jni_selfcheck(void) { return gpx_jni_check_pk_ ? (void*)gpx_jni_check_ar_ : (void*)0; }
