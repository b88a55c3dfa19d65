// Journal batches (include/gpx_journal.h): the ACCEPTs that must be logged, as one contiguous run of
// <be32 len><frame bytes> entries with one index row per entry - SQLPaxosLogger.journal()'s loop (SQLPaxosLogger.java:
// 965-1079) and FileLogger::logBatch (gigapaxos_amd/host/gpx_host.cpp) over frames that are already in HBM.
//
// The four launches, the caps rule, the copy's rounds, the scratch invariant and the bounds argument: gpx_bytes.hip.h.
// What is this family's own:
//
//   k_jr_tile     the selection (status == GPX_S_OK and GPX_R_TOLOG) and the frame test (every index and range BEFORE
//                 any byte of a frame could be read); an entry is 4 + len bytes.  Per tile: entries, refused frames and
//                 bytes in tile_cnt / tile_bad / tile_bytes.
//   k_jr_offsets  tile_eoff / tile_boff, *counts; n_done and bytes_done exact under both caps.
//   k_jr_rows     the e_* rows and one source descriptor (output position, source position, length) per done entry.
//   k_jr_copy     copy_runs over the done entries: [0, n_done) descriptors, bytes_done bytes.
//
// Entries are NOT padded.  An entry is at least 4 bytes, so an output dword touches at most two entries: the tail of one
// and (part of) the length prefix of the next; a prefix can straddle a dword, a 16-byte chunk and a tile.  jr_dword
// builds such a dword from at most three single source bytes and the two prefixes.
//
// Cache policy: the frame bytes and `out` are touched once and go through the stream_* helpers (GPX_NT_JOURNAL of
// GPX_NT_STREAMS, gpx_kernels.hip.h).  The descriptors and the per-tile words are hand-offs between the launches and the
// e_* rows are the caller's: plain.
//
// Bounds, beyond gpx_bytes.hip.h's: a source byte lies inside a frame range that k_jr_tile's test accepted, i.e. inside
// the window [win_lo, win_hi) that `frames` holds; the aligned words load4_unaligned reads hold at least one such byte.
// Includes gpx_bytes.hip.h itself: whatever included this header alone before the core existed still builds.
#pragma once

#include "gpx_bytes.hip.h"

#define GPX_JR_TILE GPX_BLOCK /* records per workgroup: one per lane */
#define GPX_JR_CTILE GPX_BYTES_TILE /* output bytes per workgroup step of k_jr_copy */
#define GPX_JR_SPAN GPX_BYTES_SPAN  /* descriptors staged per round: one per lane */
#define GPX_JR_COUNT_ONLY_ 1  /* == GPX_JR_COUNT_ONLY of include/gpx_journal.h (checked in gpx_journal_dev.inc) */
#define GPX_JR_MAX_LEN 0x7ffffffbll /* INT32_MAX - 4: the prefix and the entry size fit 32 bits */

struct JrCounts { /* == gpx_journal_counts */
  int32_t n_entries, n_done, n_bad, reserved;
  long long n_bytes, bytes_done;
};

struct JrIn {
  const uint8_t* frames; /* device memory that holds bytes [win_lo, win_hi) of the caller's block; frames[0] = byte win_lo */
  long long win_lo, win_hi; /* the _dev form: [0, frames_bytes); the host twin: the window it staged */
  int32_t n_frames;
  const long long* frame_off;
  const int32_t *frame_len, *rec_frame;
  const int32_t *gidx, *slot, *bnum, *bcoord;
  const uint8_t *r_flags, *status;
  int32_t n, rec_base; /* record i of this launch is record rec_base + i of the caller's call (host twin: chunks) */
};

struct JrMem {
  int32_t *tile_cnt, *tile_bad, *tile_eoff; /* [tiles] */
  long long *tile_bytes, *tile_boff;        /* [tiles] */
  long long *d_pos, *d_src;                 /* [max_batch] per done entry: pos(e); its frame's first byte in the window */
  int32_t* d_len;                           /* [max_batch] */
};

struct JrOut {
  uint8_t* out;
  long long cap_bytes, base_offset;
  int32_t cap_entries;
  int32_t *e_rec, *e_gidx, *e_slot, *e_bnum, *e_bcoord;
  long long* e_off;
  int32_t* e_len;
};

struct JrRec {
  bool sel, bad; /* an entry; marked to log but refused */
  int32_t len;
  long long src; /* the frame's first byte in the caller's block */
};

/* Record i: selected? usable?  Nothing of `frames` is touched here: indices and ranges only. */
__device__ __forceinline__ JrRec jr_eval(const JrIn& I, long long i) {
  JrRec r{false, false, 0, 0};
  if (i >= I.n) return r;
  if (I.status[i] != GPX_S_OK || !(I.r_flags[i] & GPX_R_TOLOG)) return r;
  r.bad = true;
  const int32_t f = I.rec_frame ? I.rec_frame[i] : I.rec_base + (int32_t)i;
  if ((uint32_t)f >= (uint32_t)I.n_frames) return r;
  const long long s = I.frame_off[f];
  if (s < 0) return r;
  long long L;
  if (I.frame_len) {
    L = I.frame_len[f];
  } else {
    const long long e = I.frame_off[f + 1];
    if (e < s) return r;
    L = e - s; /* both non-negative: no overflow */
  }
  if (L < 0 || L > GPX_JR_MAX_LEN || s < I.win_lo || s > I.win_hi - L) return r;
  r.bad = false;
  r.sel = true;
  r.len = (int32_t)L;
  r.src = s;
  return r;
}

__global__ __launch_bounds__(GPX_BLOCK) void k_jr_tile(JrIn I, JrMem M) {
  const JrRec r = jr_eval(I, (long long)blockIdx.x * GPX_JR_TILE + (long long)threadIdx.x);
  const Scan64 S = block_scan64(r.sel, r.bad, r.sel ? 4ll + r.len : 0ll);
  if (threadIdx.x == 0) {
    M.tile_cnt[blockIdx.x] = S.tot_c;
    M.tile_bad[blockIdx.x] = S.tot_b;
    M.tile_bytes[blockIdx.x] = S.tot_v;
  }
}

/* one workgroup: the tiles' bases, the counts, and - where a cap cuts - the exact prefix that is done */
__global__ __launch_bounds__(GPX_BLOCK) void k_jr_offsets(int32_t ntiles, JrIn I, JrMem M, long long cap_bytes,
                                                         int32_t cap_entries, int32_t flags,
                                                         JrCounts* __restrict__ counts) {
  int32_t run_c = 0, run_bad = 0, cut = INT32_MAX, cut_e[1] = {0};
  long long run_v = 0, cut_b = 0;
  for (int32_t t0 = 0; t0 < ntiles; t0 += GPX_BLOCK) {
    const int32_t t = t0 + (int32_t)threadIdx.x;
    const int32_t c = t < ntiles ? M.tile_cnt[t] : 0, b = t < ntiles ? M.tile_bad[t] : 0;
    const long long v = t < ntiles ? M.tile_bytes[t] : 0;
    const Scan64 S = block_scan64(c, b, v);
    const int32_t eo = run_c + S.ex_c; /* <= n: fits */
    const long long bo = run_v + S.ex_v;
    if (t < ntiles) {
      M.tile_eoff[t] = eo;
      M.tile_boff[t] = bo;
      /* a lane's tiles come in ascending order */
      if (cut == INT32_MAX && caps_cut(c, v, eo, bo, cap_entries, cap_bytes)) cut = t, cut_e[0] = eo, cut_b = bo;
    }
    run_c += S.tot_c, run_bad += S.tot_b, run_v += S.tot_v;
  }
  const int32_t first = caps_first_cut(cut, cut_b, cut_e);
  int32_t n_done = run_c;
  long long bytes_done = run_v;
  if (first != INT32_MAX) { /* the same in every lane */
    const JrRec r = jr_eval(I, (long long)first * GPX_JR_TILE + (long long)threadIdx.x);
    const long long v = r.sel ? 4ll + r.len : 0ll;
    const bool done = caps_done(r.sel, v, cut_e[0], cut_b, cap_entries, cap_bytes);
    const Scan64 D = block_scan64(done, 0, done ? v : 0ll);
    n_done = cut_e[0] + D.tot_c;
    bytes_done = cut_b + D.tot_v;
  }
  if (flags & GPX_JR_COUNT_ONLY_) n_done = 0, bytes_done = 0;
  if (threadIdx.x == 0) *counts = JrCounts{run_c, n_done, run_bad, 0, run_v, bytes_done};
}

__global__ __launch_bounds__(GPX_BLOCK) void k_jr_rows(JrIn I, JrMem M, JrOut O, const JrCounts* __restrict__ counts) {
  const int32_t n_done = counts->n_done, e0 = M.tile_eoff[blockIdx.x];
  if (e0 >= n_done) return; /* the whole workgroup: nothing of this tile is done */
  const long long i = (long long)blockIdx.x * GPX_JR_TILE + (long long)threadIdx.x;
  const JrRec r = jr_eval(I, i);
  const Scan64 S = block_scan64(r.sel, 0, r.sel ? 4ll + r.len : 0ll);
  const int32_t e = e0 + S.ex_c;
  if (!r.sel || e >= n_done) return;
  const long long pos = M.tile_boff[blockIdx.x] + S.ex_v;
  if (O.e_rec) O.e_rec[e] = I.rec_base + (int32_t)i;
  if (O.e_gidx) O.e_gidx[e] = I.gidx[i];
  if (O.e_slot) O.e_slot[e] = I.slot[i];
  if (O.e_bnum) O.e_bnum[e] = I.bnum[i];
  if (O.e_bcoord) O.e_bcoord[e] = I.bcoord[i];
  O.e_off[e] = O.base_offset + pos;
  O.e_len[e] = r.len;
  M.d_pos[e] = pos;
  M.d_src[e] = r.src - I.win_lo;
  M.d_len[e] = r.len;
}

struct JrTile { /* LDS: one round of descriptors */
  long long pos[GPX_JR_SPAN], src[GPX_JR_SPAN];
  int32_t len[GPX_JR_SPAN];
};

/* The output dword at position Q, which lies inside staged entry k (pos[k] <= Q < pos[k] + 4 + len[k]); ns entries are
 * staged.  Bytes of the entry behind k come from its prefix alone (it is at least 4 bytes long); where that entry is not
 * staged it starts at or beyond the end of what the caller stores, and those bytes stay 0. */
__device__ __forceinline__ uint32_t jr_dword(const JrTile& T, const uint8_t* frames, int32_t k, int32_t ns, long long Q) {
  const long long r = Q - T.pos[k], L = 4ll + T.len[k];
  if (r >= 4 && r + 4 <= L) return load4_unaligned<GPX_NT_JOURNAL>(frames + T.src[k] + (r - 4));
  uint32_t w = 0;
  if (r < 4) w = __builtin_bswap32((uint32_t)T.len[k]) >> (8 * (int32_t)r); /* be32(len), bytes r .. 3 */
  const long long b0 = r > 4 ? r : 4, b1 = r + 4 < L ? r + 4 : L;
  for (long long o = b0; o < b1; o++) w |= (uint32_t)frames[T.src[k] + (o - 4)] << (8 * (int32_t)(o - r));
  if (r + 4 > L && k + 1 < ns) w |= __builtin_bswap32((uint32_t)T.len[k + 1]) << (8 * (int32_t)(L - r));
  return w;
}

struct JrCopy { /* copy_runs' family: one descriptor per done entry */
  typedef JrTile Tile;
  const uint8_t* frames;
  const JrMem& M;
  __device__ __forceinline__ void stage(JrTile& T, int32_t e, int32_t s) const {
    T.src[s] = M.d_src[e];
    T.len[s] = M.d_len[e];
  }
  __device__ __forceinline__ void chunk(const JrTile& T, long long P, long long Pe, int32_t k, int32_t ns,
                                        uint32_t (&w)[4]) const {
#pragma unroll
    for (int32_t d = 0; d < 4; d++) {
      const long long Q = P + 4 * d;
      while (k + 1 < ns && T.pos[k + 1] <= Q) k++;
      w[d] = Q < Pe ? jr_dword(T, frames, k, ns, Q) : 0u;
    }
  }
};

__global__ __launch_bounds__(GPX_BLOCK) void k_jr_copy(const uint8_t* __restrict__ frames, JrMem M,
                                                      uint8_t* __restrict__ out, const JrCounts* __restrict__ counts) {
  copy_runs(JrCopy{frames, M}, M.d_pos, counts->n_done, out, counts->bytes_done);
}
