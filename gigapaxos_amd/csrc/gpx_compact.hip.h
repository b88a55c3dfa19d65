// The tile-compaction core of the control plane: what the hit-compacting scans (gpx_scan.hip.h), the deactivation sweep
// (gpx_sweep.hip.h), the retransmission sweep (gpx_timers.hip.h), the checkpoint batch (gpx_checkpoint.hip.h), the group
// images (gpx_image.hip.h) and the delta images (gpx_delta.hip.h) have in common.  A family's header holds what is its
// own: the evaluation, what a hit parks, what the move step does with it.
//
// A call is three launches on one stream, and no workgroup ever waits for another one:
//
//   k_*_tile     one workgroup per TILE consecutive entries, consecutive lanes on consecutive entries.  Every entry is
//                evaluated ONCE.  A hit's rank inside the tile is the hits of the tile's earlier passes + the hits of the
//                waves before the lane's + the set lanes of the wave's ballot below the lane (tile_count); the hit is
//                parked at tile base + rank.  The tile's counts go to its per-tile words, unconditionally.
//   k_*_offsets  ONE workgroup: the exclusive prefixes of the per-tile counts that place output, the sums of all of them
//                into the call's counts (tile_offsets); for the weighted exports the exact share of the tile that `cap`
//                cuts (cap_cut).
//   k_*_move     one workgroup per tile: parked entry j of tile t is output entry tile_off[t] + j while that is below
//                `cap` (move_span).  Only hits move; nothing is evaluated twice.
//
// The order between the steps is the stream's.  There are no look-back words, no arrival counters and no assumption
// about residency, so this scheme adds nothing to the epochs of DESIGN.md 3.3 and nothing that can starve on a shared
// device.
//
// SCRATCH INVARIANT: every scratch word a call reads is one the SAME call wrote.  k_*_offsets reads the per-tile counts
// of tiles [0, ntiles): each written unconditionally by its tile's workgroup.  k_*_move reads its tile's count and
// offset (written by k_*_offsets for every t < ntiles) and parked entries j < count of its tile: exactly the ones that
// tile's workgroup wrote.  Nothing is cleared between calls and nothing needs to be.  Words that live on from call to
// call (idle words, timer words, marks) are engine state, not scratch: zeroed when allocated.
//
// Bounds: a parked entry sits at tile * TILE + rank with rank < TILE, and the parked columns hold
// max(max_groups, max_batch) entries rounded up to whole tiles; the host refuses a larger n.  An output index is below
// min(the prefixed total, cap).  A group number indexes state only after it has been checked against S.G.
//
// Everything here is inlined into its kernel, sized at compile time and kept in registers: no array is indexed by a
// run-time value, so none of these kernels has scratch memory.
// Needs: wave_incscan, block_exscan (gpx_kernels.hip.h).
#pragma once

#define GPX_COMPACT_WAVES (GPX_BLOCK / 64)

/* lanes of this wave below the caller's whose bit is set in m */
__device__ __forceinline__ int32_t rank_below(unsigned long long m) {
  return (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

/* One pass of a tile kernel over N predicates of the lane.  before[k]: the lanes of the workgroup before this one whose
 * predicate k holds (the rank of a hit inside the pass); total[k]: the workgroup's count, the same in every lane.  A
 * `before` nobody reads costs nothing once inlined.  `w` is the CALLER's LDS, [N][waves], and there is ONE barrier here,
 * between its writes and its reads.  A kernel of one pass hands in a single block.  A kernel of several passes hands in
 * two blocks alternately: a wave that runs ahead into the next pass then writes the block nobody is still reading, and
 * it cannot run two passes ahead, because the next pass's barrier waits for the slowest wave. */
template <int N>
struct TileCount {
  int32_t before[N], total[N];
};
template <int N>
__device__ __forceinline__ TileCount<N> tile_count(int32_t (*w)[GPX_COMPACT_WAVES], const bool (&pred)[N]) {
  const int32_t wave = (int32_t)threadIdx.x >> 6;
  unsigned long long m[N];
#pragma unroll
  for (int k = 0; k < N; k++) m[k] = __ballot(pred[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; k++) w[k][wave] = __popcll(m[k]);
  }
  __syncthreads();
  TileCount<N> c;
#pragma unroll
  for (int k = 0; k < N; k++) {
    int32_t before = 0, total = 0;
#pragma unroll
    for (int32_t q = 0; q < GPX_COMPACT_WAVES; q++) {
      const int32_t s = w[k][q];
      before += q < wave ? s : 0;
      total += s;
    }
    c.before[k] = before + rank_below(m[k]);
    c.total[k] = total;
  }
  return c;
}

/* The offsets kernel's loop, for ONE workgroup of GPX_BLOCK lanes.  load(t, v) gives tile t's NP + NS words, the NP
 * prefixed ones first; store(t, off, v) gets the NP exclusive prefixes of tile t over tiles [0, t) next to the words
 * loaded.  sum[] returns the NP + NS totals over all tiles, the same in every lane.  Rounds of GPX_BLOCK tiles; with
 * ntiles == 0 nothing is loaded, nothing stored and no barrier passed.  Offsets ascend with t, so a condition like "the
 * tile that cap cuts" holds for at most one store. */
template <int NP, int NS, class Load, class Store>
__device__ __forceinline__ void tile_offsets(int32_t ntiles, Load load, Store store, int32_t (&sum)[NP + NS]) {
  __shared__ int32_t w_sum[NP + NS][GPX_COMPACT_WAVES];
  const int32_t lane = (int32_t)threadIdx.x & 63, wave = (int32_t)threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NP + NS; k++) sum[k] = 0;
  for (int32_t t0 = 0; t0 < ntiles; t0 += GPX_BLOCK) {
    const int32_t t = t0 + (int32_t)threadIdx.x;
    int32_t v[NP + NS] = {}, inc[NP + NS];
    if (t < ntiles) load(t, v);
#pragma unroll
    for (int k = 0; k < NP + NS; k++) inc[k] = wave_incscan(v[k]); /* lane 63: the wave's sum */
    if (lane == 63) {
#pragma unroll
      for (int k = 0; k < NP + NS; k++) w_sum[k][wave] = inc[k];
    }
    __syncthreads();
    int32_t off[NP];
#pragma unroll
    for (int k = 0; k < NP + NS; k++) {
      int32_t before = 0, total = 0;
#pragma unroll
      for (int32_t q = 0; q < GPX_COMPACT_WAVES; q++) {
        const int32_t s = w_sum[k][q];
        before += q < wave ? s : 0;
        total += s;
      }
      if (k < NP) off[k] = sum[k] + before + inc[k] - v[k];
      sum[k] += total;
    }
    if (t < ntiles) store(t, off, v);
    __syncthreads(); /* w_sum is rewritten by the next round */
  }
}

/* The weighted exports (an entry is 1 or 2 rows).  Entry j of a tile whose rows begin at `off` has weight w, 0 for a lane
 * past the tile's entries; it fits iff ALL its rows end at or before cap.  *pre: the rows of the tile's entries before
 * it.  The prefix counts the rows of an entry that does not fit, so nothing after it fits either: the entries that fit
 * are a prefix of the tile's.  Every lane of the workgroup calls this (block_exscan has barriers). */
__device__ __forceinline__ bool weighted_fits(int32_t off, int32_t w, int32_t cap, int32_t* pre) {
  int32_t tot = 0;
  *pre = block_exscan(w, &tot);
  return w > 0 && (int64_t)off + *pre + w <= cap;
}
/* ... and for the tile that `cap` cuts, the entries that fit and their rows: the same in every lane */
struct CapCut {
  int32_t n, rows;
};
__device__ __forceinline__ CapCut cap_cut(int32_t off, int32_t w, int32_t cap) {
  int32_t pre = 0;
  const bool fits = weighted_fits(off, w, cap, &pre);
  CapCut c{0, 0};
  block_exscan(fits ? 1 : 0, &c.n);
  block_exscan(fits ? w : 0, &c.rows);
  return c;
}

/* The head of a move kernel: this workgroup's tile has `lim` parked entries to move, from p0 + j to output entry off + j.
 * off <= the total <= 2^31 - 1 and cap >= 0: no overflow; lim <= 0 where the tile's output begins at or past cap. */
struct MoveSpan {
  int32_t p0, off, lim;
};
template <int TILE>
__device__ __forceinline__ MoveSpan move_span(const int32_t* tile_cnt, const int32_t* tile_off, int32_t cap) {
  const int32_t c = tile_cnt[blockIdx.x], off = tile_off[blockIdx.x];
  return MoveSpan{(int32_t)blockIdx.x * TILE, off, min(c, cap - off)};
}
