// Deactivation sweep (include/gpx_sweep.h): find the idle, caught-up groups, hand back their restore rows compacted in
// entry order and pause exactly the ones handed back.
//
// A call is three launches on one stream, the scheme of gpx_scan.hip.h; no workgroup ever waits for another one:
//
//   k_sweep_tile     one workgroup per GPX_SWEEP_TILE consecutive entries, consecutive lanes on consecutive entries.
//                    Every entry is evaluated ONCE (sweep_eval, gpx_kernels.hip.h: the pause test of k_group_retire and
//                    the signature in one pass over the group's words), its idle words (signature, age) are brought up
//                    to date, and a hit parks (group, age) at its rank inside the tile.  The tile's hit, no-group and
//                    busy counts go to tile_hits / tile_nog / tile_busy [tile].  NO GROUP STATE CHANGES HERE: which hits
//                    fit `cap` is not known yet, and a group that does not fit must stay alive.
//   k_sweep_offsets  ONE workgroup: exclusive prefix of tile_hits into tile_off, the sums and n_paused into *counts.
//   k_sweep_move     one workgroup per tile: parked hit j of tile t is output entry o = tile_off[t] + j while o < cap.
//                    The lane writes o_gidx[o], o_age[o], builds the restore row AT o_rows[o] (fill_hri_dev, the row of
//                    k_group_retire) and then - unless the call only peeks - pauses the group as k_group_retire does
//                    (group_retire_apply) and clears its idle words.
//
// SCRATCH INVARIANT, as in gpx_scan.hip.h: every scratch word a call reads is one the SAME call wrote.  k_sweep_offsets
// reads tile_hits / tile_nog / tile_busy [0, ntiles): each written unconditionally by its tile's workgroup.
// k_sweep_move reads tile_hits[t], tile_off[t] (written for every t < ntiles) and parked entries j < tile_hits[t] of
// tile t.  The idle words are not scratch: they are engine state, zeroed when allocated, and only these kernels touch
// them.
//
// Bounds: a parked entry sits at tile * GPX_SWEEP_TILE + rank with rank < GPX_SWEEP_TILE; the parked columns hold
// max(max_groups, max_batch) entries rounded up to whole tiles and the host refuses a larger n.  The idle words are
// indexed by a group number only after it has been checked against S.G (sweep_eval answers SWEEP_NOGROUP otherwise;
// a parked group is a live one).  An output index is below min(n_hits, cap).
//
// Distinct entries (a precondition, as for gpx_election_begin_dev): two entries naming one group would race on its
// idle words and could both park it.
#pragma once

#define GPX_SWEEP_TILE 1024
#define GPX_SWEEP_WAVES (GPX_BLOCK / 64)
#define GPX_SWEEP_PEEK_ 1 /* == GPX_SWEEP_PEEK / GPX_SWEEP_HOLD of include/gpx_sweep.h (checked in gpx_sweep_dev.inc) */
#define GPX_SWEEP_HOLD_ 2

struct SweepCounts { /* == gpx_sweep_counts */
  int32_t n_hits, n_nogroup, n_busy, n_paused;
};

/* engine-owned words of the sweep: the idle words over max_groups, the parked hits, the per-tile words */
struct SweepMem {
  uint32_t* sig;     /* [G] signature at the last sweep that saw the group caught up; 0 = none */
  uint8_t* age;      /* [G] sweeps in a row that found the signature unchanged, saturating at 255 */
  int32_t* park_g;   /* [whole tiles] */
  uint8_t* park_age; /* [whole tiles] */
  int32_t *tile_hits, *tile_nog, *tile_busy, *tile_off; /* [tiles] */
};

/* lanes of this wave below the caller's whose bit is set in m */
__device__ __forceinline__ int32_t sweep_rank_below(unsigned long long m) {
  return (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(GPX_BLOCK) void k_sweep_tile(DevState S, int32_t n, const int32_t* __restrict__ gidx,
                                                         int32_t min_age, int32_t flags, SweepMem M) {
  __shared__ int32_t w_cnt[2][3][GPX_SWEEP_WAVES];
  const int32_t t0 = (int32_t)blockIdx.x * GPX_SWEEP_TILE; /* n <= 2^31 - 1: the last tile's base fits */
  const int32_t wave = (int32_t)threadIdx.x >> 6;
  const bool peek = (flags & GPX_SWEEP_PEEK_) != 0, hold = (flags & GPX_SWEEP_HOLD_) != 0;
  int32_t base = 0, nog = 0, bsy = 0; /* the tile's counts of the passes so far: the same in every lane */
#pragma unroll 1 /* one copy of the evaluation, as in k_scan_tile */
  for (int32_t pass = 0; pass < GPX_SWEEP_TILE / GPX_BLOCK; pass++) {
    const int64_t i = (int64_t)t0 + pass * GPX_BLOCK + (int32_t)threadIdx.x;
    bool hit = false, ng = false, bz = false;
    int32_t g = 0, age = 0;
    if (i < n) {
      g = gidx ? gidx[i] : (int32_t)i;
      const bool in = (uint32_t)g < (uint32_t)S.G;
      /* the stored words first: their loads are in flight while the group is evaluated */
      const uint32_t s0 = in ? M.sig[g] : 0u;
      const int32_t a0 = in ? (int32_t)M.age[g] : 0;
      const SweepRow r = sweep_eval(S, g);
      uint32_t s1 = s0;
      if (r.kind == SWEEP_CAUGHT) {
        age = r.sig == s0 ? (hold ? a0 : min(a0 + 1, 255)) : 0;
        s1 = r.sig;
        hit = age >= min_age;
      } else {
        ng = r.kind == SWEEP_NOGROUP;
        bz = r.kind == SWEEP_BUSY;
        if (ng) s1 = 0u;
      }
      if (in && !peek) { /* stores only where a word changes: a table at rest is read, not written */
        if (s1 != s0) M.sig[g] = s1;
        if (age != a0) M.age[g] = (uint8_t)age;
      }
    }
    const unsigned long long mh = __ballot(hit), mn = __ballot(ng), mb = __ballot(bz);
    /* two sets of LDS words, used alternately: one barrier per pass */
    if ((threadIdx.x & 63) == 0) {
      w_cnt[pass & 1][0][wave] = __popcll(mh);
      w_cnt[pass & 1][1][wave] = __popcll(mn);
      w_cnt[pass & 1][2][wave] = __popcll(mb);
    }
    __syncthreads();
    int32_t before = 0, total = 0;
#pragma unroll
    for (int32_t q = 0; q < GPX_SWEEP_WAVES; q++) {
      const int32_t c = w_cnt[pass & 1][0][q];
      before += q < wave ? c : 0;
      total += c;
      nog += w_cnt[pass & 1][1][q];
      bsy += w_cnt[pass & 1][2][q];
    }
    if (hit) {
      const int32_t p = t0 + base + before + sweep_rank_below(mh);
      M.park_g[p] = g;
      M.park_age[p] = (uint8_t)age;
    }
    base += total;
  }
  if (threadIdx.x == 0) {
    M.tile_hits[blockIdx.x] = base;
    M.tile_nog[blockIdx.x] = nog;
    M.tile_busy[blockIdx.x] = bsy;
  }
}

/* one workgroup: tile_off = exclusive prefix of tile_hits, *counts = the sums and what the move step will pause */
__global__ __launch_bounds__(GPX_BLOCK) void k_sweep_offsets(int32_t ntiles, SweepMem M, int32_t cap, int32_t flags,
                                                            SweepCounts* __restrict__ counts) {
  __shared__ int32_t w_sum[3][GPX_SWEEP_WAVES];
  const int32_t lane = (int32_t)threadIdx.x & 63, wave = (int32_t)threadIdx.x >> 6;
  int32_t running = 0, nog = 0, bsy = 0;
  for (int32_t t0 = 0; t0 < ntiles; t0 += GPX_BLOCK) {
    const int32_t t = t0 + (int32_t)threadIdx.x;
    const int32_t c = t < ntiles ? M.tile_hits[t] : 0;
    int32_t ng = t < ntiles ? M.tile_nog[t] : 0;
    int32_t bz = t < ntiles ? M.tile_busy[t] : 0;
    int32_t inc = c; /* inclusive prefix within the wave */
#pragma unroll
    for (int32_t d = 1; d < 64; d <<= 1) {
      const int32_t v = __shfl_up(inc, d);
      const int32_t u = __shfl_xor(ng, d);
      const int32_t x = __shfl_xor(bz, d);
      if (lane >= d) inc += v;
      ng += u; /* butterflies: every lane ends with the wave's sum */
      bz += x;
    }
    if (lane == 63) {
      w_sum[0][wave] = inc;
      w_sum[1][wave] = ng;
      w_sum[2][wave] = bz;
    }
    __syncthreads();
    int32_t before = 0, total = 0;
#pragma unroll
    for (int32_t q = 0; q < GPX_SWEEP_WAVES; q++) {
      before += q < wave ? w_sum[0][q] : 0;
      total += w_sum[0][q];
      nog += w_sum[1][q];
      bsy += w_sum[2][q];
    }
    if (t < ntiles) M.tile_off[t] = running + before + inc - c;
    running += total;
    __syncthreads(); /* w_sum is rewritten by the next round */
  }
  if (threadIdx.x == 0)
    *counts = SweepCounts{running, nog, bsy, (flags & GPX_SWEEP_PEEK_) ? 0 : min(running, cap)};
}

__global__ __launch_bounds__(GPX_BLOCK) void k_sweep_move(DevState S, SweepMem M, NameCopies names, int32_t cap,
                                                         int32_t flags, int32_t* __restrict__ o_gidx,
                                                         uint8_t* __restrict__ o_age, gpx_hri* __restrict__ o_rows) {
  const int32_t c = M.tile_hits[blockIdx.x], off = M.tile_off[blockIdx.x];
  const int32_t lim = min(c, cap - off); /* off <= n_hits <= 2^31 - 1, cap >= 0: no overflow */
  const int32_t p0 = (int32_t)blockIdx.x * GPX_SWEEP_TILE;
  for (int32_t j = (int32_t)threadIdx.x; j < lim; j += GPX_BLOCK) {
    const int32_t g = M.park_g[p0 + j], o = off + j;
    o_gidx[o] = g;
    o_age[o] = M.park_age[p0 + j];
    fill_hri_dev(S, g, S.g_flags[g], &o_rows[o]);
    if (!(flags & GPX_SWEEP_PEEK_)) {
      group_retire_apply(S, g, names);
      M.sig[g] = 0u;
      M.age[g] = 0;
    }
  }
}
