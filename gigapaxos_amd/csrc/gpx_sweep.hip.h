// Deactivation sweep (include/gpx_sweep.h): find the idle, caught-up groups, hand back their restore rows compacted in
// entry order and pause exactly the ones handed back.
//
// The three launches, the scratch invariant and the bounds argument: gpx_compact.hip.h.  What is the sweep's own:
//
//   k_sweep_tile     GPX_SWEEP_TILE entries in passes of GPX_BLOCK.  An entry is evaluated by sweep_eval
//                    (gpx_kernels.hip.h: the pause test of k_group_retire and the signature in one pass over the group's
//                    words), its idle words (signature, age) are brought up to date, and a hit parks (group, age).  The
//                    tile's hit, no-group and busy counts go to tile_hits / tile_nog / tile_busy [tile].  NO GROUP STATE
//                    CHANGES HERE: which hits fit `cap` is not known yet, and a group that does not fit must stay alive.
//   k_sweep_offsets  tile_off = exclusive prefix of tile_hits, the sums and n_paused into *counts.
//   k_sweep_move     the lane writes o_gidx[o], o_age[o], builds the restore row AT o_rows[o] (fill_hri_dev, the row of
//                    k_group_retire) and then - unless the call only peeks - pauses the group as k_group_retire does
//                    (group_retire_apply) and clears its idle words.
//
// The idle words are not scratch: they are engine state, zeroed when allocated, and only these kernels touch them.  They
// are indexed by a group number only after it has been checked against S.G (sweep_eval answers SWEEP_NOGROUP otherwise;
// a parked group is a live one).
//
// Distinct entries (a precondition, as for gpx_election_begin_dev): two entries naming one group would race on its
// idle words and could both park it.
#pragma once

#define GPX_SWEEP_TILE 1024
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

__global__ __launch_bounds__(GPX_BLOCK) void k_sweep_tile(DevState S, int32_t n, const int32_t* __restrict__ gidx,
                                                         int32_t min_age, int32_t flags, SweepMem M) {
  __shared__ int32_t w_cnt[2][3][GPX_COMPACT_WAVES]; /* two sets, used alternately: one barrier per pass */
  const int32_t t0 = (int32_t)blockIdx.x * GPX_SWEEP_TILE; /* n <= 2^31 - 1: the last tile's base fits */
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
    const TileCount<3> c = tile_count(w_cnt[pass & 1], {hit, ng, bz});
    if (hit) {
      const int32_t p = t0 + base + c.before[0];
      M.park_g[p] = g;
      M.park_age[p] = (uint8_t)age;
    }
    base += c.total[0];
    nog += c.total[1];
    bsy += c.total[2];
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
  int32_t sum[3];
  tile_offsets<1, 2>(
      ntiles, [&](int32_t t, int32_t(&v)[3]) { v[0] = M.tile_hits[t], v[1] = M.tile_nog[t], v[2] = M.tile_busy[t]; },
      [&](int32_t t, const int32_t(&off)[1], const int32_t(&)[3]) { M.tile_off[t] = off[0]; }, sum);
  if (threadIdx.x == 0)
    *counts = SweepCounts{sum[0], sum[1], sum[2], (flags & GPX_SWEEP_PEEK_) ? 0 : min(sum[0], cap)};
}

__global__ __launch_bounds__(GPX_BLOCK) void k_sweep_move(DevState S, SweepMem M, NameCopies names, int32_t cap,
                                                         int32_t flags, int32_t* __restrict__ o_gidx,
                                                         uint8_t* __restrict__ o_age, gpx_hri* __restrict__ o_rows) {
  const MoveSpan m = move_span<GPX_SWEEP_TILE>(M.tile_hits, M.tile_off, cap);
  for (int32_t j = (int32_t)threadIdx.x; j < m.lim; j += GPX_BLOCK) {
    const int32_t g = M.park_g[m.p0 + j], o = m.off + j;
    o_gidx[o] = g;
    o_age[o] = M.park_age[m.p0 + j];
    fill_hri_dev(S, g, S.g_flags[g], &o_rows[o]);
    if (!(flags & GPX_SWEEP_PEEK_)) {
      group_retire_apply(S, g, names);
      M.sig[g] = 0u;
      M.age[g] = 0;
    }
  }
}
