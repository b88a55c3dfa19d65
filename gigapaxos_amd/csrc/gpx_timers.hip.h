// Retransmission sweep (include/gpx_timers.h): find the ACCEPTs and PREPAREs that have waited for replies longer than
// their threshold, hand back their poke rows compacted in entry order and re-arm exactly the ones handed back.
//
// The three launches, the scratch invariant and the bounds argument: gpx_compact.hip.h.  What is this sweep's own:
//
//   k_rtx_tile     GPX_RTX_TILE entries in passes of GPX_BLOCK.  The entry's three timer words (key, since, count) are
//                  loaded first, then the entry is evaluated by poke_scan_row (gpx_elect.hip.h, the function k_poke_scan
//                  calls).  A wait with a new key is armed here, a group that waits for nothing is disarmed here: neither
//                  depends on `cap`.  A wait whose key is the stored one and whose age exceeds its threshold is a hit
//                  and parks (group, waited, count).  The tile's hit, no-group and waiting counts go to tile_hits /
//                  tile_nog / tile_wait [tile].
//   k_rtx_offsets  tile_off = exclusive prefix of tile_hits, the sums and n_fired into *counts.
//   k_rtx_move     the lane evaluates its group's poke row again (no group state has changed since the first launch: the
//                  stream orders the three, and only timer words are written), writes the columns and then - unless the
//                  call only peeks - re-arms the group: count + 1 saturating at 255, since = now.  THE ONLY PLACE A
//                  HIT'S WORDS CHANGE: which hits fit `cap` is known only after the offsets.
//
// The thresholds travel in the kernel arguments (RtxCfg, 260 bytes) and are read with a lane-uniform index: the loop
// over the steps is the same in every lane, a lane keeps the entry of its own step.
//
// The timer words are not scratch: they are engine state, zeroed when allocated, and only these kernels touch them.
// They are indexed by a group number only after it has been checked against S.G; a parked group is one of those
// (poke_scan_row answers GPX_S_NOGROUP for every other).
//
// Distinct entries (a precondition, as for the pause sweep): two entries naming one group would race on its timer
// words and could both park it.
#pragma once

#define GPX_RTX_TILE 1024
#define GPX_RTX_PEEK_ 1       /* == GPX_RTX_PEEK of include/gpx_timers.h (checked in gpx_timers_dev.inc) */
#define GPX_RTX_MAX_STEPS_ 32 /* == GPX_RTX_MAX_STEPS */
#define GPX_RTX_COUNT_MAX 255

struct RtxCounts { /* == gpx_rtx_counts */
  int32_t n_hits, n_nogroup, n_waiting, n_fired;
};

struct RtxCfg { /* == gpx_rtx_cfg */
  int32_t n_steps;
  int32_t accept_ms[GPX_RTX_MAX_STEPS_];
  int32_t prepare_ms[GPX_RTX_MAX_STEPS_];
};

/* engine-owned words of the retransmission sweep: the timer words over max_groups, the parked hits, the per-tile words */
struct RtxMem {
  uint32_t* key;       /* [G] what the group was waiting for at the last sweep that saw it wait; 0 = nothing */
  int32_t* since;      /* [G] the caller's clock when that wait was first seen or last fired */
  uint8_t* count;      /* [G] retransmissions of that wait so far, saturating at 255 */
  int32_t* park_g;     /* [whole tiles] */
  int32_t* park_wait;  /* [whole tiles] */
  uint8_t* park_count; /* [whole tiles] the count BEFORE this retransmission */
  int32_t *tile_hits, *tile_nog, *tile_wait, *tile_off; /* [tiles] */
};

/* The identity of a wait: kind, slot and ballot, never `heard` (a reply does not restart WaitforUtility.initTime).  Odd
 * multipliers and the murmur3 finaliser are bijections: two waits that differ in ONE of the four fields never share a
 * key (a decision that moves the head of line, a higher ballot number, PREPARE turning into ACCEPT).  0 means "no wait". */
__device__ __forceinline__ uint32_t rtx_key(uint32_t poke, int32_t slot, int32_t bnum, int32_t bcoord) {
  uint32_t h = (uint32_t)slot * 0x9e3779b1u ^ (uint32_t)bnum * 0x85ebca77u ^ (uint32_t)bcoord * 0xc2b2ae3du ^
               poke * 0x27d4eb2fu;
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h ? h : 1u;
}

/* the threshold after c retransmissions of a wait of this kind; the index of every table read is the same in all lanes */
__device__ __forceinline__ int32_t rtx_threshold(const RtxCfg& cfg, bool prepare, int32_t c) {
  const int32_t idx = min(c, cfg.n_steps - 1);
  int32_t thr = 0;
  for (int32_t q = 0; q < cfg.n_steps; q++) {
    const int32_t a = cfg.accept_ms[q], p = cfg.prepare_ms[q];
    if (q == idx) thr = prepare ? p : a;
  }
  return thr;
}

template <int KMAX>
__global__ __launch_bounds__(GPX_BLOCK) void k_rtx_tile(DevState S, int32_t n, const int32_t* __restrict__ gidx,
                                                       int32_t now_ms, RtxCfg cfg, int32_t flags, RtxMem M) {
  __shared__ int32_t w_cnt[2][3][GPX_COMPACT_WAVES]; /* two sets, used alternately: one barrier per pass */
  const int32_t t0 = (int32_t)blockIdx.x * GPX_RTX_TILE; /* n <= 2^31 - 1: the last tile's base fits */
  const bool peek = (flags & GPX_RTX_PEEK_) != 0;
  int32_t base = 0, nog = 0, wtg = 0; /* the tile's counts of the passes so far: the same in every lane */
#pragma unroll 1 /* one copy of the evaluation, as in k_scan_tile */
  for (int32_t pass = 0; pass < GPX_RTX_TILE / GPX_BLOCK; pass++) {
    const int64_t i = (int64_t)t0 + pass * GPX_BLOCK + (int32_t)threadIdx.x;
    bool hit = false, ng = false, wt = false;
    int32_t g = 0, waited = 0, c0 = 0;
    if (i < n) {
      g = gidx ? gidx[i] : (int32_t)i;
      const bool in = (uint32_t)g < (uint32_t)S.G;
      /* the stored words first: their loads are in flight while the group is evaluated */
      const uint32_t k0 = in ? M.key[g] : 0u;
      const int32_t s0 = in ? M.since[g] : 0;
      c0 = in ? (int32_t)M.count[g] : 0;
      const PokeRow r = poke_scan_row<KMAX>(S, g);
      uint32_t k1 = 0u;
      int32_t s1 = s0, c1 = 0;
      if (r.status == GPX_S_NOGROUP) {
        ng = true;
        s1 = 0;
      } else if (r.poke != GPX_POKE_NONE) {
        wt = true;
        k1 = rtx_key(r.poke, r.slot, r.bnum, r.bcoord);
        if (k1 != k0) { /* a new wait: armed, not a hit */
          s1 = now_ms;
        } else {
          c1 = c0;
          waited = (int32_t)((uint32_t)now_ms - (uint32_t)s0);
          hit = waited > rtx_threshold(cfg, r.poke == GPX_POKE_PREPARE, c0); /* thresholds are >= 0: never with waited < 0 */
        }
      }
      if (in && !peek) { /* stores only where a word changes: a table at rest is read, not written */
        if (k1 != k0) M.key[g] = k1;
        if (s1 != s0) M.since[g] = s1;
        if (c1 != c0) M.count[g] = (uint8_t)c1;
      }
    }
    const TileCount<3> c = tile_count(w_cnt[pass & 1], {hit, ng, wt});
    if (hit) {
      const int32_t p = t0 + base + c.before[0];
      M.park_g[p] = g;
      M.park_wait[p] = waited;
      M.park_count[p] = (uint8_t)c0;
    }
    base += c.total[0];
    nog += c.total[1];
    wtg += c.total[2];
  }
  if (threadIdx.x == 0) {
    M.tile_hits[blockIdx.x] = base;
    M.tile_nog[blockIdx.x] = nog;
    M.tile_wait[blockIdx.x] = wtg;
  }
}

/* one workgroup: tile_off = exclusive prefix of tile_hits, *counts = the sums and what the move step will re-arm */
__global__ __launch_bounds__(GPX_BLOCK) void k_rtx_offsets(int32_t ntiles, RtxMem M, int32_t cap, int32_t flags,
                                                          RtxCounts* __restrict__ counts) {
  int32_t sum[3];
  tile_offsets<1, 2>(
      ntiles, [&](int32_t t, int32_t(&v)[3]) { v[0] = M.tile_hits[t], v[1] = M.tile_nog[t], v[2] = M.tile_wait[t]; },
      [&](int32_t t, const int32_t(&off)[1], const int32_t(&)[3]) { M.tile_off[t] = off[0]; }, sum);
  if (threadIdx.x == 0) *counts = RtxCounts{sum[0], sum[1], sum[2], (flags & GPX_RTX_PEEK_) ? 0 : min(sum[0], cap)};
}

/* the output columns of one call: gpx_poke_scan's row, then the count after this retransmission and the wait */
struct RtxOut {
  int32_t* gidx;
  uint8_t* poke;
  int32_t *slot, *bnum, *bcoord, *median_cp;
  uint8_t* flags;
  uint32_t* heard;
  uint8_t* count;
  int32_t* waited;
};

template <int KMAX>
__global__ __launch_bounds__(GPX_BLOCK) void k_rtx_move(DevState S, RtxMem M, int32_t now_ms, int32_t cap, int32_t flags,
                                                       RtxOut O) {
  const MoveSpan m = move_span<GPX_RTX_TILE>(M.tile_hits, M.tile_off, cap);
  for (int32_t j = (int32_t)threadIdx.x; j < m.lim; j += GPX_BLOCK) {
    const int32_t g = M.park_g[m.p0 + j], o = m.off + j;
    const int32_t c0 = (int32_t)M.park_count[m.p0 + j], c1 = min(c0 + 1, GPX_RTX_COUNT_MAX);
    const int32_t waited = M.park_wait[m.p0 + j];
    const PokeRow r = poke_scan_row<KMAX>(S, g); /* what k_rtx_tile saw: nothing has changed since */
    O.gidx[o] = g;
    O.poke[o] = r.poke;
    O.slot[o] = r.slot;
    O.bnum[o] = r.bnum;
    O.bcoord[o] = r.bcoord;
    O.median_cp[o] = r.median_cp;
    O.flags[o] = r.flags;
    O.heard[o] = r.heard;
    O.count[o] = (uint8_t)c1;
    O.waited[o] = waited;
    if (!(flags & GPX_RTX_PEEK_)) { /* incrRetransmissonCount(true): the next threshold, counted from now */
      if (c1 != c0) M.count[g] = (uint8_t)c1;
      M.since[g] = now_ms;
    }
  }
}
