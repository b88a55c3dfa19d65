// Retransmission sweep (include/gpx_timers.h): find the ACCEPTs and PREPAREs that have waited for replies longer than
// their threshold, hand back their poke rows compacted in entry order and re-arm exactly the ones handed back.
//
// A call is three launches on one stream, the scheme of gpx_scan.hip.h and gpx_sweep.hip.h; no workgroup ever waits
// for another one:
//
//   k_rtx_tile     one workgroup per GPX_RTX_TILE consecutive entries, consecutive lanes on consecutive entries.  The
//                  entry's three timer words (key, since, count) are loaded first, then the entry is evaluated ONCE by
//                  poke_scan_row (gpx_elect.hip.h, the function k_poke_scan calls).  A wait with a new key is armed
//                  here, a group that waits for nothing is disarmed here: neither depends on `cap`.  A wait whose key
//                  is the stored one and whose age exceeds its threshold is a hit and parks (group, waited, count) at
//                  its rank inside the tile.  The tile's hit, no-group and waiting counts go to tile_hits / tile_nog /
//                  tile_wait [tile], unconditionally.
//   k_rtx_offsets  ONE workgroup: exclusive prefix of tile_hits into tile_off, the sums and n_fired into *counts.
//   k_rtx_move     one workgroup per tile: parked hit j of tile t is output entry o = tile_off[t] + j while o < cap.
//                  The lane evaluates its group's poke row again (no group state has changed since the first launch:
//                  the stream orders the three, and only timer words are written), writes the columns and then -
//                  unless the call only peeks - re-arms the group: count + 1 saturating at 255, since = now.  THE ONLY
//                  PLACE A HIT'S WORDS CHANGE: which hits fit `cap` is known only after the offsets.
//
// The thresholds travel in the kernel arguments (RtxCfg, 260 bytes) and are read with a lane-uniform index: the loop
// over the steps is the same in every lane, a lane keeps the entry of its own step.
//
// SCRATCH INVARIANT, as in gpx_scan.hip.h: every scratch word a call reads is one the SAME call wrote.  k_rtx_offsets
// reads tile_hits / tile_nog / tile_wait [0, ntiles): each written unconditionally by its tile's workgroup.  k_rtx_move
// reads tile_hits[t], tile_off[t] (written for every t < ntiles) and parked entries j < tile_hits[t] of tile t.  The
// timer words are not scratch: they are engine state, zeroed when allocated, and only these kernels touch them.
//
// Bounds: a parked entry sits at tile * GPX_RTX_TILE + rank with rank < GPX_RTX_TILE; the parked columns hold
// max(max_groups, max_batch) entries rounded up to whole tiles and the host refuses a larger n.  The timer words are
// indexed by a group number only after it has been checked against S.G; a parked group is one of those (poke_scan_row
// answers GPX_S_NOGROUP for every other).  An output index is below min(n_hits, cap).
//
// Distinct entries (a precondition, as for the pause sweep): two entries naming one group would race on its timer
// words and could both park it.
#pragma once

#define GPX_RTX_TILE 1024
#define GPX_RTX_WAVES (GPX_BLOCK / 64)
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

/* lanes of this wave below the caller's whose bit is set in m */
__device__ __forceinline__ int32_t rtx_rank_below(unsigned long long m) {
  return (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

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
  __shared__ int32_t w_cnt[2][3][GPX_RTX_WAVES];
  const int32_t t0 = (int32_t)blockIdx.x * GPX_RTX_TILE; /* n <= 2^31 - 1: the last tile's base fits */
  const int32_t wave = (int32_t)threadIdx.x >> 6;
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
    const unsigned long long mh = __ballot(hit), mn = __ballot(ng), mw = __ballot(wt);
    /* two sets of LDS words, used alternately: one barrier per pass */
    if ((threadIdx.x & 63) == 0) {
      w_cnt[pass & 1][0][wave] = __popcll(mh);
      w_cnt[pass & 1][1][wave] = __popcll(mn);
      w_cnt[pass & 1][2][wave] = __popcll(mw);
    }
    __syncthreads();
    int32_t before = 0, total = 0;
#pragma unroll
    for (int32_t q = 0; q < GPX_RTX_WAVES; q++) {
      const int32_t c = w_cnt[pass & 1][0][q];
      before += q < wave ? c : 0;
      total += c;
      nog += w_cnt[pass & 1][1][q];
      wtg += w_cnt[pass & 1][2][q];
    }
    if (hit) {
      const int32_t p = t0 + base + before + rtx_rank_below(mh);
      M.park_g[p] = g;
      M.park_wait[p] = waited;
      M.park_count[p] = (uint8_t)c0;
    }
    base += total;
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
  __shared__ int32_t w_sum[3][GPX_RTX_WAVES];
  const int32_t lane = (int32_t)threadIdx.x & 63, wave = (int32_t)threadIdx.x >> 6;
  int32_t running = 0, nog = 0, wtg = 0;
  for (int32_t t0 = 0; t0 < ntiles; t0 += GPX_BLOCK) {
    const int32_t t = t0 + (int32_t)threadIdx.x;
    const int32_t c = t < ntiles ? M.tile_hits[t] : 0;
    int32_t ng = t < ntiles ? M.tile_nog[t] : 0;
    int32_t wt = t < ntiles ? M.tile_wait[t] : 0;
    int32_t inc = c; /* inclusive prefix within the wave */
#pragma unroll
    for (int32_t d = 1; d < 64; d <<= 1) {
      const int32_t v = __shfl_up(inc, d);
      const int32_t u = __shfl_xor(ng, d);
      const int32_t x = __shfl_xor(wt, d);
      if (lane >= d) inc += v;
      ng += u; /* butterflies: every lane ends with the wave's sum */
      wt += x;
    }
    if (lane == 63) {
      w_sum[0][wave] = inc;
      w_sum[1][wave] = ng;
      w_sum[2][wave] = wt;
    }
    __syncthreads();
    int32_t before = 0, total = 0;
#pragma unroll
    for (int32_t q = 0; q < GPX_RTX_WAVES; q++) {
      before += q < wave ? w_sum[0][q] : 0;
      total += w_sum[0][q];
      nog += w_sum[1][q];
      wtg += w_sum[2][q];
    }
    if (t < ntiles) M.tile_off[t] = running + before + inc - c;
    running += total;
    __syncthreads(); /* w_sum is rewritten by the next round */
  }
  if (threadIdx.x == 0) *counts = RtxCounts{running, nog, wtg, (flags & GPX_RTX_PEEK_) ? 0 : min(running, cap)};
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
  const int32_t c = M.tile_hits[blockIdx.x], off = M.tile_off[blockIdx.x];
  const int32_t lim = min(c, cap - off); /* off <= n_hits <= 2^31 - 1, cap >= 0: no overflow */
  const int32_t p0 = (int32_t)blockIdx.x * GPX_RTX_TILE;
  for (int32_t j = (int32_t)threadIdx.x; j < lim; j += GPX_BLOCK) {
    const int32_t g = M.park_g[p0 + j], o = off + j;
    const int32_t c0 = (int32_t)M.park_count[p0 + j], c1 = min(c0 + 1, GPX_RTX_COUNT_MAX);
    const int32_t waited = M.park_wait[p0 + j];
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
