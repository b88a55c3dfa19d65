// Checkpoint transfer (include/gpx_checkpoint.h): PISM.handleCheckpoint's acceptor half - PaxosAcceptor.jumpSlot, then
// extractExecuteAndCheckpoint(null) - for one record per group, the execution runs compacted in record order.
//
// The three launches, the scratch invariant and the bounds argument: gpx_compact.hip.h.  What is this call's own:
//
//   k_cp_tile<PEEK>  GPX_CP_TILE records, one lane per record.  The lane asks for its record, then for the group's words,
//                    then for the ring entries it will need - the ones the jump walks (fewer than W, or all W of them) and
//                    the one at the slot the tail starts from - in rounds of GPX_CP_ROUND independent 16-byte loads;
//                    applies steps 1-4 of the header and stores the dense outputs.  A run parks (group, first, count).
//                    The tile's four counts go to tile[t], one 16-byte word.  UNLIKE THE SWEEP, STATE CHANGES HERE: no
//                    cap decides which records are applied, so nothing has to wait for the offsets.  PEEK = true loads no
//                    ring entry and stores no state.
//   k_cp_offsets     the exclusive prefix of the tiles' run counts replaces tile[t].x (the adopted count, summed by
//                    then), the four sums go to *counts.
//   k_cp_move        parked run j of tile t is output entry tile[t].x + j: no cap, every run column holds n entries and
//                    n_runs <= n.  Not launched under PEEK (no runs).
//
// A ring index is masked with W - 1.
//
// Distinct groups (a precondition, as for gpx_election_begin_dev): two records naming one group would race on its state.
#pragma once

#define GPX_CP_TILE 256 /* == GPX_BLOCK: one lane per record */
#define GPX_CP_ROUND 4 /* ring entries requested together */
#define GPX_CP_PEEK_ 1 /* == GPX_CP_PEEK / _ADOPT / _MOVED of include/gpx_checkpoint.h (checked in gpx_checkpoint_dev.inc) */
#define GPX_CP_ADOPT_ 1
#define GPX_CP_MOVED_ 2

struct CpCounts { /* == gpx_cp_counts */
  int32_t n_adopted, n_nogroup, n_stopped, n_runs;
};

/* the call's scratch: 12 bytes per record in whole tiles, 16 per tile */
struct CpMem {
  int32_t *park_g, *park_first, *park_count; /* [whole tiles] */
  I4* tile; /* [tiles] {adopted, no group, stopped, runs}; .x becomes the tile's first output entry (k_cp_offsets) */
};

/* PaxosAcceptor.jumpSlot(target) (PaxosAcceptor.java:564-578) for d = target - slot > 0: committedRequests.remove(i)
 * and, from disk, acceptedProposals.remove(i) for every i of [slot, target); executed(i, false) only counts.  A key k
 * lies in that range iff (unsigned)(k - slot) < d, at the int wrap too.  For d < W the keys slot + j sit at ring index
 * (slot + j) & (W - 1): d entries are walked, and one more is read - the one at target, where the tail starts.  For
 * d >= W all W entries are tested.  With d == 0 (no jump) only the entry at the slot is read.  Never a loop over d.
 * Loads go out GPX_CP_ROUND at a time, ahead of the round's stores.  Returns the entry at ring index (slot + d) & (W - 1)
 * as the jump leaves it. */
__device__ __forceinline__ I4 cp_jump(const DevState& S, int32_t g, int32_t slot, int32_t d) {
  const int32_t Wm = S.W - 1;
  const bool from_disk = (S.flags & GPX_F_ACCEPTS_FROM_DISK) != 0;
  const bool all = d >= S.W;
  const int32_t cnt = all ? S.W : d + 1;
  const int32_t base = all ? 0 : slot;
  const int32_t wt = (int32_t)((uint32_t)slot + (uint32_t)d) & Wm;
  int32_t tx = 0, ty = 0, tz = 0, tw = 0; /* the entry at wt, by selects: no address of these is ever taken */
  for (int32_t j0 = 0; j0 < cnt; j0 += GPX_CP_ROUND) {
    I4 e[GPX_CP_ROUND];
    int32_t cx[GPX_CP_ROUND];
#pragma unroll
    for (int q = 0; q < GPX_CP_ROUND; q++) {
      const int32_t w = (int32_t)((uint32_t)base + (uint32_t)(j0 + q)) & Wm;
      const bool on = j0 + q < cnt;
      e[q] = on ? S.acc_ring[(int64_t)w * S.G + g] : mk4(0, 0, 0, 0);
      cx[q] = on ? S.com_ring[(int64_t)w * S.G + g].x : 0;
    }
#pragma unroll
    for (int q = 0; q < GPX_CP_ROUND; q++) {
      const int32_t w = (int32_t)((uint32_t)base + (uint32_t)(j0 + q)) & Wm;
      const bool on = j0 + q < cnt;
      const uint32_t f = (uint32_t)e[q].w;
      const bool com_in = ((f >> CF_SHIFT) & RF_PRESENT) && (uint32_t)jsub(cx[q], slot) < (uint32_t)d;
      const bool acc_in = from_disk && (f & RF_PRESENT) && (uint32_t)jsub(e[q].x, slot) < (uint32_t)d;
      const uint32_t nf = f & ~(com_in ? (uint32_t)CF_MASK : 0u) & ~(acc_in ? (uint32_t)AF_MASK : 0u);
      if (on && nf != f) ((int32_t*)&S.acc_ring[(int64_t)w * S.G + g])[3] = (int32_t)nf;
      const bool hit = on && w == wt;
      tx = hit ? e[q].x : tx;
      ty = hit ? e[q].y : ty;
      tz = hit ? e[q].z : tz;
      tw = hit ? (int32_t)nf : tw;
    }
  }
  return mk4(tx, ty, tz, tw);
}

/* extractExecuteAndCheckpoint(null) (PISM:1619-1701): putAndRemoveNextExecutable(null) until it yields nothing.  Its
 * `decision = committedRequests.get(getSlot())` branch (PaxosAcceptor.java:329-338) collects by the PARKED commit's
 * median - acc_eec collects by the incoming decision's - and puts the commit back where it was (a no-op); from
 * reconstructDecision on the slot executes as in acc_eec.  Loop exits are breaks, as there (see the note at
 * acc_reconstruct on early returns).  Returns the number of slots executed in order from the entry value of a.slot. */
__device__ __forceinline__ int32_t acc_cp_tail(const DevState& S, AccView& V, int32_t g, AccState& a) {
  int32_t count = 0;
  const int32_t Wm = S.W - 1;
  const bool from_disk = (S.flags & GPX_F_ACCEPTS_FROM_DISK) != 0;
  while (!a.stopped) {
    const int32_t wx = a.slot & Wm;
    const I4 e = V.rd(wx);
    if (!(((uint32_t)e.w >> CF_SHIFT) & RF_PRESENT)) break;
    const I4 cr = S.com_ring[(int64_t)wx * S.G + g];
    if (cr.x != a.slot) break; /* committedRequests.get(getSlot()) == null */
    acc_gc(S, V, a, cr.w);
    /* the collection may have taken the commit itself (acc_gc's `far` case): containsKey(getSlot()) is asked again */
    const I4 e2 = V.rd(wx);
    if (!(((uint32_t)e2.w >> CF_SHIFT) & RF_PRESENT)) break;
    Dec nx = Dec{0, 0, 0, 0, false, false};
    if (!acc_reconstruct(S, V, g, a.slot, &nx)) break;
    /* committedRequests.remove(_slot) */
    V.wr_flags(wx, V.rd(wx).w & ~(int32_t)CF_MASK);
    /* executed(slot, isStop) */
    a.slot = (int32_t)((uint32_t)a.slot + 1u);
    if (nx.stop) a.stopped = true;
    if (a.stopped)
      for (int32_t w = 0; w < S.W; w++) { /* committedRequests.clear() (:468-469) */
        const I4 c = V.rd(w);
        if ((uint32_t)c.w & CF_MASK) V.wr_flags(w, c.w & ~(int32_t)CF_MASK);
      }
    if (from_disk) {
      /* acceptedProposals.remove(nextExecutable.slot) (:357-359) */
      const I4 c = V.rd(wx);
      if ((c.w & RF_PRESENT) && c.x == nx.slot) V.wr_flags(wx, c.w & ~(int32_t)AF_MASK);
    }
    count++;
    if (nx.stop) break;
  }
  return count;
}

template <bool PEEK>
__global__ __launch_bounds__(GPX_CP_TILE) void k_cp_tile(DevState S, int32_t n, const int32_t* __restrict__ gidx,
                                                        const int32_t* __restrict__ cp_slot,
                                                        int32_t* __restrict__ o_from, int32_t* __restrict__ o_to,
                                                        uint8_t* __restrict__ o_flags, uint8_t* __restrict__ status,
                                                        CpMem M) {
  __shared__ int32_t w_cnt[4][GPX_COMPACT_WAVES];
  const int32_t t0 = (int32_t)blockIdx.x * GPX_CP_TILE; /* n <= 2^31 - 1: the last tile's base fits */
  const int64_t i = (int64_t)t0 + (int32_t)threadIdx.x;
  bool adopt = false, ng = false, st = false;
  int32_t g = 0, first = 0, count = 0;
  if (i < n) {
    g = gidx[i];
    const int32_t cp = cp_slot[i];
    const bool in = (uint32_t)g < (uint32_t)S.G;
    /* the group's words: independent loads */
    const uint32_t gf = in ? S.g_flags[g] : 0u;
    const int32_t slot = in ? S.a_slot[g] : 0;
    const int32_t gc = in ? S.a_gc[g] : 0;
    ng = !(gf & GF_EXISTS);
    st = !ng && (gf & GF_STOPPED);
    int32_t from = 0, to = 0, fl = 0;
    if (!ng && !st) {
      adopt = cp >= slot; /* PISM:1853: plain, not `cp - slot >= 0` */
      const int32_t target = (int32_t)((uint32_t)cp + 1u);
      const int32_t d = (adopt && jsub(target, slot) > 0) ? jsub(target, slot) : 0; /* jumpSlot moves iff i - target < 0 */
      from = slot;
      if (PEEK) {
        to = (int32_t)((uint32_t)slot + (uint32_t)d);
      } else {
        const I4 et = cp_jump(S, g, slot, d);
        AccState a;
        a.slot = (int32_t)((uint32_t)slot + (uint32_t)d);
        a.bnum = a.bcoord = 0; /* the ballot is neither read nor written here */
        a.gc = gc;
        a.stopped = false;
        AccState a0 = a;
        a0.slot = slot;
        AccView V;
        V.init(S, g);
        V.preset(a.slot & (S.W - 1), et);
        first = a.slot;
        count = acc_cp_tail(S, V, g, a);
        acc_store(S, g, gf, a, a0);
        to = a.slot;
      }
      fl = (adopt ? GPX_CP_ADOPT_ : 0) | (to != slot ? GPX_CP_MOVED_ : 0);
    }
    o_from[i] = from;
    o_to[i] = to;
    o_flags[i] = (uint8_t)fl;
    status[i] = (uint8_t)(ng ? GPX_S_NOGROUP : st ? GPX_S_STOPPED : GPX_S_OK);
  }
  const bool run = count > 0;
  const TileCount<4> c = tile_count(w_cnt, {adopt, ng, st, run});
  if (run) {
    const int32_t p = t0 + c.before[3];
    M.park_g[p] = g;
    M.park_first[p] = first;
    M.park_count[p] = count;
  }
  if (threadIdx.x == 0) M.tile[blockIdx.x] = mk4(c.total[0], c.total[1], c.total[2], c.total[3]);
}

/* one workgroup: tile[t].x = exclusive prefix of the tiles' run counts, *counts = the four sums */
__global__ __launch_bounds__(GPX_CP_TILE) void k_cp_offsets(int32_t ntiles, CpMem M, CpCounts* __restrict__ counts) {
  int32_t sum[4];
  tile_offsets<1, 3>(
      ntiles,
      [&](int32_t t, int32_t(&v)[4]) {
        const I4 w = M.tile[t];
        v[0] = w.w, v[1] = w.x, v[2] = w.y, v[3] = w.z;
      },
      [&](int32_t t, const int32_t(&off)[1], const int32_t(&)[4]) { M.tile[t].x = off[0]; }, sum);
  if (threadIdx.x == 0) *counts = CpCounts{sum[1], sum[2], sum[3], sum[0]};
}

__global__ __launch_bounds__(GPX_CP_TILE) void k_cp_move(CpMem M, int32_t* __restrict__ x_gidx,
                                                        int32_t* __restrict__ x_first, int32_t* __restrict__ x_count) {
  const I4 v = M.tile[blockIdx.x];
  const int32_t j = (int32_t)threadIdx.x; /* at most GPX_CP_TILE runs per tile: one lane each */
  if (j < v.w) {
    const int32_t p = (int32_t)blockIdx.x * GPX_CP_TILE + j, o = v.x + j;
    x_gidx[o] = M.park_g[p];
    x_first[o] = M.park_first[p];
    x_count[o] = M.park_count[p];
  }
}
