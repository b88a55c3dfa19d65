// Table scans that return only their hits (include/gpx_scan.h): election, poke and gap scan with the
// hits compacted on the device in entry order, the count left in device memory.
//
// A call is three launches on one stream, and no workgroup ever waits for another one:
//
//   k_scan_*_tile    one workgroup per GPX_SCAN_TILE consecutive entries, consecutive lanes on consecutive
//                    entries (the state columns stay coalesced dword streams, as in the dense kernels).  Every
//                    entry is evaluated ONCE, by the same per-group function the dense kernel calls
//                    (election_scan_row / poke_scan_row / gap_scan_row).  A hit's rank inside the tile comes from
//                    the wave's ballot (mbcnt below the lane), a per-wave prefix in LDS and the hits of the
//                    tile's earlier passes; its row is parked at scratch[tile base + rank].  The tile's hit and
//                    no-group counts go to tile_hits[tile] / tile_nog[tile].
//   k_scan_offsets   ONE workgroup: exclusive prefix of tile_hits into tile_off, the sums into *counts.
//   k_scan_*_move    one workgroup per tile: parked row j of tile t goes to output entry tile_off[t] + j while
//                    that is below cap.  Only hits move; nothing is evaluated twice.
//
// The order between the steps is the stream's.  There are no look-back words, no arrival counters and no
// assumption about residency, so this path adds nothing to the epochs of DESIGN.md 3.3 and nothing that can
// starve on a shared device.
//
// SCRATCH INVARIANT: every scratch word a call reads is one the SAME call wrote.  k_scan_offsets reads
// tile_hits / tile_nog [0, ntiles): each written (unconditionally) by its tile's workgroup.  k_scan_*_move reads
// tile_hits[t], tile_off[t] (written by k_scan_offsets for every t < ntiles) and parked rows j < tile_hits[t] of
// tile t: exactly the rows that tile's workgroup wrote.  Nothing is cleared between calls and nothing needs to be.
//
// Bounds: a parked row sits at tile * GPX_SCAN_TILE + rank with rank < GPX_SCAN_TILE, and the scratch columns
// hold max(max_groups, max_batch) entries rounded up to whole tiles; the host refuses a larger n.
#pragma once

#define GPX_SCAN_TILE_ 1024 /* == GPX_SCAN_TILE of include/gpx_scan.h (checked in gpx_scan_dev.inc) */
#define GPX_SCAN_WAVES (GPX_BLOCK / 64)

struct ScanCounts { /* == gpx_scan_counts */
  int32_t n_hits, n_nogroup, reserved[2];
};

/* The scratch block: six int32 columns, two byte columns of `cap` entries each (cap: whole tiles), then three arrays
 * of `tl` bytes for the per-tile words.  Kernels get the base and the two sizes and form a column's address where they
 * use it (a pointer per column would sit in scalar registers next to the state's, which the evaluation needs).
 * Columns 4 and 5 are adjacent and 8-byte aligned: the gap scan keeps its 64-bit masks there. */
struct ScanScratch {
  char* base;
  uint32_t cap, tl;
  __device__ __forceinline__ int32_t* i32(int q) const { return (int32_t*)(base + (size_t)q * 4 * cap); }
  __device__ __forceinline__ unsigned long long* u64() const { return (unsigned long long*)i32(4); }
  __device__ __forceinline__ uint8_t* u8(int q) const { return (uint8_t*)(base + (size_t)(24 + q) * cap); }
  __device__ __forceinline__ int32_t* tile(int q) const { return (int32_t*)(base + (size_t)26 * cap + (size_t)q * tl); }
  __device__ __forceinline__ int32_t* tile_hits() const { return tile(0); }
  __device__ __forceinline__ int32_t* tile_nog() const { return tile(1); }
  __device__ __forceinline__ int32_t* tile_off() const { return tile(2); }
};

/* the callers' compact columns, by type (null where a scan has none; all null when cap == 0) */
struct ScanOut {
  int32_t* i32[6];
  uint8_t* u8[2];
  unsigned long long* u64;
};

/* ---- the three scans: evaluate, test, park, move ---- */
struct ScanElection {
  typedef ElectionRow Row;
  NodeLists L;
  int32_t force;
  __device__ __forceinline__ Row eval(const DevState& S, int32_t g) const { return election_scan_row(S, g, L, force); }
  __device__ __forceinline__ bool nogroup(const Row& r) const { return r.status == GPX_S_NOGROUP; }
  __device__ __forceinline__ bool hit(const Row& r) const { return r.status == GPX_S_OK && r.run != GPX_RUN_NO; }
  __device__ __forceinline__ void park(const ScanScratch& X, int32_t p, int32_t g, const Row& r) const {
    X.i32(0)[p] = g;
    X.u8(0)[p] = (uint8_t)r.run;
    X.i32(1)[p] = r.p_bnum;
    X.i32(2)[p] = r.p_first;
  }
  static __device__ __forceinline__ void move(const ScanScratch& X, int32_t p, const ScanOut& O, int32_t o) {
    O.i32[0][o] = X.i32(0)[p];
    O.u8[0][o] = X.u8(0)[p];
    O.i32[1][o] = X.i32(1)[p];
    O.i32[2][o] = X.i32(2)[p];
  }
};

template <int KMAX>
struct ScanPoke {
  typedef PokeRow Row;
  __device__ __forceinline__ Row eval(const DevState& S, int32_t g) const { return poke_scan_row<KMAX>(S, g); }
  __device__ __forceinline__ bool nogroup(const Row& r) const { return r.status == GPX_S_NOGROUP; }
  __device__ __forceinline__ bool hit(const Row& r) const { return r.status == GPX_S_OK && r.poke != GPX_POKE_NONE; }
  __device__ __forceinline__ void park(const ScanScratch& X, int32_t p, int32_t g, const Row& r) const {
    X.i32(0)[p] = g;
    X.u8(0)[p] = r.poke;
    X.i32(1)[p] = r.slot;
    X.i32(2)[p] = r.bnum;
    X.i32(3)[p] = r.bcoord;
    X.i32(4)[p] = r.median_cp;
    X.u8(1)[p] = r.flags;
    X.i32(5)[p] = (int32_t)r.heard;
  }
  static __device__ __forceinline__ void move(const ScanScratch& X, int32_t p, const ScanOut& O, int32_t o) {
    O.i32[0][o] = X.i32(0)[p];
    O.u8[0][o] = X.u8(0)[p];
    O.i32[1][o] = X.i32(1)[p];
    O.i32[2][o] = X.i32(2)[p];
    O.i32[3][o] = X.i32(3)[p];
    O.i32[4][o] = X.i32(4)[p];
    O.u8[1][o] = X.u8(1)[p];
    O.i32[5][o] = X.i32(5)[p];
  }
};

struct ScanGap {
  typedef GapRow Row;
  int32_t threshold, sync_mode, size_limit, require;
  __device__ __forceinline__ Row eval(const DevState& S, int32_t g) const {
    return gap_scan_row(S, g, threshold, sync_mode, size_limit);
  }
  __device__ __forceinline__ bool nogroup(const Row& r) const { return r.status == GPX_S_NOGROUP; }
  __device__ __forceinline__ bool hit(const Row& r) const {
    if (r.status != GPX_S_OK) return false; /* a stopped group is never a hit */
    if ((require & GPX_GAP_HIT_SYNC) && !r.should_sync) return false;
    if ((require & GPX_GAP_HIT_MISSING) && !r.missing) return false;
    if ((require & GPX_GAP_HIT_AHEAD) && jsub(r.max_committed, r.first_slot) < 0) return false;
    return true;
  }
  __device__ __forceinline__ void park(const ScanScratch& X, int32_t p, int32_t g, const Row& r) const {
    X.i32(0)[p] = g;
    X.i32(1)[p] = r.first_slot;
    X.i32(2)[p] = r.max_committed;
    X.u64()[p] = r.missing;
    X.u8(0)[p] = (uint8_t)r.should_sync;
  }
  static __device__ __forceinline__ void move(const ScanScratch& X, int32_t p, const ScanOut& O, int32_t o) {
    O.i32[0][o] = X.i32(0)[p];
    O.i32[1][o] = X.i32(1)[p];
    O.i32[2][o] = X.i32(2)[p];
    O.u64[o] = X.u64()[p];
    O.u8[0][o] = X.u8(0)[p];
  }
};

/* lanes of this wave below the caller's whose bit is set in m */
__device__ __forceinline__ int32_t scan_rank_below(unsigned long long m) {
  return (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

template <class E>
__global__ __launch_bounds__(GPX_BLOCK) void k_scan_tile(DevState S, int32_t n, const int32_t* __restrict__ gidx,
                                                        E ev, ScanScratch X) {
  __shared__ int32_t w_hits[2][GPX_SCAN_WAVES], w_nog[2][GPX_SCAN_WAVES];
  const int32_t t0 = (int32_t)blockIdx.x * GPX_SCAN_TILE_; /* n <= 2^31 - 1: the last tile's base fits */
  const int32_t wave = (int32_t)threadIdx.x >> 6;
  int32_t base = 0, nog = 0; /* the tile's hits / no-group entries of the passes so far: the same in every lane */
#pragma unroll 1 /* one copy of the evaluation: unrolled, the state pointers of four copies spill scalar registers */
  for (int32_t pass = 0; pass < GPX_SCAN_TILE_ / GPX_BLOCK; pass++) {
    const int64_t i = (int64_t)t0 + pass * GPX_BLOCK + (int32_t)threadIdx.x;
    bool hit = false, ng = false;
    int32_t g = 0;
    typename E::Row r{};
    if (i < n) {
      g = gidx ? gidx[i] : (int32_t)i;
      r = ev.eval(S, g);
      hit = ev.hit(r);
      ng = ev.nogroup(r);
    }
    const unsigned long long mh = __ballot(hit), mn = __ballot(ng);
    /* two sets of LDS words, used alternately: one barrier per pass */
    if ((threadIdx.x & 63) == 0) {
      w_hits[pass & 1][wave] = __popcll(mh);
      w_nog[pass & 1][wave] = __popcll(mn);
    }
    __syncthreads();
    int32_t before = 0, total = 0;
#pragma unroll
    for (int32_t q = 0; q < GPX_SCAN_WAVES; q++) {
      const int32_t c = w_hits[pass & 1][q];
      before += q < wave ? c : 0;
      total += c;
      nog += w_nog[pass & 1][q];
    }
    if (hit) ev.park(X, t0 + base + before + scan_rank_below(mh), g, r);
    base += total;
  }
  if (threadIdx.x == 0) {
    X.tile_hits()[blockIdx.x] = base;
    X.tile_nog()[blockIdx.x] = nog;
  }
}

/* one workgroup: tile_off = exclusive prefix of tile_hits, *counts = the sums */
__global__ __launch_bounds__(GPX_BLOCK) void k_scan_offsets(int32_t ntiles, ScanScratch X, ScanCounts* __restrict__ counts) {
  __shared__ int32_t w_sum[GPX_SCAN_WAVES], w_nog[GPX_SCAN_WAVES];
  const int32_t lane = (int32_t)threadIdx.x & 63, wave = (int32_t)threadIdx.x >> 6;
  int32_t running = 0, nog = 0;
  for (int32_t t0 = 0; t0 < ntiles; t0 += GPX_BLOCK) {
    const int32_t t = t0 + (int32_t)threadIdx.x;
    const int32_t c = t < ntiles ? X.tile_hits()[t] : 0;
    int32_t ng = t < ntiles ? X.tile_nog()[t] : 0;
    int32_t inc = c; /* inclusive prefix within the wave */
#pragma unroll
    for (int32_t d = 1; d < 64; d <<= 1) {
      const int32_t v = __shfl_up(inc, d);
      const int32_t u = __shfl_xor(ng, d);
      if (lane >= d) inc += v;
      ng += u; /* butterfly: every lane ends with the wave's sum */
    }
    if (lane == 63) {
      w_sum[wave] = inc;
      w_nog[wave] = ng;
    }
    __syncthreads();
    int32_t before = 0, total = 0;
#pragma unroll
    for (int32_t q = 0; q < GPX_SCAN_WAVES; q++) {
      before += q < wave ? w_sum[q] : 0;
      total += w_sum[q];
      nog += w_nog[q];
    }
    if (t < ntiles) X.tile_off()[t] = running + before + inc - c;
    running += total;
    __syncthreads(); /* w_sum is rewritten by the next round */
  }
  if (threadIdx.x == 0) *counts = ScanCounts{running, nog, {0, 0}};
}

template <class E>
__global__ __launch_bounds__(GPX_BLOCK) void k_scan_move(ScanScratch X, ScanOut O, int32_t cap) {
  const int32_t c = X.tile_hits()[blockIdx.x], off = X.tile_off()[blockIdx.x];
  const int32_t lim = min(c, cap - off); /* off <= n_hits <= 2^31 - 1, cap >= 0: no overflow */
  const int32_t p0 = (int32_t)blockIdx.x * GPX_SCAN_TILE_;
  for (int32_t j = (int32_t)threadIdx.x; j < lim; j += GPX_BLOCK) E::move(X, p0 + j, O, off + j);
}

/* gpx_election_begin for the first min(counts->n_hits, cap) entries: k_election_begin's effect entry for entry */
__global__ __launch_bounds__(GPX_BLOCK) void k_scan_election_begin(DevState S, int32_t cap,
                                                                  const ScanCounts* __restrict__ counts,
                                                                  const int32_t* __restrict__ gidx,
                                                                  const int32_t* __restrict__ bnum,
                                                                  uint8_t* __restrict__ e_status) {
  const int32_t n = min(max(counts->n_hits, 0), cap);
  const int32_t i = blockIdx.x * GPX_BLOCK + threadIdx.x;
  if (i >= n) return;
  e_status[i] = election_begin_group(S, gidx[i], bnum[i]);
}
