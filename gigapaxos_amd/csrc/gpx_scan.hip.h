// Table scans that return only their hits (include/gpx_scan.h): election, poke and gap scan with the
// hits compacted on the device in entry order, the count left in device memory.
//
// The three launches, the scratch invariant and the bounds argument: gpx_compact.hip.h.  What is the scans' own:
//
//   k_scan_*_tile    GPX_SCAN_TILE entries in passes of GPX_BLOCK; the state columns stay coalesced dword streams, as in
//                    the dense kernels.  An entry is evaluated by the same per-group function the dense kernel calls
//                    (election_scan_row / poke_scan_row / gap_scan_row); a hit's row is parked.  The tile's hit and
//                    no-group counts go to tile_hits[tile] / tile_nog[tile].
//   k_scan_offsets   tile_off = exclusive prefix of tile_hits, the two sums into *counts.
//   k_scan_*_move    copies the parked row.
#pragma once

#define GPX_SCAN_TILE_ 1024 /* == GPX_SCAN_TILE of include/gpx_scan.h (checked in gpx_scan_dev.inc) */

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

template <class E>
__global__ __launch_bounds__(GPX_BLOCK) void k_scan_tile(DevState S, int32_t n, const int32_t* __restrict__ gidx,
                                                        E ev, ScanScratch X) {
  __shared__ int32_t w_cnt[2][2][GPX_COMPACT_WAVES]; /* two sets, used alternately: one barrier per pass */
  const int32_t t0 = (int32_t)blockIdx.x * GPX_SCAN_TILE_; /* n <= 2^31 - 1: the last tile's base fits */
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
    const TileCount<2> c = tile_count(w_cnt[pass & 1], {hit, ng});
    if (hit) ev.park(X, t0 + base + c.before[0], g, r);
    base += c.total[0];
    nog += c.total[1];
  }
  if (threadIdx.x == 0) {
    X.tile_hits()[blockIdx.x] = base;
    X.tile_nog()[blockIdx.x] = nog;
  }
}

/* one workgroup: tile_off = exclusive prefix of tile_hits, *counts = the sums */
__global__ __launch_bounds__(GPX_BLOCK) void k_scan_offsets(int32_t ntiles, ScanScratch X, ScanCounts* __restrict__ counts) {
  int32_t sum[2];
  tile_offsets<1, 1>(
      ntiles, [&](int32_t t, int32_t(&v)[2]) { v[0] = X.tile_hits()[t], v[1] = X.tile_nog()[t]; },
      [&](int32_t t, const int32_t(&off)[1], const int32_t(&)[2]) { X.tile_off()[t] = off[0]; }, sum);
  if (threadIdx.x == 0) *counts = ScanCounts{sum[0], sum[1], {0, 0}};
}

template <class E>
__global__ __launch_bounds__(GPX_BLOCK) void k_scan_move(ScanScratch X, ScanOut O, int32_t cap) {
  const MoveSpan m = move_span<GPX_SCAN_TILE_>(X.tile_hits(), X.tile_off(), cap);
  for (int32_t j = (int32_t)threadIdx.x; j < m.lim; j += GPX_BLOCK) E::move(X, m.p0 + j, O, m.off + j);
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
