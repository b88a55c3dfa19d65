// The log index on the device (include/gpx_logindex.h): the reference's per-group LogIndex (paxosutil/LogIndex.java) as
// ONE flat table of rows in append order, keyed by gidx, with the per-group GC slot and min file beside it.
//
// Built on gpx_compact.hip.h: add, lookup, file_rows and compact are its three launches (tile, offsets, move) with a tile
// of GPX_BLOCK entries, one lane per entry, so a tile is ONE pass.  What is this family's own:
//
//   The tail.  hdr[LI_ROWS] lives in device memory: add's offsets kernel reads it, keeps it in hdr[LI_BASE] for the move
//     and moves it on, so add after add needs no host.  The host only keeps an UPPER BOUND of it (the sum of the n of
//     every add since open, at most cap_rows; the exact tail after a host twin) and sizes the row scans' grids by that:
//     a workgroup whose tile starts at or past the tail writes its per-tile word (0) and ends.
//   Arming.  set_gc and lookup find a row's record through arm[g].  k_li_arm claims each group for the LOWEST record
//     that names it with an atomic min; k_li_mark then calls a record first (arm[g] == i) or GPX_LI_REPEAT; the row scan
//     reads arm of its row's group - ONE random 4-byte read per alive row, the only gather of the scan - and the call's
//     last launch over the records clears exactly the words the call set (the first records' own), so between calls
//     every arming word is idle.  No epoch, look-back word, arrival counter or assumption about residency.
//   Min file under set_gc.  The scan takes an atomic min of the row index of each surviving row into first[g], the
//     arming word's companion; k_li_gc_finish reads that row's file and sets the companion idle again.
//   files.  An LDS histogram of n_files <= 4096 bins per workgroup, over a grid-stride loop of tiles, flushed with one
//     global atomic per non-zero bin.
//
// SCRATCH INVARIANT (gpx_compact.hip.h): park, the per-tile words and hdr[LI_BASE], hdr[LI_MINF] are scratch, and every
// such word a call reads is one the same call wrote.  The table, gc, min_file, arm, first and hdr[LI_ROWS..LI_GEN] are
// engine state, initialised by open.
//
// Bounds.  A group number indexes gc / min_file / arm / first only after it has been checked against M.G; a table row's
// gidx was checked by the add that wrote it.  A row index indexes the table only after it has been checked against the
// tail, and the tail is at most cap_rows: add's move writes rows [base, base + min(addable, cap_rows - base)).  A parked
// entry sits at tile * 256 + rank with rank < 256; park holds whole tiles of max(cap_rows, max_batch) entries.  An
// arming word other than idle is a record index of the running call (< n); a companion other than idle is a row below
// the tail.  Nothing here is an array indexed by a run-time value: no kernel has scratch memory.
// Needs: gpx_compact.hip.h.
#pragma once

#define GPX_LI_TILE GPX_BLOCK
#define GPX_LI_IDLE 0xffffffffu
#define GPX_LI_ADDED_ 0 /* == GPX_LI_* of include/gpx_logindex.h (checked in gpx_logindex_dev.inc) */
#define GPX_LI_STALE_ 1
#define GPX_LI_NOGROUP_ 2
#define GPX_LI_FULL_ 3
#define GPX_LI_REPEAT_ 4
#define GPX_LI_RESET_ 1
#define GPX_LI_MAX_FILES_ 4096
#define GPX_LI_HIST_GRID 1024 /* workgroups of a files histogram, at most */

enum { LI_ROWS = 0, LI_ALIVE = 1, LI_GEN = 2, LI_BASE = 3, LI_MINF = 4, LI_HDR_WORDS = 8 };

struct LiCounts { /* == gpx_logindex_counts */
  int32_t n_rows, n_alive, generation, n_done, n_hits, n_stale, n_nogroup, n_repeat;
};

struct LiCols { /* one block of the table's columns, [cap_rows] */
  int32_t *gidx, *slot, *bnum, *bcoord, *file;
  long long* off;
  int32_t* len;
  uint8_t* alive;
};

struct LiMem {
  LiCols T, U;                /* the table and the block compact moves it into */
  int32_t *gc, *min_file;     /* [G] the GC slot, the min file: -1 at open */
  uint32_t *arm, *first;      /* [G] the arming word and its companion: GPX_LI_IDLE between calls */
  int32_t* hdr;               /* [LI_HDR_WORDS] the tail, the alive rows, the generation; scratch: LI_BASE, LI_MINF */
  int32_t* park;              /* [whole tiles of max(cap_rows, max_batch)] */
  int32_t *tile_cnt, *tile_off; /* [tiles of max(cap_rows, max_batch, max_groups)] */
  int32_t *rt_a, *rt_b, *rt_c;  /* [tiles of max_batch] the record launches' counts */
  int32_t cap_rows, G;
};

/* the records a call with n_dev takes */
__device__ __forceinline__ int32_t li_taken(int32_t n, const int32_t* n_dev) {
  return n_dev ? min(n, max(*n_dev, 0)) : n;
}
/* (int32)(a - b), the reference's wrapping comparison */
__device__ __forceinline__ int32_t li_diff(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }

/* ---- add ---- */

__global__ __launch_bounds__(GPX_BLOCK) void k_li_add_tile(LiMem M, int32_t n, const int32_t* __restrict__ n_dev,
                                                          const int32_t* __restrict__ e_gidx,
                                                          const int32_t* __restrict__ e_slot,
                                                          uint8_t* __restrict__ status) {
  __shared__ int32_t w_cnt[3][GPX_COMPACT_WAVES];
  const int32_t m = li_taken(n, n_dev);
  const int32_t i = (int32_t)blockIdx.x * GPX_LI_TILE + (int32_t)threadIdx.x; /* the grid covers n <= max_batch */
  bool add = false, stale = false, nog = false;
  if (i < m) {
    const int32_t g = e_gidx[i];
    if ((uint32_t)g >= (uint32_t)M.G) nog = true;
    else if (li_diff(e_slot[i], M.gc[g]) <= 0) stale = true; /* LogIndex.java:193 */
    else add = true;
    if (status && !add) status[i] = nog ? GPX_LI_NOGROUP_ : GPX_LI_STALE_;
  }
  const TileCount<3> c = tile_count(w_cnt, {add, stale, nog});
  if (add) M.park[(int32_t)blockIdx.x * GPX_LI_TILE + c.before[0]] = i;
  if (threadIdx.x == 0) {
    M.tile_cnt[blockIdx.x] = c.total[0];
    M.rt_a[blockIdx.x] = c.total[1];
    M.rt_b[blockIdx.x] = c.total[2];
  }
}

__global__ __launch_bounds__(GPX_BLOCK) void k_li_add_offsets(int32_t ntiles, LiMem M, LiCounts* __restrict__ counts) {
  int32_t sum[3];
  tile_offsets<1, 2>(
      ntiles, [&](int32_t t, int32_t(&v)[3]) { v[0] = M.tile_cnt[t], v[1] = M.rt_a[t], v[2] = M.rt_b[t]; },
      [&](int32_t t, const int32_t(&off)[1], const int32_t(&)[3]) { M.tile_off[t] = off[0]; }, sum);
  if (threadIdx.x == 0) {
    const int32_t tail = M.hdr[LI_ROWS], done = min(sum[0], M.cap_rows - tail), alive = M.hdr[LI_ALIVE] + done;
    M.hdr[LI_BASE] = tail;
    M.hdr[LI_ROWS] = tail + done;
    M.hdr[LI_ALIVE] = alive;
    *counts = LiCounts{tail + done, alive, M.hdr[LI_GEN], done, 0, sum[1], sum[2], 0};
  }
}

struct LiRowsIn { /* the pack's row columns */
  const int32_t *gidx, *slot, *bnum, *bcoord;
  const long long* off;
  const int32_t* len;
};

__global__ __launch_bounds__(GPX_BLOCK) void k_li_add_move(LiMem M, LiRowsIn I, int32_t file, uint8_t* __restrict__ status) {
  const int32_t base = M.hdr[LI_BASE]; /* the tail before this call */
  const MoveSpan m = move_span<GPX_LI_TILE>(M.tile_cnt, M.tile_off, M.cap_rows - base);
  const int32_t j = (int32_t)threadIdx.x;
  if (j >= M.tile_cnt[blockIdx.x]) return;
  const int32_t i = M.park[m.p0 + j];
  if (j >= m.lim) { /* no room: nothing changes */
    if (status) status[i] = GPX_LI_FULL_;
    return;
  }
  const int32_t r = base + m.off + j, g = I.gidx[i]; /* r < cap_rows; g was checked by k_li_add_tile */
  M.T.gidx[r] = g;
  M.T.slot[r] = I.slot[i];
  M.T.bnum[r] = I.bnum[i];
  M.T.bcoord[r] = I.bcoord[i];
  M.T.file[r] = file;
  M.T.off[r] = I.off[i];
  M.T.len[r] = I.len[i];
  M.T.alive[r] = 1;
  if (M.min_file[g] == -1) atomicCAS(&M.min_file[g], -1, file); /* every record of the call carries the same file */
  if (status) status[i] = GPX_LI_ADDED_;
}

/* ---- arming (set_gc, lookup) ---- */

__global__ __launch_bounds__(GPX_BLOCK) void k_li_arm(LiMem M, int32_t n, const int32_t* __restrict__ gidx) {
  const int32_t i = (int32_t)blockIdx.x * GPX_LI_TILE + (int32_t)threadIdx.x;
  if (i >= n) return;
  const int32_t g = gidx[i];
  if ((uint32_t)g < (uint32_t)M.G) atomicMin(&M.arm[g], (uint32_t)i);
}

/* first or repeat; set_gc (GC): a first record stores its group's GC slot */
template <bool GC>
__global__ __launch_bounds__(GPX_BLOCK) void k_li_mark(LiMem M, int32_t n, const int32_t* __restrict__ gidx,
                                                      const int32_t* __restrict__ gc_slot, int32_t flags,
                                                      uint8_t* __restrict__ status) {
  __shared__ int32_t w_cnt[3][GPX_COMPACT_WAVES];
  const int32_t i = (int32_t)blockIdx.x * GPX_LI_TILE + (int32_t)threadIdx.x;
  bool first = false, rep = false, nog = false;
  if (i < n) {
    const int32_t g = gidx[i];
    if ((uint32_t)g >= (uint32_t)M.G) nog = true;
    else if (M.arm[g] == (uint32_t)i) first = true;
    else rep = true;
    if constexpr (GC) {
      if (first) M.gc[g] = (flags & GPX_LI_RESET_) ? -1 : gc_slot[i]; /* LogIndex.java:129: unconditionally */
    }
    if (status) status[i] = nog ? GPX_LI_NOGROUP_ : rep ? GPX_LI_REPEAT_ : GPX_LI_ADDED_;
  }
  const TileCount<3> c = tile_count(w_cnt, {first, rep, nog});
  if (threadIdx.x == 0) {
    M.rt_a[blockIdx.x] = c.total[0];
    M.rt_b[blockIdx.x] = c.total[1];
    M.rt_c[blockIdx.x] = c.total[2];
  }
}

/* clears exactly the arming words this call set: each by the record that holds it */
__global__ __launch_bounds__(GPX_BLOCK) void k_li_disarm(LiMem M, int32_t n, const int32_t* __restrict__ gidx) {
  const int32_t i = (int32_t)blockIdx.x * GPX_LI_TILE + (int32_t)threadIdx.x;
  if (i >= n) return;
  const int32_t g = gidx[i];
  if ((uint32_t)g < (uint32_t)M.G && M.arm[g] == (uint32_t)i) M.arm[g] = GPX_LI_IDLE;
}

/* ---- set_gc ---- */

__global__ __launch_bounds__(GPX_BLOCK) void k_li_gc_scan(LiMem M, int32_t flags) {
  __shared__ int32_t w_cnt[1][GPX_COMPACT_WAVES];
  const int32_t n_rows = M.hdr[LI_ROWS], t0 = (int32_t)blockIdx.x * GPX_LI_TILE;
  if (t0 >= n_rows) { /* the whole workgroup: a tile past the tail */
    if (threadIdx.x == 0) M.tile_cnt[blockIdx.x] = 0;
    return;
  }
  const int32_t r = t0 + (int32_t)threadIdx.x;
  bool die = false;
  if (r < n_rows && M.T.alive[r]) {
    const int32_t g = M.T.gidx[r];
    if (M.arm[g] != GPX_LI_IDLE) { /* k_li_mark stored the group's new GC slot */
      die = (flags & GPX_LI_RESET_) || li_diff(M.T.slot[r], M.gc[g]) <= 0; /* LogIndex.java:136-146 */
      if (die) M.T.alive[r] = 0;
      else atomicMin(&M.first[g], (uint32_t)r);
    }
  }
  const TileCount<1> c = tile_count(w_cnt, {die});
  if (threadIdx.x == 0) M.tile_cnt[blockIdx.x] = c.total[0];
}

/* the min file of every group a first record names, from the companion; then companion and arming word are idle again */
__global__ __launch_bounds__(GPX_BLOCK) void k_li_gc_finish(LiMem M, int32_t n, const int32_t* __restrict__ gidx) {
  const int32_t i = (int32_t)blockIdx.x * GPX_LI_TILE + (int32_t)threadIdx.x;
  if (i >= n) return;
  const int32_t g = gidx[i];
  if ((uint32_t)g >= (uint32_t)M.G || M.arm[g] != (uint32_t)i) return;
  const uint32_t f = M.first[g];
  M.min_file[g] = f == GPX_LI_IDLE ? -1 : M.T.file[f]; /* f: a row below the tail (k_li_gc_scan) */
  if (f != GPX_LI_IDLE) M.first[g] = GPX_LI_IDLE;
  M.arm[g] = GPX_LI_IDLE;
}

/* the sums of the record launch's three per-tile words */
__device__ __forceinline__ void li_rec_sums(int32_t rec_tiles, const LiMem& M, bool three, int32_t (&sum)[3]) {
  tile_offsets<1, 2>(
      rec_tiles,
      [&](int32_t t, int32_t(&v)[3]) { v[0] = M.rt_a[t], v[1] = M.rt_b[t], v[2] = three ? M.rt_c[t] : 0; },
      [&](int32_t, const int32_t(&)[1], const int32_t(&)[3]) {}, sum);
}

__global__ __launch_bounds__(GPX_BLOCK) void k_li_gc_sum(int32_t rec_tiles, int32_t row_tiles, LiMem M,
                                                        LiCounts* __restrict__ counts) {
  int32_t rec[3], died[1];
  li_rec_sums(rec_tiles, M, true, rec);
  tile_offsets<1, 0>(
      row_tiles, [&](int32_t t, int32_t(&v)[1]) { v[0] = M.tile_cnt[t]; },
      [&](int32_t, const int32_t(&)[1], const int32_t(&)[1]) {}, died);
  if (threadIdx.x == 0) {
    const int32_t alive = M.hdr[LI_ALIVE] - died[0];
    M.hdr[LI_ALIVE] = alive;
    *counts = LiCounts{M.hdr[LI_ROWS], alive, M.hdr[LI_GEN], rec[0], 0, died[0], rec[2], rec[1]};
  }
}

/* ---- the row scans that park their hits: lookup, file_rows, compact ---- */

enum { LI_SCAN_LOOKUP = 0, LI_SCAN_FILE = 1, LI_SCAN_ALIVE = 2 };

struct LiQuery { /* lookup's record columns */
  const int32_t *min_slot, *max_slot;
  const uint8_t* has_max;
};

template <int KIND>
__global__ __launch_bounds__(GPX_BLOCK) void k_li_scan(LiMem M, LiQuery Q, int32_t file) {
  __shared__ int32_t w_cnt[1][GPX_COMPACT_WAVES];
  const int32_t n_rows = M.hdr[LI_ROWS], t0 = (int32_t)blockIdx.x * GPX_LI_TILE;
  if (t0 >= n_rows) {
    if (threadIdx.x == 0) M.tile_cnt[blockIdx.x] = 0;
    return;
  }
  const int32_t r = t0 + (int32_t)threadIdx.x;
  bool hit = false;
  if (r < n_rows && M.T.alive[r]) {
    if constexpr (KIND == LI_SCAN_ALIVE) {
      hit = true;
    } else if constexpr (KIND == LI_SCAN_FILE) {
      hit = M.T.file[r] == file;
    } else {
      const uint32_t a = M.arm[M.T.gidx[r]]; /* the record that asks for this row's group: < n, or idle */
      if (a != GPX_LI_IDLE) {
        const int32_t s = M.T.slot[r];
        hit = li_diff(s, Q.min_slot[a]) >= 0 && (!(Q.has_max && Q.has_max[a]) || li_diff(s, Q.max_slot[a]) <= 0);
      }
    }
  }
  const TileCount<1> c = tile_count(w_cnt, {hit});
  if (hit) M.park[t0 + c.before[0]] = r;
  if (threadIdx.x == 0) M.tile_cnt[blockIdx.x] = c.total[0];
}

/* one workgroup: where each tile's hits go, and the counts; compact also moves the tail and the generation */
template <int KIND>
__global__ __launch_bounds__(GPX_BLOCK) void k_li_scan_offsets(int32_t rec_tiles, int32_t row_tiles, LiMem M, int32_t cap,
                                                              LiCounts* __restrict__ counts) {
  int32_t rec[3] = {0, 0, 0}, hits[1];
  if constexpr (KIND == LI_SCAN_LOOKUP) li_rec_sums(rec_tiles, M, true, rec);
  tile_offsets<1, 0>(
      row_tiles, [&](int32_t t, int32_t(&v)[1]) { v[0] = M.tile_cnt[t]; },
      [&](int32_t t, const int32_t(&off)[1], const int32_t(&)[1]) { M.tile_off[t] = off[0]; }, hits);
  if (threadIdx.x != 0) return;
  if constexpr (KIND == LI_SCAN_ALIVE) {
    const int32_t gen = (int32_t)((uint32_t)M.hdr[LI_GEN] + 1u);
    M.hdr[LI_ROWS] = hits[0];
    M.hdr[LI_ALIVE] = hits[0];
    M.hdr[LI_GEN] = gen;
    *counts = LiCounts{hits[0], hits[0], gen, hits[0], 0, 0, 0, 0};
  } else {
    *counts = LiCounts{M.hdr[LI_ROWS], M.hdr[LI_ALIVE], M.hdr[LI_GEN], min(hits[0], cap), hits[0], 0, rec[2], rec[1]};
  }
}

struct LiOut { /* lookup: rec, row and the entry; file_rows: row, the six row columns and gc */
  int32_t *rec, *row, *gidx, *slot, *bnum, *bcoord, *file;
  long long* off;
  int32_t *len, *gc;
};

template <int KIND>
__global__ __launch_bounds__(GPX_BLOCK) void k_li_scan_move(LiMem M, int32_t cap, LiOut O) {
  const MoveSpan m = move_span<GPX_LI_TILE>(M.tile_cnt, M.tile_off, cap);
  const int32_t j = (int32_t)threadIdx.x;
  if (j >= m.lim) return;
  const int32_t r = M.park[m.p0 + j], o = m.off + j; /* r: an alive row below the tail; o < min(hits, cap) */
  const int32_t g = M.T.gidx[r];
  if constexpr (KIND == LI_SCAN_ALIVE) { /* into the other block: o <= r < cap_rows */
    M.U.gidx[o] = g;
    M.U.slot[o] = M.T.slot[r];
    M.U.bnum[o] = M.T.bnum[r];
    M.U.bcoord[o] = M.T.bcoord[r];
    M.U.file[o] = M.T.file[r];
    M.U.off[o] = M.T.off[r];
    M.U.len[o] = M.T.len[r];
    M.U.alive[o] = 1;
  } else {
    O.row[o] = r;
    O.slot[o] = M.T.slot[r];
    O.bnum[o] = M.T.bnum[r];
    O.bcoord[o] = M.T.bcoord[r];
    O.off[o] = M.T.off[r];
    O.len[o] = M.T.len[r];
    if constexpr (KIND == LI_SCAN_LOOKUP) {
      O.rec[o] = (int32_t)M.arm[g]; /* still armed: k_li_disarm comes last */
      O.file[o] = M.T.file[r];
    } else {
      O.gidx[o] = g;
      O.gc[o] = M.gc[g];
    }
  }
}

/* ---- relocate ---- */

__global__ __launch_bounds__(GPX_BLOCK) void k_li_reloc(LiMem M, int32_t n, const int32_t* __restrict__ n_dev,
                                                       int32_t generation, const int32_t* __restrict__ o_row,
                                                       const int32_t* __restrict__ k_src, int32_t new_file,
                                                       const long long* __restrict__ k_off,
                                                       const int32_t* __restrict__ k_len) {
  __shared__ int32_t w_cnt[2][GPX_COMPACT_WAVES];
  const int32_t m = li_taken(n, n_dev);
  const int32_t j = (int32_t)blockIdx.x * GPX_LI_TILE + (int32_t)threadIdx.x;
  bool ok = false;
  if (j < m && generation == M.hdr[LI_GEN]) {
    const int32_t src = k_src ? k_src[j] : j;
    if ((uint32_t)src < (uint32_t)n) { /* o_row holds n entries */
      const int32_t r = o_row[src];
      if ((uint32_t)r < (uint32_t)M.hdr[LI_ROWS] && M.T.alive[r]) {
        M.T.file[r] = new_file;
        M.T.off[r] = k_off[j];
        M.T.len[r] = k_len[j];
        ok = true;
      }
    }
  }
  const TileCount<2> c = tile_count(w_cnt, {ok, j < m && !ok});
  if (threadIdx.x == 0) {
    M.rt_a[blockIdx.x] = c.total[0];
    M.rt_b[blockIdx.x] = c.total[1];
  }
}

__global__ __launch_bounds__(GPX_BLOCK) void k_li_reloc_sum(int32_t rec_tiles, LiMem M, LiCounts* __restrict__ counts) {
  int32_t rec[3];
  li_rec_sums(rec_tiles, M, false, rec);
  if (threadIdx.x == 0) *counts = LiCounts{M.hdr[LI_ROWS], M.hdr[LI_ALIVE], M.hdr[LI_GEN], rec[0], 0, rec[1], 0, 0};
}

/* ---- files ---- */

__global__ __launch_bounds__(GPX_BLOCK) void k_li_files_init(LiMem M, int32_t n_files, int32_t* __restrict__ o_rows,
                                                            int32_t* __restrict__ o_groups) {
  const int32_t f = (int32_t)blockIdx.x * GPX_BLOCK + (int32_t)threadIdx.x;
  if (f < n_files) {
    if (o_rows) o_rows[f] = 0;
    if (o_groups) o_groups[f] = 0;
  }
  if (f == 0) M.hdr[LI_MINF] = INT32_MAX;
}

/* GROUPS: over the min files of all groups (and their minimum); otherwise over the files of the alive rows.  The
 * workgroup's count of ids outside the range goes to its word of `outside`, unconditionally. */
template <bool GROUPS>
__global__ __launch_bounds__(GPX_BLOCK) void k_li_files_hist(LiMem M, int32_t file_base, int32_t n_files,
                                                            int32_t* __restrict__ out, int32_t* __restrict__ outside) {
  __shared__ int32_t s_bin[GPX_LI_MAX_FILES_], s_out, s_min;
  for (int32_t b = (int32_t)threadIdx.x; b < n_files; b += GPX_BLOCK) s_bin[b] = 0;
  if (threadIdx.x == 0) s_out = 0, s_min = INT32_MAX;
  __syncthreads();
  const long long total = GROUPS ? M.G : M.hdr[LI_ROWS];
  int32_t lo = INT32_MAX, nout = 0;
  for (long long i = (long long)blockIdx.x * GPX_BLOCK + (long long)threadIdx.x; i < total;
       i += (long long)gridDim.x * GPX_BLOCK) {
    int32_t f;
    if constexpr (GROUPS) {
      f = M.min_file[i];
      if (f == -1) continue;
      lo = min(lo, f);
    } else {
      if (!M.T.alive[i]) continue;
      f = M.T.file[i];
    }
    const long long d = (long long)f - (long long)file_base;
    if (d >= 0 && d < n_files) atomicAdd(&s_bin[d], 1);
    else nout++;
  }
  if (nout) atomicAdd(&s_out, nout);
  if (GROUPS && lo != INT32_MAX) atomicMin(&s_min, lo);
  __syncthreads();
  if (out)
    for (int32_t b = (int32_t)threadIdx.x; b < n_files; b += GPX_BLOCK) {
      const int32_t v = s_bin[b];
      if (v) atomicAdd(&out[b], v);
    }
  if (threadIdx.x == 0) {
    outside[blockIdx.x] = s_out;
    if (GROUPS && s_min != INT32_MAX) atomicMin(&M.hdr[LI_MINF], s_min);
  }
}

__global__ __launch_bounds__(GPX_BLOCK) void k_li_files_sum(int32_t row_wgs, int32_t grp_wgs, LiMem M,
                                                           int32_t* __restrict__ o_min_file,
                                                           LiCounts* __restrict__ counts) {
  int32_t a[1], b[1];
  tile_offsets<1, 0>(
      row_wgs, [&](int32_t t, int32_t(&v)[1]) { v[0] = M.tile_cnt[t]; },
      [&](int32_t, const int32_t(&)[1], const int32_t(&)[1]) {}, a);
  tile_offsets<1, 0>(
      grp_wgs, [&](int32_t t, int32_t(&v)[1]) { v[0] = M.tile_off[t]; },
      [&](int32_t, const int32_t(&)[1], const int32_t(&)[1]) {}, b);
  if (threadIdx.x == 0) {
    const int32_t lo = M.hdr[LI_MINF];
    if (o_min_file) *o_min_file = lo == INT32_MAX ? -1 : lo;
    *counts = LiCounts{M.hdr[LI_ROWS], M.hdr[LI_ALIVE], M.hdr[LI_GEN], 0, 0, a[0] + b[0], 0, 0};
  }
}
