// Journal compaction (include/gpx_journal_gc.h): of the logged ACCEPTs a caller names by their index rows, the ones
// garbage collection still needs, copied out contiguously with their new index rows - compactLogfile's loop
// (SQLPaxosLogger.java:3347-3440) with LogIndex.isLogMsgNeeded (LogIndex.java:331-345) decided from the acceptors' GC
// slots in HBM.
//
// The four launches, the caps rule, the copy's rounds, the scratch invariant and the bounds argument: gpx_bytes.hip.h.
// What is this family's own:
//
//   k_jg_tile     one lane per row, GPX_JR_TILE = 256 per workgroup: the range test (every index and range BEFORE any
//                 byte of `in` could be read), then the length prefix, then the gather of g_flags / a_gc by e_gidx, then
//                 the verdict.  A kept row is a RUN HEAD unless row i - 1 of the same call is kept and ends exactly where
//                 row i starts; across a tile edge row i - 1 is evaluated again.  The tile's kept entries, their bytes,
//                 run heads, refused rows, unjudged rows and named bytes go to the per-tile words, unconditionally.
//   k_jg_offsets  a second scan (run heads, unjudged rows, named bytes), `unchanged` and the GPX_JG_SKIP_UNCHANGED rule;
//                 under the caps n_done, bytes_done and n_runs_done are exact.
//   k_jg_rows     the k_* rows, and ONE descriptor (output position, source position) PER RUN.  A run's length is the
//                 next descriptor's position, or bytes_done for the last: a run a cap cuts needs no length of its own.
//   k_jg_copy     copy_runs over runs, not entries: the source already holds the length prefixes, so inside a run the
//                 copy is a plain shifted copy - one aligned 16-byte store from at most two aligned 16-byte loads - with
//                 no prefix synthesis and no per-entry descriptor (a run is at least 4 bytes, which is all the rounds
//                 need).  Only a chunk that straddles a run boundary, and the last partial chunk of the call, take the
//                 narrow path.
//
// Cache policy: `in` and `out` are touched once by the copy and go through the stream_* helpers under GPX_NT_JOURNAL;
// the prefix test reads 4 bytes the copy reads again, the descriptors and per-tile words are hand-offs: plain.
//
// SCRATCH INVARIANT, beyond gpx_bytes.hip.h's: k_jg_offsets reads first_ok only when there is a tile 0; k_jg_copy reads
// descriptors [0, n_runs_done).
//
// Bounds, beyond gpx_bytes.hip.h's: a descriptor index is below n_runs_done <= n_done.  A source byte lies inside a range
// the range test accepted, inside the window [win_lo, win_hi) that `in` holds; every aligned word that is read holds at
// least one such byte, so nothing at or beyond in + round_up(win_hi - win_lo, 16) is read.
// Needs: gpx_bytes.hip.h, gpx_journal.hip.h (GPX_JR_TILE, GPX_JR_MAX_LEN).
#pragma once

#define GPX_JG_COUNT_ONLY_ 1     /* == GPX_JG_COUNT_ONLY of include/gpx_journal_gc.h (checked in gpx_journal_gc_dev.inc) */
#define GPX_JG_SKIP_UNCHANGED_ 2 /* == GPX_JG_SKIP_UNCHANGED */
#define GPX_JG_DROP_ 0
#define GPX_JG_KEEP_ 1
#define GPX_JG_KEEP_UNJUDGED_ 2
#define GPX_JG_BAD_ 3
#define GPX_JG_GF_EXISTS 1u /* == GF_EXISTS of gpx_kernels.hip.h (checked in gpx_journal_gc_dev.inc) */

struct JgCounts { /* == gpx_journal_gc_counts */
  int32_t n_usable, n_keep, n_done, n_bad, n_unjudged, n_runs_done, unchanged, reserved;
  long long keep_bytes, bytes_done, named_bytes, reserved2;
};

struct JgIn {
  const uint8_t* in;        /* device memory that holds bytes [win_lo, win_hi) of the caller's block, or NULL: no prefix test */
  long long win_lo, win_hi; /* the _dev form: [0, in_bytes); the host twin: the window it staged */
  long long in_base;
  const int32_t *e_gidx, *e_slot;
  const long long* e_off;
  const int32_t *e_len, *e_bnum, *e_bcoord, *cp_slot;
  const uint8_t* force;     /* the host twin's second pass: the verdicts of its first, nothing is judged again */
  const uint32_t* g_flags;  /* the two state columns, [max_groups] */
  const int32_t* a_gc;
  int32_t max_groups;
  int32_t n, row_base;      /* row i of this launch is row row_base + i of the caller's call (host twin: chunks) */
};

struct JgMem {
  int32_t *tile_cnt, *tile_heads, *tile_bad, *tile_unj, *tile_eoff, *tile_hoff; /* [tiles] */
  long long *tile_bytes, *tile_named, *tile_boff;                               /* [tiles] */
  long long *d_pos, *d_src; /* [max_batch] per done run: pos of its first byte; that byte's place in the window */
  int32_t* first_ok;        /* [1] row 0 is kept and starts at in_base */
};

struct JgOut {
  uint8_t* out;
  long long cap_bytes, out_base;
  int32_t cap_entries;
  int32_t *k_src, *k_gidx, *k_slot, *k_bnum, *k_bcoord;
  long long* k_off;
  int32_t* k_len;
};

struct JgRow {
  bool valid, keep; /* a row of the call; kept: an entry */
  uint8_t v;        /* GPX_JG_* */
  int32_t len;
  long long rel;    /* the prefix's place in the caller's block (relative to in_base); kept rows only */
};

/* Row i: the range, then the prefix, then the group, then the verdict. */
__device__ __forceinline__ JgRow jg_eval(const JgIn& I, long long i) {
  JgRow r{false, false, GPX_JG_DROP_, 0, 0};
  if (i >= I.n) return r;
  r.valid = true;
  if (I.force) { /* decided by the first pass: only kept rows are looked at, and only their range */
    r.v = I.force[i];
    if (r.v != GPX_JG_KEEP_ && r.v != GPX_JG_KEEP_UNJUDGED_) return r;
  }
  const uint8_t forced = r.v;
  r.v = GPX_JG_BAD_;
  const long long off = I.e_off[i], L = I.e_len[i];
  if (off < I.in_base) return r;
  const unsigned long long urel = (unsigned long long)off - (unsigned long long)I.in_base; /* the true difference */
  if (urel > (unsigned long long)I.win_hi) return r;
  const long long rel = (long long)urel;
  if (L < 0 || L > GPX_JR_MAX_LEN || rel < I.win_lo || rel > I.win_hi - (4 + L)) return r;
  if (I.in && !I.force && load4_unaligned<0>(I.in + (rel - I.win_lo)) != __builtin_bswap32((uint32_t)L)) return r;
  r.len = (int32_t)L;
  r.rel = rel;
  r.keep = true;
  if (I.force) {
    r.v = forced;
    return r;
  }
  const int32_t g = I.e_gidx[i];
  if ((uint32_t)g >= (uint32_t)I.max_groups || !(I.g_flags[g] & GPX_JG_GF_EXISTS)) {
    r.v = GPX_JG_KEEP_UNJUDGED_; /* never drop what cannot be judged */
    return r;
  }
  const uint32_t acc = (uint32_t)I.a_gc[g];
  uint32_t gc = acc;
  if (I.cp_slot) {
    const uint32_t cp = (uint32_t)I.cp_slot[i];
    if ((int32_t)(cp - acc) < 0) gc = cp; /* SQLPaxosLogger.java:1482 */
  }
  r.keep = (int32_t)((uint32_t)I.e_slot[i] - gc) > 0; /* LogIndex.java:333 */
  r.v = r.keep ? GPX_JG_KEEP_ : GPX_JG_DROP_;
  return r;
}

/* Is the kept row r = row i a run head?  Every lane of the workgroup calls it with the row of its lane; lane 0 has no
 * neighbour in the workgroup and evaluates row i - 1 again. */
__device__ __forceinline__ bool jg_head(const JgIn& I, long long i, const JgRow& r) {
  __shared__ long long s_end[GPX_JR_TILE]; /* where a kept row ends, -1 for any other */
  s_end[threadIdx.x] = r.keep ? r.rel + 4 + r.len : -1;
  __syncthreads();
  long long pe = -1;
  if (threadIdx.x > 0) {
    pe = s_end[threadIdx.x - 1];
  } else if (r.keep && i > 0) {
    const JgRow p = jg_eval(I, i - 1);
    if (p.keep) pe = p.rel + 4 + p.len;
  }
  __syncthreads(); /* the words are rewritten by the next call */
  return r.keep && pe != r.rel; /* rel >= 0 */
}

__global__ __launch_bounds__(GPX_BLOCK) void k_jg_tile(JgIn I, JgMem M, uint8_t* __restrict__ verdict) {
  const long long i = (long long)blockIdx.x * GPX_JR_TILE + (long long)threadIdx.x;
  const JgRow r = jg_eval(I, i);
  const bool head = jg_head(I, i, r);
  const bool bad = r.valid && r.v == GPX_JG_BAD_, usable = r.valid && !bad;
  if (verdict && r.valid) verdict[i] = r.v;
  const Scan64 S = block_scan64(r.keep, bad, r.keep ? 4ll + r.len : 0ll);
  const Scan64 H = block_scan64(head, r.valid && r.v == GPX_JG_KEEP_UNJUDGED_, usable ? 4ll + r.len : 0ll);
  if (threadIdx.x == 0) {
    M.tile_cnt[blockIdx.x] = S.tot_c;
    M.tile_bad[blockIdx.x] = S.tot_b;
    M.tile_bytes[blockIdx.x] = S.tot_v;
    M.tile_heads[blockIdx.x] = H.tot_c;
    M.tile_unj[blockIdx.x] = H.tot_b;
    M.tile_named[blockIdx.x] = H.tot_v;
    if (blockIdx.x == 0) *M.first_ok = r.keep && r.rel == 0;
  }
}

/* one workgroup: the tiles' bases, the counts, `unchanged`, and - where a cap cuts - the exact prefix that is done */
__global__ __launch_bounds__(GPX_BLOCK) void k_jg_offsets(int32_t ntiles, JgIn I, JgMem M, long long cap_bytes,
                                                         int32_t cap_entries, int32_t flags, long long in_bytes,
                                                         JgCounts* __restrict__ counts) {
  int32_t run_c = 0, run_h = 0, run_bad = 0, run_unj = 0, cut = INT32_MAX, cut_x[2] = {0, 0}; /* entries, heads */
  long long run_v = 0, run_named = 0, cut_b = 0;
  for (int32_t t0 = 0; t0 < ntiles; t0 += GPX_BLOCK) {
    const int32_t t = t0 + (int32_t)threadIdx.x;
    const bool live = t < ntiles;
    const int32_t c = live ? M.tile_cnt[t] : 0, b = live ? M.tile_bad[t] : 0;
    const int32_t hd = live ? M.tile_heads[t] : 0, u = live ? M.tile_unj[t] : 0;
    const long long v = live ? M.tile_bytes[t] : 0, nm = live ? M.tile_named[t] : 0;
    const Scan64 S = block_scan64(c, b, v);
    const Scan64 H = block_scan64(hd, u, nm);
    const int32_t eo = run_c + S.ex_c, ho = run_h + H.ex_c; /* <= n: fit */
    const long long bo = run_v + S.ex_v;
    if (live) {
      M.tile_eoff[t] = eo;
      M.tile_boff[t] = bo;
      M.tile_hoff[t] = ho;
      /* a lane's tiles come in ascending order */
      if (cut == INT32_MAX && caps_cut(c, v, eo, bo, cap_entries, cap_bytes)) cut = t, cut_x[0] = eo, cut_b = bo, cut_x[1] = ho;
    }
    run_c += S.tot_c, run_bad += S.tot_b, run_v += S.tot_v;
    run_h += H.tot_c, run_unj += H.tot_b, run_named += H.tot_v;
  }
  const int32_t first = caps_first_cut(cut, cut_b, cut_x);
  int32_t n_done = run_c, runs_done = run_h;
  long long bytes_done = run_v;
  if (first != INT32_MAX) { /* the same in every lane */
    const long long i = (long long)first * GPX_JR_TILE + (long long)threadIdx.x;
    const JgRow r = jg_eval(I, i);
    const bool head = jg_head(I, i, r);
    const long long v = r.keep ? 4ll + r.len : 0ll;
    const bool done = caps_done(r.keep, v, cut_x[0], cut_b, cap_entries, cap_bytes);
    const Scan64 D = block_scan64(done, done && head, done ? v : 0ll);
    n_done = cut_x[0] + D.tot_c;
    bytes_done = cut_b + D.tot_v;
    runs_done = cut_x[1] + D.tot_b;
  }
  /* every row kept and adjacent to its predecessor: one run (none for no rows) that starts at in_base and is the block */
  const bool unchanged = run_bad == 0 && run_c == I.n && run_h == (I.n > 0 ? 1 : 0) && (I.n == 0 || *M.first_ok) && run_v == in_bytes;
  if ((flags & GPX_JG_COUNT_ONLY_) || ((flags & GPX_JG_SKIP_UNCHANGED_) && unchanged)) n_done = 0, bytes_done = 0, runs_done = 0;
  if (threadIdx.x == 0)
    *counts = JgCounts{I.n - run_bad, run_c, n_done, run_bad, run_unj, runs_done, unchanged ? 1 : 0, 0, run_v, bytes_done, run_named, 0};
}

__global__ __launch_bounds__(GPX_BLOCK) void k_jg_rows(JgIn I, JgMem M, JgOut O, const JgCounts* __restrict__ counts) {
  const int32_t n_done = counts->n_done, e0 = M.tile_eoff[blockIdx.x];
  if (e0 >= n_done) return; /* the whole workgroup: nothing of this tile is done */
  const long long i = (long long)blockIdx.x * GPX_JR_TILE + (long long)threadIdx.x;
  const JgRow r = jg_eval(I, i);
  const bool head = jg_head(I, i, r);
  const Scan64 S = block_scan64(r.keep, 0, r.keep ? 4ll + r.len : 0ll);
  const Scan64 H = block_scan64(head, 0, 0ll);
  const int32_t e = e0 + S.ex_c;
  if (!r.keep || e >= n_done) return;
  const long long pos = M.tile_boff[blockIdx.x] + S.ex_v;
  if (O.k_src) O.k_src[e] = I.row_base + (int32_t)i;
  if (O.k_gidx) O.k_gidx[e] = I.e_gidx[i];
  if (O.k_slot) O.k_slot[e] = I.e_slot[i];
  if (O.k_bnum) O.k_bnum[e] = I.e_bnum[i];
  if (O.k_bcoord) O.k_bcoord[e] = I.e_bcoord[i];
  O.k_off[e] = O.out_base + pos;
  O.k_len[e] = r.len;
  if (head) { /* a done head: its run index is below n_runs_done */
    const int32_t q = M.tile_hoff[blockIdx.x] + H.ex_c;
    M.d_pos[q] = pos;
    M.d_src[q] = r.rel - I.win_lo;
  }
}

struct JgTile { /* LDS: one round of run descriptors */
  long long pos[GPX_JR_SPAN], src[GPX_JR_SPAN];
};

/* word dw .. of five consecutive ones out of eight, without an indexed register array */
__device__ __forceinline__ uint32_t jg_pick(int32_t dw, int32_t a, int32_t b, int32_t c, int32_t d) {
  return (uint32_t)(dw == 0 ? a : dw == 1 ? b : dw == 2 ? c : d);
}

struct JgCopy { /* copy_runs' family: one descriptor per done run */
  typedef JgTile Tile;
  const uint8_t* in;
  const JgMem& M;
  __device__ __forceinline__ void stage(JgTile& T, int32_t e, int32_t s) const { T.src[s] = M.d_src[e]; }
  __device__ __forceinline__ void chunk(const JgTile& T, long long P, long long Pe, int32_t k, int32_t ns,
                                        uint32_t (&w)[4]) const {
    if (Pe == P + 16 && (k + 1 >= ns || T.pos[k + 1] >= Pe)) {
      /* the chunk lies inside run k: sixteen source bytes from the one or two aligned words that hold them */
      const long long s = T.src[k] + (P - T.pos[k]);
      const int32_t sh = (int32_t)(s & 15), dw = sh >> 2;
      const uint32_t b = (uint32_t)(sh & 3);
      const I4* q = (const I4*)(in + (s - sh));
      const I4 A = stream_load16<GPX_NT_JOURNAL>(q);
      I4 B = mk4(0, 0, 0, 0);
      if (sh) B = stream_load16<GPX_NT_JOURNAL>(q + 1); /* holds byte s + 15 */
      const uint32_t y0 = jg_pick(dw, A.x, A.y, A.z, A.w), y1 = jg_pick(dw, A.y, A.z, A.w, B.x);
      const uint32_t y2 = jg_pick(dw, A.z, A.w, B.x, B.y), y3 = jg_pick(dw, A.w, B.x, B.y, B.z);
      const uint32_t y4 = jg_pick(dw, B.x, B.y, B.z, B.w);
      w[0] = __builtin_amdgcn_alignbyte(y1, y0, b), w[1] = __builtin_amdgcn_alignbyte(y2, y1, b);
      w[2] = __builtin_amdgcn_alignbyte(y3, y2, b), w[3] = __builtin_amdgcn_alignbyte(y4, y3, b);
      return;
    }
    /* a run boundary inside the chunk, or the last chunk of the call: dword by dword, byte by byte at a boundary */
#pragma unroll
    for (int32_t d = 0; d < 4; d++) {
      const long long Q = P + 4 * d;
      w[d] = 0u;
      if (Q >= Pe) continue;
      while (k + 1 < ns && T.pos[k + 1] <= Q) k++;
      if (Q + 4 <= Pe && (k + 1 >= ns || T.pos[k + 1] >= Q + 4)) {
        w[d] = load4_unaligned<GPX_NT_JOURNAL>(in + T.src[k] + (Q - T.pos[k]));
      } else {
        for (int32_t c = 0; c < 4 && Q + c < Pe; c++) {
          while (k + 1 < ns && T.pos[k + 1] <= Q + c) k++;
          w[d] |= (uint32_t)in[T.src[k] + (Q + c - T.pos[k])] << (8 * c);
        }
      }
    }
  }
};

__global__ __launch_bounds__(GPX_BLOCK) void k_jg_copy(const uint8_t* __restrict__ in, JgMem M, uint8_t* __restrict__ out,
                                                      const JgCounts* __restrict__ counts) {
  copy_runs(JgCopy{in, M}, M.d_pos, counts->n_runs_done, out, counts->bytes_done);
}

