// View change in list form (include/gpx_viewchange.h): the pvalues a PREPARE is answered with and the proposals a
// completed election hands back, as compacted lists instead of `window` dense planes.
//
// The three launches, the scratch invariant and the bounds argument: gpx_compact.hip.h.  What is this family's own:
//
// Acceptor side (k_pl_*).  k_bucket_prepare<false> (gpx_kernels.hip.h) has left p_mask[i] of every record in the
// engine's scratch: 8 bytes per record, no planes.  An entry is a RECORD, its weight popcount(mask).
//   k_pl_tile      the tile's entries and its dropped / NACK / to-log records.
//   k_pl_offsets   the exclusive prefix of the entries, the sums, and the cut: the leading records whose lists end at or
//                  before cap_entries (ends ascend with the record index, so they are a prefix).
//   k_pl_move      pv_off of the complete records, and their lists gathered straight from acc_ring (the call does not
//                  change acc_ring and the stream orders the passes) in ascending SIGNED slot: the rank of a pvalue is
//                  the number of the record's other pvalues with a smaller slot.  Two nested walks over the bits of the
//                  mask: no per-lane array.
//
// Coordinator side (k_vl_*).  gpx_prepare_reply_batch_dev has run into the engine's scratch exactly as a caller would
// run it.  An entry is a record; a HIT (status != GPX_S_OK, or ELECTED / PREEMPTED) is parked with its clamped count and
// the entries of the tile's hits before it.
//   k_vl_tile      parks the hits; the tile's hits, entries and class counts.
//   k_vl_offsets   the exclusive prefixes of hits and entries, the sums; then for the hits from `from_hit` on the entry
//                  the output begins at and the cut: hit H fits iff H < from_hit + cap_hits and its list ends at or
//                  before cap_entries.  Both bounds ascend with H, so the hits that fit are a prefix; the one tile the
//                  cut falls into is settled here, by this one workgroup.
//   k_vl_move      the hit rows, then the entries COALESCED: lanes walk the tile's output entries and find (hit, j) by a
//                  binary search over the tile's prefixes in LDS - most records have no entries and a few have `window`.
// k_vl_offsets + k_vl_move are all a continuation (gpx_prepare_reply_lists_more) runs: the parked hits, the dense
// scratch and the per-tile words stay as the first call left them.
#pragma once

#define GPX_VCL_TILE_ 256 /* == GPX_VCL_TILE of include/gpx_viewchange.h (checked in gpx_vclists_dev.inc) */
static_assert(GPX_VCL_TILE_ == GPX_BLOCK, "one lane per record of a tile");

struct PlCounts { /* == gpx_pl_counts */
  int32_t n_entries, recs_done, entries_done, n_dropped, n_nack, n_tolog, reserved[2];
};
struct PrlCounts { /* == gpx_prl_counts */
  int32_t n_hits, n_entries, from_hit, hits_done, entries_done, n_elected, n_preempted, n_dropped;
};

/* acceptor scratch: the masks of the largest batch, the per-tile words, the cut for the move pass */
struct PlMem {
  unsigned long long* mask;                                       /* [max_batch in whole tiles] */
  int32_t *t_ent, *t_drop, *t_nack, *t_tolog, *t_off;             /* [tiles] */
  int32_t* cut;                                                   /* recs_done, entries_done */
};

/* coordinator scratch: the dense call's outputs, the parked hits, the per-tile words, the span for the move pass */
struct PrlMem {
  uint8_t *v_kind, *status; /* dense, [max_batch in whole tiles] */
  int32_t *e_count, *e_median;
  int32_t* e_slot; /* planes: [window][n], n the call's */
  uint8_t *e_kind, *e_flags;
  int64_t* e_handle;
  int32_t *p_rec, *p_gidx, *p_pre, *p_cnt;                        /* parked hits, tile * TILE + rank */
  int32_t *t_hits, *t_ent, *t_el, *t_pre, *t_drop, *t_hoff, *t_eoff; /* [tiles] */
  int32_t* ctl;                                                   /* from_hit, end hit, first entry: absolute */
};

struct PrlOut {
  int32_t *h_rec, *h_gidx;
  uint8_t *h_kind, *h_status;
  int32_t *h_median, *h_off, *h_count;
  int32_t* e_slot;
  uint8_t* e_kind;
  int64_t* e_handle;
  uint8_t* e_flags;
};

/* ---- acceptor side ---- */

__global__ __launch_bounds__(GPX_BLOCK) void k_pl_tile(int32_t n, const uint8_t* __restrict__ r_flags,
                                                      const uint8_t* __restrict__ status, PlMem M) {
  __shared__ int32_t w_cnt[3][GPX_COMPACT_WAVES];
  const int64_t i = (int64_t)blockIdx.x * GPX_VCL_TILE_ + (int32_t)threadIdx.x;
  int32_t w = 0;
  bool drop = false, nack = false, tolog = false;
  if (i < n) {
    w = __popcll(M.mask[i]);
    const uint8_t f = r_flags[i];
    drop = status[i] != GPX_S_OK;
    nack = (f & GPX_P_NACK) != 0;
    tolog = (f & GPX_P_TOLOG) != 0;
  }
  const TileCount<3> c = tile_count(w_cnt, {drop, nack, tolog});
  int32_t ent = 0;
  block_exscan(w, &ent);
  if (threadIdx.x == 0) {
    M.t_ent[blockIdx.x] = ent;
    M.t_drop[blockIdx.x] = c.total[0];
    M.t_nack[blockIdx.x] = c.total[1];
    M.t_tolog[blockIdx.x] = c.total[2];
  }
}

/* one workgroup */
__global__ __launch_bounds__(GPX_BLOCK) void k_pl_offsets(int32_t n, int32_t ntiles, int32_t cap, PlMem M,
                                                         int32_t* __restrict__ pv_off, PlCounts* __restrict__ counts) {
  __shared__ int32_t s_cut;
  int32_t sum[4];
  tile_offsets<1, 3>(
      ntiles,
      [&](int32_t t, int32_t(&v)[4]) { v[0] = M.t_ent[t], v[1] = M.t_drop[t], v[2] = M.t_nack[t], v[3] = M.t_tolog[t]; },
      [&](int32_t t, const int32_t(&off)[1], const int32_t(&)[4]) { M.t_off[t] = off[0]; }, sum);
  if (threadIdx.x == 0) s_cut = ntiles;
  __syncthreads();
  /* the first tile whose entries do not all end at or before cap: ends ascend with t */
  for (int32_t t = (int32_t)threadIdx.x; t < ntiles; t += GPX_BLOCK)
    if ((int64_t)M.t_off[t] + M.t_ent[t] > cap) atomicMin(&s_cut, t);
  __syncthreads();
  const int32_t c = s_cut; /* the same in every lane */
  int32_t recs = n, ents = sum[0];
  if (c < ntiles) {
    const int64_t i = (int64_t)c * GPX_VCL_TILE_ + (int32_t)threadIdx.x;
    const int32_t w = i < n ? __popcll(M.mask[i]) : 0, off = M.t_off[c];
    int32_t tot = 0, nf = 0, ef = 0;
    const int32_t pre = block_exscan(w, &tot);
    const bool fits = i < n && (int64_t)off + pre + w <= cap; /* a prefix of the tile's records */
    block_exscan(fits ? 1 : 0, &nf);
    block_exscan(fits ? w : 0, &ef);
    recs = c * GPX_VCL_TILE_ + nf;
    ents = off + ef;
  }
  if (threadIdx.x == 0) {
    *counts = PlCounts{sum[0], recs, ents, sum[1], sum[2], sum[3], {0, 0}};
    M.cut[0] = recs;
    M.cut[1] = ents;
    if (n == 0 && pv_off) pv_off[0] = 0;
  }
}

__global__ __launch_bounds__(GPX_BLOCK) void k_pl_move(DevState S, int32_t n, const int32_t* __restrict__ gidx, PlMem M,
                                                      int32_t* __restrict__ pv_off, int32_t* __restrict__ pv_slot,
                                                      int32_t* __restrict__ pv_bnum, int32_t* __restrict__ pv_bcoord) {
  const int32_t recs = M.cut[0];
  const int32_t t0 = (int32_t)blockIdx.x * GPX_VCL_TILE_;
  if (t0 > recs) return; /* the whole workgroup: record `recs` still gets its pv_off */
  const int64_t i = (int64_t)t0 + (int32_t)threadIdx.x;
  unsigned long long m = i < n ? M.mask[i] : 0ull;
  if (S.W < 64) m &= (1ull << S.W) - 1ull;
  const int32_t w = __popcll(m);
  int32_t tot = 0;
  const int32_t o = M.t_off[blockIdx.x] + block_exscan(w, &tot);
  if (i >= n) return;
  if (pv_off) {
    if (i <= recs) pv_off[i] = o;
    if (i == n - 1 && recs == n) pv_off[n] = o + w;
  }
  if (i >= recs || !m || !pv_slot) return;
  const int32_t g = gidx[i];
  if ((uint32_t)g >= (uint32_t)S.G) return; /* (a record of no group has an empty mask) */
  for (unsigned long long a = m; a; a &= a - 1) {
    const I4 v = S.acc_ring[(int64_t)(__ffsll((long long)a) - 1) * S.G + g];
    int32_t rank = 0; /* TreeMap<Integer, ...> order: signed compare, as for_signed_order */
    for (unsigned long long b = m; b; b &= b - 1)
      rank += S.acc_ring[(int64_t)(__ffsll((long long)b) - 1) * S.G + g].x < v.x ? 1 : 0;
    pv_slot[o + rank] = v.x;
    pv_bnum[o + rank] = v.y;
    pv_bcoord[o + rank] = v.z;
  }
}

/* ---- coordinator side ---- */

__global__ __launch_bounds__(GPX_BLOCK) void k_vl_tile(int32_t n, int32_t W, const int32_t* __restrict__ gidx, PrlMem M) {
  __shared__ int32_t w_cnt[4][GPX_COMPACT_WAVES];
  const int32_t t0 = (int32_t)blockIdx.x * GPX_VCL_TILE_;
  const int64_t i = (int64_t)t0 + (int32_t)threadIdx.x;
  bool el = false, pr = false, dr = false;
  int32_t cnt = 0;
  if (i < n) {
    const uint8_t vk = M.v_kind[i];
    el = vk == GPX_V_ELECTED;
    pr = vk == GPX_V_PREEMPTED;
    dr = M.status[i] != GPX_S_OK;
    if (el || pr || dr) cnt = min(max(M.e_count[i], 0), W); /* clamped before it indexes anything */
  }
  const bool hit = el || pr || dr;
  const TileCount<4> c = tile_count(w_cnt, {hit, el, pr, dr});
  int32_t ent = 0;
  const int32_t pre = block_exscan(cnt, &ent);
  if (hit) {
    const int32_t p = t0 + c.before[0];
    M.p_rec[p] = (int32_t)i;
    M.p_gidx[p] = gidx[i];
    M.p_pre[p] = pre;
    M.p_cnt[p] = cnt;
  }
  if (threadIdx.x == 0) {
    M.t_hits[blockIdx.x] = c.total[0];
    M.t_ent[blockIdx.x] = ent;
    M.t_el[blockIdx.x] = c.total[1];
    M.t_pre[blockIdx.x] = c.total[2];
    M.t_drop[blockIdx.x] = c.total[3];
  }
}

/* one workgroup */
__global__ __launch_bounds__(GPX_BLOCK) void k_vl_offsets(int32_t ntiles, int32_t from_hit, int32_t cap_hits,
                                                         int32_t cap_entries, PrlMem M, PrlCounts* __restrict__ counts) {
  __shared__ int32_t s_eb, s_cut, s_emax;
  int32_t sum[5];
  tile_offsets<2, 3>(
      ntiles,
      [&](int32_t t, int32_t(&v)[5]) {
        v[0] = M.t_hits[t], v[1] = M.t_ent[t], v[2] = M.t_el[t], v[3] = M.t_pre[t], v[4] = M.t_drop[t];
      },
      [&](int32_t t, const int32_t(&off)[2], const int32_t(&)[5]) { M.t_hoff[t] = off[0], M.t_eoff[t] = off[1]; }, sum);
  if (threadIdx.x == 0) {
    s_eb = sum[1]; /* from_hit at or past the last hit: nothing left */
    s_cut = ntiles;
    s_emax = 0;
  }
  __syncthreads();
  /* the entry hit `from_hit` begins at: one tile holds it */
  for (int32_t t = (int32_t)threadIdx.x; t < ntiles; t += GPX_BLOCK) {
    const int32_t ho = M.t_hoff[t], h = M.t_hits[t];
    if (from_hit >= ho && from_hit - ho < h) s_eb = M.t_eoff[t] + M.p_pre[t * GPX_VCL_TILE_ + (from_hit - ho)];
  }
  __syncthreads();
  const int32_t eb = s_eb;
  const int64_t lim_h = (int64_t)from_hit + cap_hits, lim_e = (int64_t)eb + cap_entries;
  /* the first tile whose hits do not all fit */
  for (int32_t t = (int32_t)threadIdx.x; t < ntiles; t += GPX_BLOCK) {
    const int32_t h = M.t_hits[t];
    if (h > 0 && !((int64_t)M.t_hoff[t] + h <= lim_h && (int64_t)M.t_eoff[t] + M.t_ent[t] <= lim_e)) atomicMin(&s_cut, t);
  }
  __syncthreads();
  const int32_t c = s_cut; /* the same in every lane */
  int32_t end_hit = sum[0], end_ent = sum[1];
  if (c < ntiles) {
    const int32_t h = M.t_hits[c], ho = M.t_hoff[c], eo = M.t_eoff[c], j = (int32_t)threadIdx.x;
    bool fit = false;
    int32_t e1 = 0;
    if (j < h) {
      e1 = eo + M.p_pre[c * GPX_VCL_TILE_ + j] + M.p_cnt[c * GPX_VCL_TILE_ + j];
      fit = (int64_t)ho + j < lim_h && (int64_t)e1 <= lim_e; /* a prefix of the tile's hits */
    }
    int32_t nf = 0;
    block_exscan(fit ? 1 : 0, &nf);
    if (fit) atomicMax(&s_emax, e1);
    __syncthreads();
    end_hit = ho + nf;
    end_ent = max(s_emax, eo);
  }
  const int32_t hits_done = end_hit > from_hit ? end_hit - from_hit : 0;
  if (threadIdx.x == 0) {
    *counts = PrlCounts{sum[0], sum[1], from_hit, hits_done, hits_done ? end_ent - eb : 0, sum[2], sum[3], sum[4]};
    M.ctl[0] = from_hit;
    M.ctl[1] = from_hit + hits_done;
    M.ctl[2] = eb;
  }
}

__global__ __launch_bounds__(GPX_BLOCK) void k_vl_move(int32_t n, int32_t bias, PrlMem M, PrlOut O) {
  __shared__ int32_t s_pre[GPX_VCL_TILE_], s_rec[GPX_VCL_TILE_], s_cnt[GPX_VCL_TILE_];
  const int32_t from = M.ctl[0], end = M.ctl[1], eb = M.ctl[2];
  const int32_t h = M.t_hits[blockIdx.x], ho = M.t_hoff[blockIdx.x], eo = M.t_eoff[blockIdx.x];
  const int32_t j0 = min(max(from - ho, 0), h), j1 = min(max(end - ho, 0), h);
  if (j0 >= j1) return; /* the whole workgroup */
  const int32_t j = (int32_t)threadIdx.x, p = (int32_t)blockIdx.x * GPX_VCL_TILE_ + j;
  int32_t rec = 0, pre = 0, cnt = 0;
  if (j < h) {
    rec = M.p_rec[p];
    pre = M.p_pre[p];
    cnt = M.p_cnt[p];
    s_rec[j] = rec;
    s_pre[j] = pre;
    s_cnt[j] = cnt;
  }
  __syncthreads();
  if (j >= j0 && j < j1) {
    const int32_t q = ho + j - from;
    O.h_rec[q] = rec;
    O.h_gidx[q] = M.p_gidx[p];
    O.h_kind[q] = M.v_kind[rec];
    O.h_status[q] = M.status[rec];
    O.h_median[q] = M.e_median[rec];
    O.h_off[q] = eo + pre - eb + bias;
    O.h_count[q] = cnt;
  }
  const int32_t x0 = s_pre[j0], x1 = j1 < h ? s_pre[j1] : M.t_ent[blockIdx.x];
  for (int32_t x = x0 + j; x < x1; x += GPX_BLOCK) {
    int32_t lo = j0, hi = j1 - 1; /* the last hit whose entries begin at or before x: the one that holds x */
    while (lo < hi) {
      const int32_t mid = (lo + hi + 1) >> 1;
      if (s_pre[mid] <= x) lo = mid;
      else hi = mid - 1;
    }
    const int32_t k = x - s_pre[lo];
    if (k >= s_cnt[lo]) continue;
    const int64_t src = (int64_t)k * n + s_rec[lo];
    const int32_t dst = eo + x - eb;
    O.e_slot[dst] = M.e_slot[src];
    O.e_kind[dst] = M.e_kind[src];
    O.e_handle[dst] = M.e_handle[src];
    O.e_flags[dst] = M.e_flags[src];
  }
}
