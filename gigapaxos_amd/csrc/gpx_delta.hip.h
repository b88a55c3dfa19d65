// Delta images (include/gpx_delta.h): export the groups whose state differs from their mark, apply such a delta.
//
// EXPORT is the three launches of the image export (gpx_image.hip.h) with one more thing per entry, the signature:
//   k_delta_tile     one workgroup per GPX_IMAGE_TILE entries, one lane per entry.  The lane reads its group's columns
//                    the way sweep_eval and the image's column side do - coalesced dwords, a ring entry whole as one
//                    16-byte load, c_wait / co_ring / the handles only for a group that is running for coordinator - and
//                    feeds the CANONICAL words, in row order, into two hash streams that live in two registers
//                    (delta_sig: the rules of image_put_main / image_put_cont RESTATED - a change to either must be made
//                    in both by hand.  tests/delta_emulation.cpp does not compare the two word streams; it flips one
//                    state word per group for every word of both rows and expects that group reported, and rewrites
//                    words the state does not define and expects none).
//                    A changed entry parks (group | GPX_IMAGE_PREP, signature) at its rank inside the tile, a gone one its group at its own rank; tile_live / tile_chg / tile_rows /
//                    tile_gone are written unconditionally.  NO MARK AND NO STATE CHANGES HERE: what fits is not known.
//   k_delta_offsets  ONE workgroup: exclusive prefixes of tile_rows, tile_chg and tile_gone, the counts, and where
//                    `cap` cuts a tile the exact n_done / n_rows_done from that tile's parked entries.
//   k_delta_move     one workgroup per tile.  Gone entries below cap_gone go to o_gone and their marks to 0.  The rows
//                    of the changed entries that fit are built through LDS by the image export's own functions
//                    (image_put_main / image_put_cont / image_lds_flush: byte for byte gpx_group_export's rows); then
//                    the lane stores the mark of its group - the parked signature, or 0 under GPX_DELTA_EVICT, where it
//                    also retires the group, after it has read the last word of it.
// APPLY is the import's two launches with the replace rule (image_rows_body<., true>) and k_delta_gone.
//
// SCRATCH INVARIANT (gpx_compact.hip.h): beyond the per-tile words k_delta_offsets reads parked entries below tile_chg of
// the cut tile; k_delta_move reads parked entries below tile_chg / tile_gone of its tile.  The marks are not scratch:
// engine state, zeroed when allocated, touched by k_delta_tile (read) and k_delta_move (write) alone.
//
// Bounds.  A parked entry sits at tile * GPX_IMAGE_TILE + rank, rank < GPX_IMAGE_TILE; the host refuses n above the
// entries the parked columns hold.  A group number indexes state or marks only after it has been compared with S.G
// (a parked group passed that test).  An output row index r satisfies r + weight <= cap, a gone index is below
// cap_gone.  Distinct entries are a precondition, as for the image export: two entries naming one group would race on
// its mark.
#pragma once

struct DeltaCounts { /* == gpx_delta_counts */
  int32_t n_live, n_changed, n_rows, n_done, n_rows_done, n_gone, n_gone_done, reserved;
};
struct DeltaMem {
  unsigned long long* marks;    /* [G] engine state: 0 = never written, else the signature at the last written export */
  int32_t* park;                /* [whole tiles] changed: group | GPX_IMAGE_PREP */
  unsigned long long* park_sig; /* [whole tiles] ... and its signature */
  int32_t* park_gone;           /* [whole tiles] gone: group */
  int32_t *tile_live, *tile_chg, *tile_rows, *tile_gone; /* [tiles] counts */
  int32_t *tile_off, *tile_goff, *tile_xoff;             /* [tiles] exclusive prefixes of rows, changed, gone */
};
#define GPX_DELTA_EVICT_ 1 /* == GPX_DELTA_EVICT / GPX_DELTA_FULL of include/gpx_delta.h (checked in gpx_delta_dev.inc) */
#define GPX_DELTA_FULL_ 2

/* The two streams: the block step of MurmurHash3 x86_32, and the same shape with other multipliers, rotations and
 * seed, so that a collision of one says nothing about the other. */
struct DeltaHash {
  uint32_t a, b;
};
__device__ __forceinline__ void delta_mix(DeltaHash& h, uint32_t v) {
  uint32_t p = v * 0xcc9e2d51u;
  p = (p << 15) | (p >> 17);
  p *= 0x1b873593u;
  h.a ^= p;
  h.a = (h.a << 13) | (h.a >> 19);
  h.a = h.a * 5u + 0xe6546b64u;
  uint32_t q = v * 0x85ebca77u;
  q = (q << 13) | (q >> 19);
  q *= 0xc2b2ae3du;
  h.b ^= q;
  h.b = (h.b << 17) | (h.b >> 15);
  h.b = h.b * 5u + 0x165667b1u;
}
__device__ __forceinline__ uint32_t delta_fin(uint32_t h, uint32_t m1, uint32_t m2) {
  h ^= h >> 16;
  h *= m1;
  h ^= h >> 13;
  h *= m2;
  return h ^ (h >> 16);
}

/* The signature of live group g: every word of its row(s) before padding, in row order, as image_put_main and
 * image_put_cont would write them (include/gpx_image.h, "Canonical").  No array: the words go from the loads into the
 * two streams; the present bits the later sections depend on travel in 64-bit masks (window <= 64). */
__device__ __forceinline__ unsigned long long delta_sig(const DevState& S, int32_t g, uint32_t gf, bool prep) {
  const int64_t G = S.G;
  const bool hc = (gf & GF_HASCOORD) != 0;
  const int32_t k = min((int32_t)GF_K(gf), S.kmax);
  DeltaHash h{0x9747b28cu, 0x27d4eb2fu};
  auto mix = [&](int32_t v) { delta_mix(h, (uint32_t)v); };
  mix(GPX_IMAGE_FORMAT);
  mix(GPX_IMAGE_MAIN);
  mix((int32_t)(GPX_IMG_F_EXISTS | ((gf & GF_STOPPED) ? GPX_IMG_F_STOPPED : 0) | (hc ? GPX_IMG_F_HASCOORD : 0) |
                (prep ? GPX_IMG_F_PREPARING | GPX_IMG_F_CONTINUED : 0) | (GF_K(gf) << GPX_IMG_F_K_SHIFT)));
  mix(S.my_id);
  mix(S.kmax | (S.W << 16));
  mix(g);
  mix(S.g_version[g]);
  mix(S.a_slot[g]);
  mix(S.a_bnum[g]);
  mix(S.a_bcoord[g]);
  mix(S.a_gc[g]);
  mix(hc ? S.c_bnum[g] : 0);
  mix(hc ? S.c_bcoord[g] : 0);
  mix(hc ? S.c_next[g] : 0);
  mix(hc ? S.c_pcount[g] : 0);
  mix(0);
  for (int32_t j = 0; j < S.kmax; j++) mix(j < k ? S.members[(int64_t)j * G + g] : 0);
  for (int32_t j = 0; j < S.kmax; j++) mix(hc && j < k ? S.node_slots[(int64_t)j * G + g] : 0);
  unsigned long long p_present = 0ull, com_present = 0ull, co_present = 0ull;
#pragma unroll 4
  for (int32_t x = 0; x < S.W; x++) {
    const uint32_t e = (hc || prep) ? S.p_ring[(int64_t)x * G + g] : 0u;
    if (e & PR_PRESENT) p_present |= 1ull << x;
    mix(hc && (e & PR_PRESENT) ? (int32_t)(e & (0xffffu | PR_PRESENT | PR_STOP)) : 0);
  }
#pragma unroll 4
  for (int32_t x = 0; x < S.W; x++) {
    const I4 v = S.acc_ring[(int64_t)x * G + g];
    const uint32_t af = (uint32_t)v.w & AF_MASK, cf = ((uint32_t)v.w >> CF_SHIFT) & 0xffu;
    const bool ap = (af & RF_PRESENT) != 0, cp = (cf & RF_PRESENT) != 0;
    if (cp) com_present |= 1ull << x;
    mix(ap ? v.x : 0);
    mix(ap ? v.y : 0);
    mix(ap ? v.z : 0);
    mix((int32_t)((ap ? af & (RF_PRESENT | RF_STOP) : 0u) | (cp ? (cf & (RF_PRESENT | RF_STOP | RF_HASVALUE)) << CF_SHIFT : 0u)));
  }
#pragma unroll 4
  for (int32_t x = 0; x < S.W; x++) {
    I4 v = mk4(0, 0, 0, 0);
    if ((com_present >> x) & 1ull) v = S.com_ring[(int64_t)x * G + g];
    mix(v.x);
    mix(v.y);
    mix(v.z);
    mix(v.w);
  }
  if (prep) { /* only after gpx_election_begin: the election arrays exist */
    mix(GPX_IMAGE_FORMAT);
    mix(GPX_IMAGE_CONT);
    mix(0);
    mix(0);
    mix(0);
    mix(g);
    mix((int32_t)S.c_wait[g]);
    for (int32_t j = 7; j < GPX_IMAGE_HEADER_WORDS; j++) mix(0);
#pragma unroll 4
    for (int32_t x = 0; x < S.W; x++) {
      const I4 v = S.co_ring[(int64_t)x * G + g];
      const bool p = (v.w & CO_PRESENT) != 0;
      if (p) co_present |= 1ull << x;
      mix(p ? v.x : 0);
      mix(p ? v.y : 0);
      mix(p ? v.z : 0);
      mix(p ? v.w & (CO_PRESENT | GPX_PV_STOP | GPX_PV_NOOP) : 0);
    }
    for (int32_t x = 0; x < S.W; x++) {
      const uint64_t hv = ((co_present >> x) & 1ull) ? (uint64_t)S.co_handle[(int64_t)x * G + g] : 0ull;
      mix((int32_t)(uint32_t)hv);
      mix((int32_t)(uint32_t)(hv >> 32));
    }
    for (int32_t x = 0; x < S.W; x++) {
      const uint64_t hv = ((p_present >> x) & 1ull) ? (uint64_t)S.p_handle[(int64_t)x * G + g] : 0ull;
      mix((int32_t)(uint32_t)hv);
      mix((int32_t)(uint32_t)(hv >> 32));
    }
  }
  const unsigned long long s = ((unsigned long long)delta_fin(h.a, 0x85ebca6bu, 0xc2b2ae35u) << 32) |
                               (unsigned long long)delta_fin(h.b, 0x7feb352du, 0x846ca68bu);
  return s ? s : 1ull;
}

/* ------------------------------------------------------------------------- */
/* export                                                                      */

__global__ __launch_bounds__(GPX_BLOCK) void k_delta_tile(DevState S, int32_t n, const int32_t* __restrict__ gidx,
                                                         int32_t g_base, int32_t flags, DeltaMem M) {
  __shared__ int32_t w_cnt[4][GPX_COMPACT_WAVES];
  const int32_t t0 = (int32_t)blockIdx.x * GPX_IMAGE_TILE;
  const int64_t i = (int64_t)t0 + (int32_t)threadIdx.x;
  bool live = false, prep = false, chg = false, gone = false;
  int32_t g = 0;
  unsigned long long sig = 0ull;
  if (i < n) {
    g = gidx ? gidx[i] : g_base + (int32_t)i;
    if ((uint32_t)g < (uint32_t)S.G) {
      /* the mark first: its load is in flight while the group is read */
      const unsigned long long mark = M.marks[g];
      const uint32_t gf = S.g_flags[g];
      live = (gf & GF_EXISTS) != 0;
      prep = live && (gf & GF_PREPARING) && S.c_wait;
      if (live) {
        sig = delta_sig(S, g, gf, prep);
        chg = (flags & GPX_DELTA_FULL_) || sig != mark;
      } else {
        gone = mark != 0ull;
      }
    }
  }
  const TileCount<4> c = tile_count(w_cnt, {live, chg, chg && prep, gone});
  if (chg) {
    const int32_t p = t0 + c.before[1];
    M.park[p] = (int32_t)((uint32_t)g | (prep ? GPX_IMAGE_PREP : 0u));
    M.park_sig[p] = sig;
  }
  if (gone) M.park_gone[t0 + c.before[3]] = g;
  if (threadIdx.x == 0) {
    M.tile_live[blockIdx.x] = c.total[0];
    M.tile_chg[blockIdx.x] = c.total[1];
    M.tile_rows[blockIdx.x] = c.total[1] + c.total[2];
    M.tile_gone[blockIdx.x] = c.total[3];
  }
}

__global__ __launch_bounds__(GPX_BLOCK) void k_delta_offsets(int32_t ntiles, DeltaMem M, int32_t cap, int32_t cap_gone,
                                                            DeltaCounts* __restrict__ counts) {
  __shared__ int32_t s_cut;
  if (threadIdx.x == 0) s_cut = -1;
  int32_t sum[4]; /* rows, changed, gone, live */
  tile_offsets<3, 1>(
      ntiles,
      [&](int32_t t, int32_t(&v)[4]) { v[0] = M.tile_rows[t], v[1] = M.tile_chg[t], v[2] = M.tile_gone[t], v[3] = M.tile_live[t]; },
      [&](int32_t t, const int32_t(&off)[3], const int32_t(&v)[4]) {
        M.tile_off[t] = off[0];
        M.tile_goff[t] = off[1];
        M.tile_xoff[t] = off[2];
        if (off[0] <= cap && (int64_t)off[0] + v[0] > cap) s_cut = t; /* at most one tile: offsets ascend */
      },
      sum);
  __syncthreads(); /* s_cut: initialised (ntiles == 0: no barrier above) or stored */
  const int32_t cut = s_cut; /* the same in every lane */
  int32_t n_done = sum[1], n_rows_done = sum[0];
  if (cut >= 0) {
    /* the tile `cap` cuts: the entries of it that still fit (its own words: written above, by this workgroup) */
    const int32_t c = M.tile_chg[cut], off = M.tile_off[cut], j = (int32_t)threadIdx.x;
    const CapCut f = cap_cut(off, j < c ? image_weight(M.park[(int64_t)cut * GPX_IMAGE_TILE + j]) : 0, cap);
    n_done = M.tile_goff[cut] + f.n;
    n_rows_done = off + f.rows;
  }
  if (threadIdx.x == 0) *counts = DeltaCounts{sum[3], sum[1], sum[0], n_done, n_rows_done, sum[2], min(sum[2], cap_gone), 0};
}

__global__ __launch_bounds__(GPX_BLOCK) void k_delta_move(DevState S, DeltaMem M, NameCopies names, ImageIdle idle,
                                                         int32_t cap, int32_t cap_gone, int32_t flags,
                                                         int32_t* __restrict__ o_rows, int32_t* __restrict__ o_gone) {
  __shared__ __attribute__((aligned(16))) int32_t lds[GPX_IMAGE_TILE * GPX_IMAGE_LS];
  __shared__ int32_t s_main[GPX_IMAGE_TILE], s_cont[GPX_IMAGE_TILE];
  const int32_t j = (int32_t)threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * GPX_IMAGE_TILE;
  { /* the gone entries below cap_gone */
    const MoveSpan x = move_span<GPX_IMAGE_TILE>(M.tile_gone, M.tile_xoff, cap_gone);
    if (j < x.lim) {
      const int32_t g = M.park_gone[p0 + j];
      o_gone[x.off + j] = g;
      M.marks[g] = 0ull;
    }
  }
  const int32_t c = M.tile_chg[blockIdx.x], off = M.tile_off[blockIdx.x];
  if (c == 0 || off >= cap) return; /* the same in every lane: a group needs a row, none of this tile's fits */
  const int32_t e = j < c ? M.park[p0 + j] : 0;
  const int32_t g = (int32_t)((uint32_t)e & ~GPX_IMAGE_PREP);
  const bool prep = e < 0;
  int32_t pre = 0;
  const bool fits = weighted_fits(off, j < c ? image_weight(e) : 0, cap, &pre);
  s_main[j] = fits ? off + pre : -1;
  s_cont[j] = fits && prep ? off + pre + 1 : -1;
  const int any_cont = __syncthreads_or(fits && prep);
  const ImageLayout L = image_layout(S);
  const uint32_t gf = fits ? S.g_flags[g] : 0u;
  const unsigned long long sig = fits ? M.park_sig[p0 + j] : 0ull;
  int32_t* mine = &lds[j * GPX_IMAGE_LS];
  for (int32_t lo = 0; lo < L.stride_w; lo += GPX_IMAGE_CW) {
    image_lds_zero(lds);
    __syncthreads();
    if (fits) image_put_main(S, L, g, gf, prep, lo, mine);
    __syncthreads();
    image_lds_flush(lds, s_main, lo, L.stride_w, o_rows);
    __syncthreads();
  }
  if (any_cont)
    for (int32_t lo = 0; lo < L.stride_w; lo += GPX_IMAGE_CW) {
      image_lds_zero(lds);
      __syncthreads();
      if (fits && prep) image_put_cont(S, L, g, lo, mine);
      __syncthreads();
      image_lds_flush(lds, s_cont, lo, L.stride_w, o_rows);
      __syncthreads();
    }
  if (fits) { /* the offsets are known and every word of the group has been read: by this lane alone */
    const bool evict = (flags & GPX_DELTA_EVICT_) != 0;
    M.marks[g] = evict ? 0ull : sig;
    if (evict) {
      group_retire_apply(S, g, names);
      if (idle.sig) {
        idle.sig[g] = 0u;
        idle.age[g] = 0;
      }
    }
  }
}

/* ------------------------------------------------------------------------- */
/* apply                                                                       */

template <bool APPLY>
__global__ __launch_bounds__(GPX_BLOCK) void k_delta_rows(DevState S, ImageMem M, NameCopies names, ImageIdle idle,
                                                         int32_t n_rows, const int32_t* __restrict__ rows,
                                                         const int32_t* __restrict__ gidx, uint8_t* __restrict__ status) {
  image_rows_body<APPLY, true>(S, M, names, idle, n_rows, rows, gidx, status);
}

/* the groups the source no longer has: retired as k_group_retire(GPX_RETIRE_KILL) does */
__global__ __launch_bounds__(GPX_BLOCK) void k_delta_gone(DevState S, NameCopies names, ImageIdle idle, int32_t n_gone,
                                                         const int32_t* __restrict__ gone, uint8_t* __restrict__ gone_status) {
  const int32_t i = (int32_t)(blockIdx.x * GPX_BLOCK + threadIdx.x);
  if (i >= n_gone) return;
  const int32_t g = gone[i];
  if ((uint32_t)g >= (uint32_t)S.G || !(S.g_flags[g] & GF_EXISTS)) {
    gone_status[i] = GPX_S_NOGROUP;
    return;
  }
  group_retire_apply(S, g, names);
  if (idle.sig) {
    idle.sig[g] = 0u;
    idle.age[g] = 0;
  }
  gone_status[i] = GPX_S_OK;
}
