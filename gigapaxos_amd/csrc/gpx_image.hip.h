// Group images (include/gpx_image.h): the full state of groups as fixed-stride rows, out of the table and into it.
//
// The work is a transposition between the engine's column streams (one array per state word, the rings [W][G]) and
// rows of one group each.  Both directions keep the two sides apart:
//   column side   consecutive lanes on consecutive entries: lane j of a tile reads (export) or writes (import) the
//                 words of entry j, a ring entry whole as one 16-byte access.  Coalesced whenever the entries name
//                 consecutive groups (gidx == NULL, any ascending list).
//   row side      through LDS in chunks of GPX_IMAGE_CW = 32 words (128 bytes) of every row of the tile: a wave
//                 moves 16-byte pieces, 8 consecutive lanes on the 128 contiguous bytes of one row's chunk, so every
//                 wave-level row access covers whole 64-byte segments (a stride is a multiple of 64 bytes).
//   LDS           GPX_IMAGE_TILE = 256 rows x GPX_IMAGE_LS = 36 words = 36 KiB per workgroup.  The lane stride of 36
//                 words keeps the 16-byte pieces aligned and spreads the per-lane word accesses over 8 banks (4-way on
//                 ds_write_b32: twice the conflict-free time of an instruction that is a small part of the kernel).
//   no arrays     the ring loops run over the runtime window; a lane never collects ring words in an array of its
//                 own (it would live in scratch): words go straight from global memory to LDS or back.  A ring entry
//                 of the import that straddles two chunks carries its first words in three named registers.
//
// EXPORT is the three launches of gpx_compact.hip.h with a per-entry weight of 1 or 2 rows:
//   k_image_tile     one lane per entry: a live entry parks its group (bit 31: it is running for coordinator and needs
//                    a continuation row); tile_live / tile_rows.
//   k_image_offsets  exclusive prefixes of tile_rows (tile_off) and tile_live (tile_goff), and the counts; where `cap`
//                    cuts a tile it walks that tile's parked entries for the exact n_done (cap_cut).
//   k_image_move     the row offset of parked entry j is tile_off + the prefix of the weights before it; it is written
//                    iff ALL its rows end at or before cap (weighted_fits): the groups written are a prefix.
//                    Under GPX_IMG_EVICT a lane retires its group after it has read the last word of it.
// IMPORT is two launches over tiles of GPX_IMAGE_TILE rows:
//   k_image_rows<false>  judges every row by itself (header, ring indices, c_pcount, every word canonical,
//                        destination) into desc / src; a continuation row looks at p_ring of the row before it for
//                        its p_handle words.  Writes no state.
//   k_image_rows<true>   joins a main row and its continuation (desc / src of rows j - 1, j, j + 1), writes status
//                        and, for the groups taken, every state word: the election words (c_wait, co_ring, co_handle,
//                        p_handle) from the continuation row, or zero where there is none and they are allocated.
//
// SCRATCH INVARIANT (gpx_compact.hip.h), and beyond the export's three launches: k_image_offsets reads parked entries
// below tile_live of the cut tile; k_image_rows<true> reads desc / src of rows < n_rows, all written by
// k_image_rows<false> of the same call.
//
// Bounds.  A parked entry sits at tile * GPX_IMAGE_TILE + rank, rank < GPX_IMAGE_TILE; the host refuses n above the
// entries the parked column holds and n_rows above desc / src.  A group number indexes state only after it has been
// compared with S.G.  An output row index r satisfies r + weight <= cap.  Of an imported row the import itself uses only
// the destination (range checked) as an index; kmax and window must equal the engine's, every loop bound is the engine's
// own.  Words that OTHER kernels use as a bound or an index are checked before a row is taken: k (1..kmax), the ring
// slots (at their index), c_pcount (0..W, the number of present p_ring entries, and while the group is preparing the
// slots c_next - c_pcount .. c_next - 1: k_bucket_prepare_reply writes one output plane per pre-active proposal).  LDS
// indices are below GPX_IMAGE_TILE * GPX_IMAGE_LS by construction (lane * LS + word < CW).
#pragma once

#define GPX_IMAGE_TILE GPX_BLOCK
#define GPX_IMAGE_CW 32
#define GPX_IMAGE_LS 36
#define GPX_IMAGE_PREP 0x80000000u

/* desc byte of an imported row (k_image_rows<false> -> k_image_rows<true>) */
#define IMG_D_BAD 1u       /* the row by itself is no image this engine can take */
#define IMG_D_DEST_SHIFT 1 /* bits 1-2: destination 0 free, 1 out of range, 2 alive */
#define IMG_D_MAIN 16u
#define IMG_D_CONT 32u
#define IMG_D_CONTINUED 64u

struct ImageCounts { /* == gpx_image_counts */
  int32_t n_live, n_rows, n_done, n_rows_done;
};
struct ImageMem {
  int32_t* park;                                        /* [whole tiles] group | GPX_IMAGE_PREP */
  int32_t *tile_live, *tile_rows, *tile_off, *tile_goff; /* [tiles] */
  uint8_t* desc;                                        /* [2 * entries] import: IMG_D_* of every row */
  int32_t* src;                                         /* [2 * entries] import: the row's source gidx word */
};
struct ImageIdle { /* the deactivation sweep's idle words (null: never allocated) */
  uint32_t* sig;
  uint8_t* age;
};

/* words of a row before padding, and the stride in words (a multiple of 16) */
__host__ __device__ inline int32_t image_row_words(int32_t K, int32_t W) { return GPX_IMAGE_HEADER_WORDS + 2 * K + 9 * W; }
__host__ __device__ inline int32_t image_stride_words(int32_t K, int32_t W) { return (image_row_words(K, W) + 15) & ~15; }

struct ImageLayout {
  int32_t K, W;
  int32_t o_mem, o_ns, o_p, o_acc, o_com; /* main row */
  int32_t o_co, o_coh, o_ph;              /* continuation row */
  int32_t stride_w;
};
__device__ __forceinline__ ImageLayout image_layout(const DevState& S) {
  ImageLayout L;
  L.K = S.kmax;
  L.W = S.W;
  L.o_mem = GPX_IMAGE_HEADER_WORDS;
  L.o_ns = L.o_mem + L.K;
  L.o_p = L.o_ns + L.K;
  L.o_acc = L.o_p + L.W;
  L.o_com = L.o_acc + 4 * L.W;
  L.o_co = GPX_IMAGE_HEADER_WORDS;
  L.o_coh = L.o_co + 4 * L.W;
  L.o_ph = L.o_coh + 2 * L.W;
  L.stride_w = image_stride_words(L.K, L.W);
  return L;
}
/* entries [*a, *b) of a section of `count` entries of `ew` words at word `base` that have a word in [lo, hi) */
__device__ __forceinline__ void image_touching(int32_t base, int32_t ew_shift, int32_t count, int32_t lo, int32_t hi,
                                               int32_t* a, int32_t* b) {
  const int32_t ew = 1 << ew_shift;
  *a = lo > base ? (lo - base) >> ew_shift : 0;
  *b = hi > base ? min(count, (hi - base + ew - 1) >> ew_shift) : 0;
}
/* ... and the ones whose LAST word lies in [lo, hi) */
__device__ __forceinline__ void image_ending(int32_t base, int32_t ew_shift, int32_t count, int32_t lo, int32_t hi,
                                             int32_t* a, int32_t* b) {
  *a = lo > base ? (lo - base) >> ew_shift : 0; /* ceil((lo - base - (ew - 1)) / ew) */
  *b = hi > base ? min(count, (hi - base) >> ew_shift) : 0;
}

/* ------------------------------------------------------------------------- */
/* export                                                                      */

__global__ __launch_bounds__(GPX_BLOCK) void k_image_tile(DevState S, int32_t n, const int32_t* __restrict__ gidx,
                                                         int32_t g_base, ImageMem M) {
  __shared__ int32_t w_cnt[2][GPX_COMPACT_WAVES];
  const int32_t t0 = (int32_t)blockIdx.x * GPX_IMAGE_TILE;
  const int64_t i = (int64_t)t0 + (int32_t)threadIdx.x;
  bool live = false, prep = false;
  int32_t g = 0;
  if (i < n) {
    g = gidx ? gidx[i] : g_base + (int32_t)i;
    if ((uint32_t)g < (uint32_t)S.G) {
      const uint32_t gf = S.g_flags[g];
      live = (gf & GF_EXISTS) != 0;
      prep = live && (gf & GF_PREPARING) && S.c_wait;
    }
  }
  const TileCount<2> c = tile_count(w_cnt, {live, prep});
  if (live) M.park[t0 + c.before[0]] = (int32_t)((uint32_t)g | (prep ? GPX_IMAGE_PREP : 0u));
  if (threadIdx.x == 0) {
    M.tile_live[blockIdx.x] = c.total[0];
    M.tile_rows[blockIdx.x] = c.total[0] + c.total[1];
  }
}

/* the weight of parked entry e of the exports: a group that is running for coordinator has a continuation row */
__device__ __forceinline__ int32_t image_weight(int32_t e) { return e < 0 ? 2 : 1; }

__global__ __launch_bounds__(GPX_BLOCK) void k_image_offsets(int32_t ntiles, ImageMem M, int32_t cap,
                                                            ImageCounts* __restrict__ counts) {
  __shared__ int32_t s_cut;
  if (threadIdx.x == 0) s_cut = -1;
  int32_t sum[2]; /* rows, live */
  tile_offsets<2, 0>(
      ntiles, [&](int32_t t, int32_t(&v)[2]) { v[0] = M.tile_rows[t], v[1] = M.tile_live[t]; },
      [&](int32_t t, const int32_t(&off)[2], const int32_t(&v)[2]) {
        M.tile_off[t] = off[0];
        M.tile_goff[t] = off[1];
        if (off[0] <= cap && (int64_t)off[0] + v[0] > cap) s_cut = t; /* at most one tile: offsets ascend */
      },
      sum);
  __syncthreads(); /* s_cut: initialised (ntiles == 0: no barrier above) or stored */
  const int32_t cut = s_cut; /* the same in every lane */
  int32_t n_done = sum[1], n_rows_done = sum[0];
  if (cut >= 0) {
    /* the tile `cap` cuts: the entries of it that still fit (its own words: written above, by this workgroup) */
    const int32_t c = M.tile_live[cut], off = M.tile_off[cut], j = (int32_t)threadIdx.x;
    const CapCut f = cap_cut(off, j < c ? image_weight(M.park[(int64_t)cut * GPX_IMAGE_TILE + j]) : 0, cap);
    n_done = M.tile_goff[cut] + f.n;
    n_rows_done = off + f.rows;
  }
  if (threadIdx.x == 0) *counts = ImageCounts{sum[1], sum[0], n_done, n_rows_done};
}

/* lane's words of chunk [lo, lo + CW) of the MAIN row of live group g into dst (zeroed): canonical.
 * delta_sig (gpx_delta.hip.h) restates these rules and image_put_cont's word for word, to hash the words a row would
 * hold without building it: a change here must be made there too. */
__device__ __forceinline__ void image_put_main(const DevState& S, const ImageLayout& L, int32_t g, uint32_t gf, bool prep,
                                               int32_t lo, int32_t* __restrict__ dst) {
  const int32_t hi = lo + GPX_IMAGE_CW;
  const int64_t G = S.G;
  const bool hc = (gf & GF_HASCOORD) != 0;
  const int32_t k = min((int32_t)GF_K(gf), S.kmax);
  auto put = [&](int32_t wi, int32_t v) {
    const uint32_t d = (uint32_t)(wi - lo);
    if (d < (uint32_t)GPX_IMAGE_CW) dst[d] = v;
  };
  if (lo == 0) { /* the header lies in the first chunk whole: GPX_IMAGE_HEADER_WORDS <= GPX_IMAGE_CW */
    dst[0] = GPX_IMAGE_FORMAT;
    dst[1] = GPX_IMAGE_MAIN;
    dst[2] = (int32_t)(GPX_IMG_F_EXISTS | ((gf & GF_STOPPED) ? GPX_IMG_F_STOPPED : 0) | (hc ? GPX_IMG_F_HASCOORD : 0) |
                       (prep ? GPX_IMG_F_PREPARING | GPX_IMG_F_CONTINUED : 0) | (GF_K(gf) << GPX_IMG_F_K_SHIFT));
    dst[3] = S.my_id;
    dst[4] = S.kmax | (S.W << 16);
    dst[5] = g;
    dst[6] = S.g_version[g];
    dst[7] = S.a_slot[g];
    dst[8] = S.a_bnum[g];
    dst[9] = S.a_bcoord[g];
    dst[10] = S.a_gc[g];
    if (hc) {
      dst[11] = S.c_bnum[g];
      dst[12] = S.c_bcoord[g];
      dst[13] = S.c_next[g];
      dst[14] = S.c_pcount[g];
    }
  }
  int32_t a, b;
  image_touching(L.o_mem, 0, L.K, lo, hi, &a, &b);
  for (int32_t j = a; j < min(b, k); j++) dst[L.o_mem + j - lo] = S.members[(int64_t)j * G + g];
  if (hc) {
    image_touching(L.o_ns, 0, L.K, lo, hi, &a, &b);
    for (int32_t j = a; j < min(b, k); j++) dst[L.o_ns + j - lo] = S.node_slots[(int64_t)j * G + g];
    image_touching(L.o_p, 0, L.W, lo, hi, &a, &b);
    for (int32_t x = a; x < b; x++) {
      const uint32_t e = S.p_ring[(int64_t)x * G + g];
      if (e & PR_PRESENT) dst[L.o_p + x - lo] = (int32_t)(e & (0xffffu | PR_PRESENT | PR_STOP));
    }
  }
  image_touching(L.o_acc, 2, L.W, lo, hi, &a, &b);
  for (int32_t x = a; x < b; x++) {
    const I4 v = S.acc_ring[(int64_t)x * G + g];
    const uint32_t af = (uint32_t)v.w & AF_MASK, cf = ((uint32_t)v.w >> CF_SHIFT) & 0xffu;
    const bool ap = (af & RF_PRESENT) != 0, cp = (cf & RF_PRESENT) != 0;
    const int32_t f = L.o_acc + 4 * x;
    if (ap) {
      put(f, v.x);
      put(f + 1, v.y);
      put(f + 2, v.z);
    }
    put(f + 3, (int32_t)((ap ? af & (RF_PRESENT | RF_STOP) : 0u) |
                         (cp ? (cf & (RF_PRESENT | RF_STOP | RF_HASVALUE)) << CF_SHIFT : 0u)));
  }
  image_touching(L.o_com, 2, L.W, lo, hi, &a, &b);
  for (int32_t x = a; x < b; x++) {
    const int64_t o = (int64_t)x * G + g;
    const uint32_t fw = (uint32_t)((const int32_t*)&S.acc_ring[o])[3];
    if ((fw >> CF_SHIFT) & RF_PRESENT) {
      const I4 v = S.com_ring[o];
      const int32_t f = L.o_com + 4 * x;
      put(f, v.x);
      put(f + 1, v.y);
      put(f + 2, v.z);
      put(f + 3, v.w);
    }
  }
}

/* ... and of the CONTINUATION row of a group that is running for coordinator */
__device__ __forceinline__ void image_put_cont(const DevState& S, const ImageLayout& L, int32_t g, int32_t lo,
                                               int32_t* __restrict__ dst) {
  const int32_t hi = lo + GPX_IMAGE_CW;
  const int64_t G = S.G;
  auto put = [&](int32_t wi, int32_t v) {
    const uint32_t d = (uint32_t)(wi - lo);
    if (d < (uint32_t)GPX_IMAGE_CW) dst[d] = v;
  };
  if (lo == 0) {
    dst[0] = GPX_IMAGE_FORMAT;
    dst[1] = GPX_IMAGE_CONT;
    dst[5] = g;
    dst[6] = (int32_t)S.c_wait[g];
  }
  int32_t a, b;
  image_touching(L.o_co, 2, L.W, lo, hi, &a, &b);
  for (int32_t x = a; x < b; x++) {
    const I4 v = S.co_ring[(int64_t)x * G + g];
    if (v.w & CO_PRESENT) {
      const int32_t f = L.o_co + 4 * x;
      put(f, v.x);
      put(f + 1, v.y);
      put(f + 2, v.z);
      put(f + 3, v.w & (CO_PRESENT | GPX_PV_STOP | GPX_PV_NOOP));
    }
  }
  image_touching(L.o_coh, 1, L.W, lo, hi, &a, &b);
  for (int32_t x = a; x < b; x++) {
    const int64_t o = (int64_t)x * G + g;
    if (((const int32_t*)&S.co_ring[o])[3] & CO_PRESENT) {
      const uint64_t hv = (uint64_t)S.co_handle[o];
      put(L.o_coh + 2 * x, (int32_t)(uint32_t)hv);
      put(L.o_coh + 2 * x + 1, (int32_t)(uint32_t)(hv >> 32));
    }
  }
  image_touching(L.o_ph, 1, L.W, lo, hi, &a, &b);
  for (int32_t x = a; x < b; x++) {
    const int64_t o = (int64_t)x * G + g;
    if (S.p_ring[o] & PR_PRESENT) {
      const uint64_t hv = (uint64_t)S.p_handle[o];
      put(L.o_ph + 2 * x, (int32_t)(uint32_t)hv);
      put(L.o_ph + 2 * x + 1, (int32_t)(uint32_t)(hv >> 32));
    }
  }
}

__device__ __forceinline__ void image_lds_zero(int32_t* lds) {
  for (int32_t p = (int32_t)threadIdx.x; p < GPX_IMAGE_TILE * GPX_IMAGE_LS / 4; p += GPX_BLOCK) ((I4*)lds)[p] = mk4(0, 0, 0, 0);
}
/* chunk [lo, lo + CW) of the tile's staged rows out: row j of the tile goes to output row s_row[j] (-1: none) */
__device__ __forceinline__ void image_lds_flush(const int32_t* lds, const int32_t* s_row, int32_t lo, int32_t stride_w,
                                                int32_t* __restrict__ o_rows) {
  for (int32_t p = (int32_t)threadIdx.x; p < GPX_IMAGE_TILE * (GPX_IMAGE_CW / 4); p += GPX_BLOCK) {
    const int32_t r = p / (GPX_IMAGE_CW / 4), q = p % (GPX_IMAGE_CW / 4);
    const int32_t row = s_row[r], wi = lo + 4 * q;
    if (row >= 0 && wi < stride_w) *(I4*)(o_rows + (int64_t)row * stride_w + wi) = *(const I4*)&lds[r * GPX_IMAGE_LS + 4 * q];
  }
}

__global__ __launch_bounds__(GPX_BLOCK) void k_image_move(DevState S, ImageMem M, NameCopies names, ImageIdle idle,
                                                         int32_t cap, int32_t flags, int32_t* __restrict__ o_rows) {
  __shared__ __attribute__((aligned(16))) int32_t lds[GPX_IMAGE_TILE * GPX_IMAGE_LS];
  __shared__ int32_t s_main[GPX_IMAGE_TILE], s_cont[GPX_IMAGE_TILE];
  const int32_t c = M.tile_live[blockIdx.x], off = M.tile_off[blockIdx.x];
  if (c == 0 || off >= cap) return; /* the same in every lane: a group needs a row, none of this tile's fits */
  const int32_t j = (int32_t)threadIdx.x;
  const int32_t e = j < c ? M.park[(int64_t)blockIdx.x * GPX_IMAGE_TILE + j] : 0;
  const int32_t g = (int32_t)((uint32_t)e & ~GPX_IMAGE_PREP);
  const bool prep = e < 0;
  int32_t pre = 0;
  const bool fits = weighted_fits(off, j < c ? image_weight(e) : 0, cap, &pre);
  s_main[j] = fits ? off + pre : -1;
  s_cont[j] = fits && prep ? off + pre + 1 : -1;
  const int any_cont = __syncthreads_or(fits && prep);
  const ImageLayout L = image_layout(S);
  const uint32_t gf = fits ? S.g_flags[g] : 0u;
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
  if (fits && (flags & GPX_IMG_EVICT)) { /* every word of the group has been read: by this lane alone */
    group_retire_apply(S, g, names);
    if (idle.sig) {
      idle.sig[g] = 0u;
      idle.age[g] = 0;
    }
  }
}

/* ------------------------------------------------------------------------- */
/* import                                                                      */

/* The two passes of an import.  REPLACE (the delta apply, gpx_delta.hip.h): a destination that is alive is taken like a
 * free one - the second pass writes every state word of a group either way. */
template <bool APPLY, bool REPLACE>
__device__ __forceinline__ void image_rows_body(const DevState& S, const ImageMem& M, const NameCopies& names,
                                                const ImageIdle& idle, int32_t n_rows,
                                                const int32_t* __restrict__ rows, const int32_t* __restrict__ gidx,
                                                uint8_t* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) int32_t lds[GPX_IMAGE_TILE * GPX_IMAGE_LS];
  const ImageLayout L = image_layout(S);
  const int64_t G = S.G;
  const int64_t t0 = (int64_t)blockIdx.x * GPX_IMAGE_TILE;
  const int32_t j = (int32_t)threadIdx.x;
  const int64_t row = t0 + j;
  const bool in = row < n_rows;
  int32_t kind = 0, dest = 0;
  bool go = in;
  if (APPLY) { /* the row's final status: a main row and its continuation are taken or refused together */
    uint8_t st = GPX_S_IMAGE;
    if (in) {
      const uint32_t d = M.desc[row];
      if (d & IMG_D_MAIN) {
        bool bad = (d & IMG_D_BAD) != 0;
        if (d & IMG_D_CONTINUED) {
          bool pair = row + 1 < n_rows;
          if (pair) {
            const uint32_t d1 = M.desc[row + 1];
            pair = (d1 & IMG_D_CONT) && !(d1 & IMG_D_BAD) && M.src[row + 1] == M.src[row];
          }
          bad = bad || !pair;
        }
        const uint32_t dc = (d >> IMG_D_DEST_SHIFT) & 3u;
        st = bad ? GPX_S_IMAGE : (dc == 0 || (REPLACE && dc == 2)) ? GPX_S_OK : dc == 1 ? GPX_S_NOGROUP : GPX_S_EXISTS;
        kind = GPX_IMAGE_MAIN;
        dest = gidx ? gidx[row] : M.src[row];
      } else if ((d & IMG_D_CONT) && row > 0) {
        const uint32_t d0 = M.desc[row - 1];
        if ((d0 & IMG_D_MAIN) && (d0 & IMG_D_CONTINUED) && M.src[row - 1] == M.src[row]) {
          const bool bad = ((d0 | d) & IMG_D_BAD) != 0;
          const uint32_t dc = (d0 >> IMG_D_DEST_SHIFT) & 3u;
          st = bad ? GPX_S_IMAGE : (dc == 0 || (REPLACE && dc == 2)) ? GPX_S_OK : dc == 1 ? GPX_S_NOGROUP : GPX_S_EXISTS;
          kind = GPX_IMAGE_CONT;
          dest = gidx ? gidx[row - 1] : M.src[row - 1];
        }
      }
      status[row] = st;
    }
    go = in && st == GPX_S_OK; /* then dest was found in range and free by the first pass */
  }
  int32_t c0 = 0, c1 = 0, c2 = 0; /* the first words of a ring entry that began in the chunk before */
  unsigned long long com_present = 0ull;
  bool bad = false;
  uint32_t fl = 0u, desc = 0u;
  int32_t src = 0, version = 0;
  int32_t c_next = 0, pcount = 0, p_seen = 0; /* first pass: the header's words, the present p_ring entries met */
  unsigned long long co_present = 0ull;
  const int32_t* w = &lds[j * GPX_IMAGE_LS];
  for (int32_t lo = 0; lo < L.stride_w; lo += GPX_IMAGE_CW) {
    const int32_t hi = lo + GPX_IMAGE_CW;
    __syncthreads(); /* the chunk before has been read */
    for (int32_t p = j; p < GPX_IMAGE_TILE * (GPX_IMAGE_CW / 4); p += GPX_BLOCK) {
      const int32_t r = p / (GPX_IMAGE_CW / 4), q = p % (GPX_IMAGE_CW / 4);
      const int32_t wi = lo + 4 * q;
      I4 v = mk4(0, 0, 0, 0);
      if (t0 + r < n_rows && wi < L.stride_w) v = *(const I4*)(rows + (t0 + r) * L.stride_w + wi);
      *(I4*)&lds[r * GPX_IMAGE_LS + 4 * q] = v;
    }
    __syncthreads();
    if (!go) continue;
    /* word i of the entry that begins at row word f (its last word lies in this chunk) */
    auto word = [&](int32_t f, int32_t i) -> int32_t {
      const int32_t wi = f + i;
      return wi >= lo ? w[wi - lo] : i == 0 ? c0 : i == 1 ? c1 : c2;
    };
    /* the entry of an `ew`-word section that begins in this chunk and ends in the next leaves its words here */
    auto carry = [&](int32_t base, int32_t ew_shift, int32_t count, int32_t b) {
      const int32_t f = base + (b << ew_shift);
      if (b < count && f >= lo && f < hi) {
        c0 = w[f - lo];
        if (f + 1 < hi) c1 = w[f + 1 - lo];
        if (f + 2 < hi) c2 = w[f + 2 - lo];
      }
    };
    if (lo == 0) {
      if (!APPLY) {
        kind = w[1];
        fl = (uint32_t)w[2];
        src = w[5];
        bad = w[0] != GPX_IMAGE_FORMAT;
        if (kind == GPX_IMAGE_MAIN) {
          const int32_t k = (int32_t)((fl >> GPX_IMG_F_K_SHIFT) & 0xffu);
          const uint32_t known = GPX_IMG_F_EXISTS | GPX_IMG_F_STOPPED | GPX_IMG_F_HASCOORD | GPX_IMG_F_PREPARING |
                                 GPX_IMG_F_CONTINUED | (0xffu << GPX_IMG_F_K_SHIFT);
          bad = bad || w[3] != S.my_id || w[4] != (S.kmax | (S.W << 16)) || w[15] != 0 || k < 1 || k > S.kmax ||
                (fl & ~known) || !(fl & GPX_IMG_F_EXISTS) || ((fl & GPX_IMG_F_PREPARING) && !(fl & GPX_IMG_F_HASCOORD)) ||
                (((fl & GPX_IMG_F_CONTINUED) != 0) != ((fl & GPX_IMG_F_PREPARING) != 0));
          /* c_pcount bounds loops and output planes of k_bucket_prepare_reply: 0 .. W, and (below) the number of
           * present p_ring entries; no coordinator, no coordinator words */
          c_next = w[13];
          pcount = w[14];
          bad = bad || ((fl & GPX_IMG_F_HASCOORD) ? (uint32_t)pcount > (uint32_t)S.W : (w[11] | w[12] | w[13] | w[14]) != 0);
          dest = gidx ? gidx[row] : src;
          uint32_t dc = 1u;
          if ((uint32_t)dest < (uint32_t)S.G) dc = (S.g_flags[dest] & GF_EXISTS) ? 2u : 0u;
          desc = IMG_D_MAIN | ((fl & GPX_IMG_F_CONTINUED) ? IMG_D_CONTINUED : 0u) | (dc << IMG_D_DEST_SHIFT);
        } else if (kind == GPX_IMAGE_CONT) {
          bad = bad || !S.c_wait || (w[2] | w[3] | w[4] | w[7] | w[8] | w[9] | w[10] | w[11] | w[12] | w[13] | w[14] | w[15]) != 0;
          desc = IMG_D_CONT;
        } else {
          bad = true;
          go = false;
        }
      } else if (kind == GPX_IMAGE_MAIN) {
        fl = (uint32_t)w[2];
        version = w[6];
        const bool hc = (fl & GPX_IMG_F_HASCOORD) != 0;
        S.g_version[dest] = version;
        S.a_slot[dest] = w[7];
        S.a_bnum[dest] = w[8];
        S.a_bcoord[dest] = w[9];
        S.a_gc[dest] = w[10];
        S.c_bnum[dest] = hc ? w[11] : 0;
        S.c_bcoord[dest] = hc ? w[12] : 0;
        S.c_next[dest] = hc ? w[13] : 0;
        S.c_pcount[dest] = hc ? w[14] : 0;
        if (!(fl & GPX_IMG_F_CONTINUED) && S.c_wait) { /* no continuation row: the election words are the group's too */
          S.c_wait[dest] = 0u;
          for (int32_t x = 0; x < L.W; x++) {
            const int64_t o = (int64_t)x * G + dest;
            S.co_ring[o] = mk4(0, 0, 0, 0);
            S.co_handle[o] = 0;
            S.p_handle[o] = 0;
          }
        }
      } else {
        S.c_wait[dest] = (uint32_t)w[6];
      }
    }
    int32_t a, b;
    /* The first pass refuses every word that is not canonical (include/gpx_image.h), so the second one stores the
     * words of a row as they are and export(import(row)) == row for every row taken. */
    if (kind == GPX_IMAGE_MAIN) {
      const int32_t k = (int32_t)((fl >> GPX_IMG_F_K_SHIFT) & 0xffu);
      const bool hc = (fl & GPX_IMG_F_HASCOORD) != 0;
      image_touching(L.o_mem, 0, L.K, lo, hi, &a, &b);
      for (int32_t q = a; q < b; q++) {
        const int32_t v = w[L.o_mem + q - lo];
        if (APPLY) S.members[(int64_t)q * G + dest] = v;
        else if (q >= k && v != 0) bad = true;
      }
      image_touching(L.o_ns, 0, L.K, lo, hi, &a, &b);
      for (int32_t q = a; q < b; q++) {
        const int32_t v = w[L.o_ns + q - lo];
        if (APPLY) S.node_slots[(int64_t)q * G + dest] = v;
        else if ((q >= k || !hc) && v != 0) bad = true;
      }
      image_touching(L.o_p, 0, L.W, lo, hi, &a, &b);
      for (int32_t x = a; x < b; x++) {
        const uint32_t e = (uint32_t)w[L.o_p + x - lo];
        if (APPLY) {
          S.p_ring[(int64_t)x * G + dest] = e;
        } else if (!hc || !(e & PR_PRESENT)) {
          if (e != 0u) bad = true;
        } else {
          /* the entry of slot c_next - d, 1 <= d <= W; while the group is preparing the proposals are the slots
           * c_next - c_pcount .. c_next - 1 (k_bucket_prepare_reply reads them by position): d <= c_pcount */
          const int32_t d = (int32_t)(((uint32_t)c_next - 1u - (uint32_t)x) & (uint32_t)(L.W - 1)) + 1;
          if ((e & ~(0xffffu | PR_PRESENT | PR_STOP)) || ((fl & GPX_IMG_F_PREPARING) && d > pcount)) bad = true;
          p_seen++;
        }
      }
      image_ending(L.o_acc, 2, L.W, lo, hi, &a, &b);
      for (int32_t x = a; x < b; x++) {
        const int32_t f = L.o_acc + 4 * x;
        const I4 v = mk4(word(f, 0), word(f, 1), word(f, 2), word(f, 3));
        if (APPLY) {
          S.acc_ring[(int64_t)x * G + dest] = v;
        } else {
          const uint32_t fw = (uint32_t)v.w, cf = (fw >> CF_SHIFT) & 0xffu;
          if (fw & ~((uint32_t)(RF_PRESENT | RF_STOP) | ((uint32_t)(RF_PRESENT | RF_STOP | RF_HASVALUE) << CF_SHIFT))) bad = true;
          if (fw & RF_PRESENT) {
            if ((v.x & (L.W - 1)) != x) bad = true;
          } else if ((v.x | v.y | v.z) != 0 || (fw & AF_MASK) != 0u) {
            bad = true;
          }
          if (cf & RF_PRESENT) com_present |= 1ull << x;
          else if (cf != 0u) bad = true;
        }
      }
      carry(L.o_acc, 2, L.W, b);
      image_ending(L.o_com, 2, L.W, lo, hi, &a, &b);
      for (int32_t x = a; x < b; x++) {
        const int32_t f = L.o_com + 4 * x;
        const I4 v = mk4(word(f, 0), word(f, 1), word(f, 2), word(f, 3));
        if (APPLY) {
          S.com_ring[(int64_t)x * G + dest] = v;
        } else if ((com_present >> x) & 1ull) {
          if ((v.x & (L.W - 1)) != x) bad = true;
        } else if ((v.x | v.y | v.z | v.w) != 0) {
          bad = true;
        }
      }
      carry(L.o_com, 2, L.W, b);
    } else {
      image_ending(L.o_co, 2, L.W, lo, hi, &a, &b);
      for (int32_t x = a; x < b; x++) {
        const int32_t f = L.o_co + 4 * x;
        const I4 v = mk4(word(f, 0), word(f, 1), word(f, 2), word(f, 3));
        if (APPLY) {
          S.co_ring[(int64_t)x * G + dest] = v;
        } else if (v.w & CO_PRESENT) {
          if ((v.x & (L.W - 1)) != x || (v.w & ~(CO_PRESENT | GPX_PV_STOP | GPX_PV_NOOP))) bad = true;
          co_present |= 1ull << x;
        } else if ((v.x | v.y | v.z | v.w) != 0) {
          bad = true;
        }
      }
      carry(L.o_co, 2, L.W, b);
      image_ending(L.o_coh, 1, L.W, lo, hi, &a, &b);
      for (int32_t x = a; x < b; x++) {
        const int32_t f = L.o_coh + 2 * x;
        const int32_t h0 = word(f, 0), h1 = word(f, 1);
        if (APPLY) S.co_handle[(int64_t)x * G + dest] = (int64_t)((uint64_t)(uint32_t)h0 | ((uint64_t)(uint32_t)h1 << 32));
        else if (!((co_present >> x) & 1ull) && (h0 | h1) != 0) bad = true;
      }
      carry(L.o_coh, 1, L.W, b);
      image_ending(L.o_ph, 1, L.W, lo, hi, &a, &b);
      for (int32_t x = a; x < b; x++) {
        const int32_t f = L.o_ph + 2 * x;
        const int32_t h0 = word(f, 0), h1 = word(f, 1);
        if (APPLY) {
          S.p_handle[(int64_t)x * G + dest] = (int64_t)((uint64_t)(uint32_t)h0 | ((uint64_t)(uint32_t)h1 << 32));
        } else if ((h0 | h1) != 0) {
          /* a handle needs its proposal: p_ring of the row before, the main row if this pair is taken at all (row
           * index and word offset are the call's and the engine's own, not the row's) */
          const uint32_t pe = row > 0 ? (uint32_t)rows[(row - 1) * L.stride_w + L.o_p + x] : 0u;
          if (!(pe & PR_PRESENT)) bad = true;
        }
      }
      carry(L.o_ph, 1, L.W, b);
    }
  }
  if (!APPLY) {
    if (kind == GPX_IMAGE_MAIN && (fl & GPX_IMG_F_HASCOORD) && p_seen != pcount) bad = true;
    if (in) {
      M.desc[row] = (uint8_t)(desc | (bad ? IMG_D_BAD : 0u));
      M.src[row] = src;
    }
  } else if (go && kind == GPX_IMAGE_MAIN) {
    /* last: the group exists from here on (k_group_create's order) */
    S.g_flags[dest] = GF_EXISTS | ((fl & GPX_IMG_F_STOPPED) ? GF_STOPPED : 0u) | ((fl & GPX_IMG_F_HASCOORD) ? GF_HASCOORD : 0u) |
                      ((fl & GPX_IMG_F_PREPARING) ? GF_PREPARING : 0u) | (((fl >> GPX_IMG_F_K_SHIFT) & 0xffu) << 8);
    names.set(dest, true, true, version);
    if (idle.sig) {
      idle.sig[dest] = 0u;
      idle.age[dest] = 0;
    }
  }
}

template <bool APPLY>
__global__ __launch_bounds__(GPX_BLOCK) void k_image_rows(DevState S, ImageMem M, NameCopies names, ImageIdle idle,
                                                         int32_t n_rows, const int32_t* __restrict__ rows,
                                                         const int32_t* __restrict__ gidx, uint8_t* __restrict__ status) {
  image_rows_body<APPLY, false>(S, M, names, idle, n_rows, rows, gidx, status);
}
