/*
 * gpx_wire_accept.hip.h — the coordinator's ACCEPT frames, packed on the device (include/gpx_wire.h,
 * gpx_wire_pack_accepts_dev / gpx_wire_request_sizes_dev).
 *
 * replaces: RequestPacket.latchToBatch / toArray (RequestPacket.java:1090-1150) over the requests that
 * gpx_request_batch latched together, then AcceptPacket.toBytes (AcceptPacket.java:95-135) behind the
 * (possibly flattened) request bytes - what the C++ host layer does per proposal with latchToBatch +
 * makeAcceptFrame (gigapaxos_amd/host/gpx_host.cpp).
 *
 * Passes (all on the engine's back-end stream, no host sync):
 *   k_acc_parse    per request record: the RequestPacket walker of gpx_wire.hip.h over the record's
 *                  REQUEST frame -> (batched-count position h, end of the batched list e, frame length,
 *                  own batched count); per follower, atomics into its leader's totals (followers, bytes
 *                  of their pieces, elements).  Per proposal: the lowest proposal that names a leader
 *                  record claims it.
 *   k_acc_size     per proposal: frame length, tile totals (bytes / frames / followers)
 *   k_acc_place    per proposal: tile bases + block scan -> frame_off / frame_len / f_gidx / f_batch /
 *                  frame_of and one AccFrame descriptor per frame
 *   k_acc_members  per follower record: its slot inside its leader's segment (unordered)
 *   k_acc_rank     per segment entry: rank by record index (the per-group FIFO) -> sorted members and the
 *                  absolute output offset of each member's piece
 *   k_acc_copy     parallel over OUTPUT bytes: 16 KB tiles; a tile finds its first frame and member piece
 *                  with a wave-wide 64-ary search, stages the descriptors of what it overlaps in LDS, and
 *                  every lane assembles 16-byte chunks from unaligned source dwords (v_alignbyte) into
 *                  aligned dwordx4 stores.  Pad bytes are zero, so every output dword belongs to one frame.
 *                  The searches and the unaligned load are gpx_bytes.hip.h's (wave_search, lds_search,
 *                  load4_unaligned); the loop is this kernel's own: one round, two descriptor lists, padded
 *                  frames, the `fit` rule.
 *
 * A frame is a concatenation of regions, each a byte range of one REQUEST frame with dword-sized patches:
 *   leader   bytes [0, E) of the leader frame; [4, 8) = ACCEPT; flattened: [h, h + 4) = be32(total),
 *            E = end of its batched list (trailing bytes dropped); else E = the whole frame
 *   member   be32(h + 4), then the member's bytes [0, e) with [h, h + 4) = be32(0): its head with an empty
 *            batched list as one element, its own batched elements as top-level elements that follow
 *   tail     be32 slot, be32 bnum, be32 bcoord, u8 0, be32 median, u8 0, be32 my_id (22 bytes)
 */
#pragma once

#define GPX_WA_TAIL 22
#define GPX_WA_TILE 16384                 /* output bytes per workgroup step of k_acc_copy */
#define GPX_WA_SPAN 256                   /* frames / member pieces a tile may overlap (a frame >= 92 B, a piece >= 72 B) */
#define GPX_WA_BAD (1ull << 40)           /* a member that does not parse poisons its leader's byte total */

struct AccRec {  /* per request record (16 bytes: one load) */
  int32_t h;     /* offset of the batched-count field */
  int32_t e;     /* end of the batched list, -1: the frame does not parse */
  int32_t len;   /* frame length */
  int32_t nb;    /* own batched count */
};
struct AccLead { /* per leader record, zeroed every call */
  int32_t own;   /* INT32_MAX - the lowest proposal naming this record as its leader */
  int32_t fcnt;  /* followers; k_acc_members counts it back down */
  int32_t fel;   /* sum over followers of 1 + their batched count */
  int32_t lfr;   /* 1 + the frame whose member segment the followers go to, 0: none (k_acc_place) */
  unsigned long long fbytes; /* sum over followers of their piece bytes (e + 4), + GPX_WA_BAD per unparsable one */
};
struct AccFrame { /* per output frame */
  long long src;  /* leader frame's first byte inside `frames` */
  int32_t E, H;   /* leader region end; batched-count position (flattened) or -1 */
  int32_t total;  /* flattened batched count */
  int32_t fseg, nfol; /* member segment */
  int32_t b;      /* proposal */
};
struct AccScratch {
  AccRec* rec;
  AccLead* lead;
  int32_t *psize, *pfol;      /* per proposal: frame length (0: none), members in the frame */
  long long* tile_b;          /* per 256-proposal tile */
  int32_t *tile_f, *tile_k;
  AccFrame* fd;
  int32_t *flist, *fsorted;   /* member segments: unordered, then by record index */
  long long* fpos;            /* absolute output offset of each sorted member's piece */
  int32_t* n_members;         /* [1] members of all frames */
};
struct AccIn {
  const uint8_t* frames;
  const long long* foff;
  int32_t n_frames, n_req;
  const int32_t *r_frame, *leader;
  int32_t n;
  const int32_t* n_dev;
  const int32_t *b_gidx, *b_leader, *b_count, *slot, *bnum, *bcoord, *median;
  const uint8_t* status;
  int32_t my_id;
};
struct AccOut {
  uint8_t* out;
  long long cap;
  long long* frame_off;
  int32_t *frame_len, *f_gidx, *f_batch, *frame_of, *n_frames;
  long long* n_bytes;
};

__device__ __forceinline__ int32_t acc_props(const AccIn& I) {
  int32_t n = I.n;
  if (I.n_dev) {
    const int32_t m = *I.n_dev;
    n = m < n ? (m < 0 ? 0 : m) : n;
  }
  return n;
}

/* RequestPacket(ByteBuffer) of record i's frame, in place in global memory */
__device__ __forceinline__ AccRec acc_parse(const AccIn& I, int32_t i) {
  AccRec r{0, -1, 0, 0};
  const int32_t fr = I.r_frame[i];
  if ((uint32_t)fr >= (uint32_t)I.n_frames) return r;
  const long long s = I.foff[fr], L = I.foff[fr + 1] - s;
  if (s < 0 || L < 0 || L > 0x7fffffffll) return r;
  const uint8_t* p = I.frames + s;
  int64_t pos = 0;
  int32_t nb = 0;
  bool st = false;
  int64_t rid = 0;
  if (!w_request_fixed(p, pos, (int64_t)L, nb, st, rid)) return r;
  r.h = (int32_t)pos - 4;
  r.nb = nb;
  r.len = (int32_t)L;
  if (nb > 0) { /* the batched elements are walked (and checked) as the decode walked them */
    pos = 0;
    if (!w_walk_request(p, pos, (int64_t)L, st, rid)) return r;
  }
  r.e = (int32_t)pos;
  return r;
}

/* est_bytes / weight columns of gpx_request_batch (gpx_host.cpp: the frame size and batchSizeOf(f) + 1) */
__global__ __launch_bounds__(GPX_BLOCK) void k_acc_req_sizes(AccIn I, int32_t* __restrict__ est_bytes,
                                                            int32_t* __restrict__ weight) {
  const int32_t i = blockIdx.x * GPX_BLOCK + threadIdx.x;
  if (i >= I.n_req) return;
  const AccRec r = acc_parse(I, i);
  est_bytes[i] = r.e >= 0 ? r.len : 0;
  weight[i] = r.e >= 0 ? r.nb + 1 : 1;
}

__global__ __launch_bounds__(GPX_BLOCK) void k_acc_parse(AccIn I, AccScratch X) {
  const int32_t i = blockIdx.x * GPX_BLOCK + threadIdx.x;
  if (i < I.n_req) {
    const AccRec r = acc_parse(I, i);
    X.rec[i] = r;
    const int32_t L = I.leader ? I.leader[i] : -1;
    if ((uint32_t)L < (uint32_t)I.n_req && L != i) {
      AccLead& d = X.lead[L];
      atomicAdd(&d.fcnt, 1);
      if (r.e >= 0) {
        atomicAdd(&d.fel, 1 + r.nb);
        atomicAdd(&d.fbytes, (unsigned long long)r.e + 4ull);
      } else {
        atomicAdd(&d.fbytes, GPX_WA_BAD);
      }
    }
  }
  if (i < acc_props(I)) {
    const int32_t L = I.b_leader ? I.b_leader[i] : i;
    if ((uint32_t)L < (uint32_t)I.n_req) atomicMax(&X.lead[L].own, 0x7fffffff - i);
  }
}

/* proposal b's frame: length (0 = none) and members */
__device__ __forceinline__ int32_t acc_frame_len(const AccIn& I, const AccScratch& X, int32_t n, int32_t b,
                                                 int32_t* nfol, int32_t* L_out, bool* flat_out) {
  *nfol = 0;
  *L_out = -1;
  *flat_out = false;
  if (b >= n || I.status[b] != GPX_S_OK) return 0;
  const int32_t L = I.b_leader ? I.b_leader[b] : b;
  if ((uint32_t)L >= (uint32_t)I.n_req) return 0;
  const AccLead d = X.lead[L];
  if (d.own != 0x7fffffff - b) return 0; /* a later proposal naming the same leader record */
  *L_out = L;
  const AccRec r = X.rec[L];
  if (r.e < 0) return 0;
  const bool flat = I.b_count && I.b_count[b] > 1;
  *flat_out = flat;
  long long len;
  if (!flat) {
    len = (long long)r.len + GPX_WA_TAIL;
  } else {
    const unsigned long long fb = I.leader ? d.fbytes : 0ull;
    if (fb >= GPX_WA_BAD) return 0;
    len = (long long)r.e + (long long)fb + GPX_WA_TAIL;
    *nfol = I.leader ? d.fcnt : 0;
  }
  if (len > 0x7ffffff0ll) {
    *nfol = 0;
    return 0;
  }
  return (int32_t)len;
}

__device__ __forceinline__ long long acc_shfl_up64(long long v, int d) {
  const int lo = __shfl_up((int)(uint32_t)v, d, 64), hi = __shfl_up((int)(uint32_t)((unsigned long long)v >> 32), d, 64);
  return (long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ long long acc_shfl_xor64(long long v, int d) {
  const int lo = __shfl_xor((int)(uint32_t)v, d, 64), hi = __shfl_xor((int)(uint32_t)((unsigned long long)v >> 32), d, 64);
  return (long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
}

/* exclusive scan of a 64-bit value over the workgroup */
__device__ __forceinline__ long long acc_block_exscan64(long long v, long long* total) {
  __shared__ long long ws[GPX_BLOCK / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  long long x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long y = acc_shfl_up64(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) ws[wid] = x;
  __syncthreads();
  long long base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < GPX_BLOCK / 64; w++) {
    const long long s = ws[w];
    if (w < wid) base += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return base + x - v;
}

__global__ __launch_bounds__(GPX_BLOCK) void k_acc_size(AccIn I, AccScratch X) {
  const int32_t n = acc_props(I);
  const int32_t b = blockIdx.x * GPX_BLOCK + threadIdx.x;
  int32_t nfol, L;
  bool flat;
  const int32_t len = acc_frame_len(I, X, n, b, &nfol, &L, &flat);
  if (b < n) {
    X.psize[b] = len;
    X.pfol[b] = nfol;
  }
  long long tb;
  int32_t tf, tk;
  acc_block_exscan64(len ? (long long)((len + 3) & ~3) : 0ll, &tb);
  block_exscan(len ? 1 : 0, &tf);
  block_exscan(nfol, &tk);
  if (threadIdx.x == 0) {
    X.tile_b[blockIdx.x] = tb;
    X.tile_f[blockIdx.x] = tf;
    X.tile_k[blockIdx.x] = tk;
  }
}

__global__ __launch_bounds__(GPX_BLOCK) void k_acc_place(AccIn I, AccScratch X, AccOut O) {
  __shared__ long long s_b[GPX_BLOCK / 64];
  __shared__ int32_t s_f[GPX_BLOCK / 64], s_k[GPX_BLOCK / 64];
  const int32_t n = acc_props(I);
  const int32_t b = blockIdx.x * GPX_BLOCK + threadIdx.x;
  const int32_t len = b < n ? X.psize[b] : 0;
  const int32_t nfol = b < n ? X.pfol[b] : 0;
  /* this tile's base: the totals of the tiles before it (as k_pack_write) */
  long long bb = 0;
  int32_t bf = 0, bk = 0;
  for (int32_t t0 = threadIdx.x; t0 < (int32_t)blockIdx.x; t0 += 4 * GPX_BLOCK) {
    long long vb[4];
    int32_t vf[4], vk[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int32_t t = t0 + k * GPX_BLOCK;
      const bool ok = t < (int32_t)blockIdx.x;
      vb[k] = ok ? X.tile_b[t] : 0;
      vf[k] = ok ? X.tile_f[t] : 0;
      vk[k] = ok ? X.tile_k[t] : 0;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      bb += vb[k];
      bf += vf[k];
      bk += vk[k];
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    bb += acc_shfl_xor64(bb, d);
    bf += __shfl_xor(bf, d, 64);
    bk += __shfl_xor(bk, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_b[threadIdx.x >> 6] = bb;
    s_f[threadIdx.x >> 6] = bf;
    s_k[threadIdx.x >> 6] = bk;
  }
  long long tb;
  int32_t tf, tk;
  const long long eb = acc_block_exscan64(len ? (long long)((len + 3) & ~3) : 0ll, &tb); /* (publishes s_*) */
  const int32_t ef = block_exscan(len ? 1 : 0, &tf);
  const int32_t ek = block_exscan(nfol, &tk);
  long long B0 = 0;
  int32_t F0 = 0, K0 = 0;
#pragma unroll
  for (int w = 0; w < GPX_BLOCK / 64; w++) {
    B0 += s_b[w];
    F0 += s_f[w];
    K0 += s_k[w];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    *O.n_frames = F0 + tf;
    *O.n_bytes = B0 + tb;
    *X.n_members = K0 + tk;
  }
  if (b >= I.n) return;
  const int32_t f = F0 + ef;
  if (O.frame_of) O.frame_of[b] = len ? f : -1;
  if (b >= n) return;
  const int32_t L = I.b_leader ? I.b_leader[b] : b;
  if ((uint32_t)L >= (uint32_t)I.n_req) return;
  /* the owner of a leader record tells its followers where they go (lfr = frame + 1, 0: nowhere) */
  if (X.lead[L].own == 0x7fffffff - b) X.lead[L].lfr = len && nfol ? f + 1 : 0;
  if (!len) return;
  const AccRec r = X.rec[L];
  const bool flat = I.b_count && I.b_count[b] > 1;
  AccFrame F;
  F.src = I.foff[I.r_frame[L]];
  F.E = flat ? r.e : r.len;
  F.H = flat ? r.h : -1;
  F.total = flat ? r.nb + (I.leader ? X.lead[L].fel : 0) : 0;
  F.fseg = K0 + ek;
  F.nfol = nfol;
  F.b = b;
  X.fd[f] = F;
  O.frame_off[f] = B0 + eb;
  O.frame_len[f] = len;
  O.f_gidx[f] = I.b_gidx[b];
  O.f_batch[f] = b;
}

/* follower i -> a free entry of its leader frame's segment */
__global__ __launch_bounds__(GPX_BLOCK) void k_acc_members(AccIn I, AccScratch X) {
  const int32_t i = blockIdx.x * GPX_BLOCK + threadIdx.x;
  if (i >= I.n_req || !I.leader) return;
  const int32_t L = I.leader[i];
  if ((uint32_t)L >= (uint32_t)I.n_req || L == i) return;
  AccLead& d = X.lead[L];
  const int32_t f = d.lfr - 1; /* no frame of a proposal led by this record: the follower stays out */
  if (f < 0) return;
  const int32_t q = atomicSub(&d.fcnt, 1) - 1;
  X.flist[X.fd[f].fseg + q] = i;
}

/* rank of a member by record index inside its segment (the batcher's per-group FIFO), and the byte
 * offset of its piece: a sweep over the segment with 16-byte loads (segments hold up to max_size
 * records; the whole wave mostly reads the same words) */
__global__ __launch_bounds__(GPX_BLOCK) void k_acc_rank(AccIn I, AccScratch X, AccOut O) {
  const int32_t k = blockIdx.x * GPX_BLOCK + threadIdx.x;
  if (k >= *X.n_members) return;
  const int32_t i = X.flist[k];
  const int32_t f = X.lead[I.leader[i]].lfr - 1;
  const AccFrame F = X.fd[f];
  const int32_t* seg = X.flist + F.fseg;
  const int32_t m = F.nfol;
  int32_t rank = 0;
  long long bytes = 0;
  int32_t j = 0;
  const int32_t lead = (int32_t)((4 - (F.fseg & 3)) & 3); /* entries before the first 16-byte aligned one */
  for (; j < m && j < lead; j++) {
    const int32_t v = seg[j];
    if (v < i) {
      rank++;
      bytes += X.rec[v].e + 4;
    }
  }
  for (; j + 4 <= m; j += 4) {
    const int4 v = *(const int4*)(seg + j);
    const int32_t vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (vv[q] < i) {
        rank++;
        bytes += X.rec[vv[q]].e + 4;
      }
  }
  for (; j < m; j++) {
    const int32_t v = seg[j];
    if (v < i) {
      rank++;
      bytes += X.rec[v].e + 4;
    }
  }
  X.fsorted[F.fseg + rank] = i;
  X.fpos[F.fseg + rank] = O.frame_off[f] + F.E + bytes;
}

__device__ __forceinline__ uint32_t acc_be_byte(int32_t v, int32_t k) { /* byte k of be32(v) */
  return ((uint32_t)v >> (24 - 8 * k)) & 0xffu;
}

struct AccTile { /* LDS: what one 16 KB output tile overlaps */
  long long off[GPX_WA_SPAN], src[GPX_WA_SPAN];
  int32_t len[GPX_WA_SPAN], E[GPX_WA_SPAN], H[GPX_WA_SPAN], total[GPX_WA_SPAN], fit[GPX_WA_SPAN];
  int32_t slot[GPX_WA_SPAN], bnum[GPX_WA_SPAN], bcoord[GPX_WA_SPAN], median[GPX_WA_SPAN];
  long long kpos[GPX_WA_SPAN], ksrc[GPX_WA_SPAN];
  int32_t kh[GPX_WA_SPAN], ke[GPX_WA_SPAN];
  int32_t nf, nk;
};

/* byte q of frame j of the tile (q < len) */
__device__ __forceinline__ uint32_t acc_byte(const AccTile& T, const AccIn& I, int32_t j, int32_t q) {
  const int32_t E = T.E[j], len = T.len[j];
  if (q < E) {
    if (q >= 4 && q < 8) return acc_be_byte(GPX_WT_ACCEPT, q - 4);
    const int32_t H = T.H[j];
    if (H >= 0 && q >= H && q < H + 4) return acc_be_byte(T.total[j], q - H);
    return I.frames[T.src[j] + q];
  }
  if (q < len - GPX_WA_TAIL) {
    if (T.nk == 0) return 0u; /* (cannot happen: the tile staged the pieces it overlaps) */
    const long long P = T.off[j] + q;
    const int32_t k = lds_search(T.kpos, T.nk, P);
    const int32_t r = (int32_t)(P - T.kpos[k]), h = T.kh[k];
    if (r < 0 || r >= 4 + T.ke[k]) return 0u;
    if (r < 4) return acc_be_byte(h + 4, r);
    if (r >= 4 + h && r < 8 + h) return 0u;
    return I.frames[T.ksrc[k] + r - 4];
  }
  const int32_t t = q - (len - GPX_WA_TAIL);
  if (t < 4) return acc_be_byte(T.slot[j], t);
  if (t < 8) return acc_be_byte(T.bnum[j], t - 4);
  if (t < 12) return acc_be_byte(T.bcoord[j], t - 8);
  if (t == 12 || t == 17) return 0u; /* recovery, noCoalesce */
  if (t < 17) return acc_be_byte(T.median[j], t - 13);
  return acc_be_byte(I.my_id, t - 18);
}

/* the output dword at frame position q (4-aligned) of frame j */
__device__ __forceinline__ uint32_t acc_dword(const AccTile& T, const AccIn& I, int32_t j, int32_t q) {
  const int32_t E = T.E[j], len = T.len[j];
  if (q == 4) return __builtin_bswap32((uint32_t)GPX_WT_ACCEPT);
  if (q + 4 <= E) {
    const int32_t H = T.H[j];
    if (H < 0 || q + 4 <= H || q >= H + 4) return load4_unaligned<0>(I.frames + T.src[j] + q);
  } else if (q >= E && q + 4 <= len - GPX_WA_TAIL && T.nk > 0) {
    const long long P = T.off[j] + q;
    const int32_t k = lds_search(T.kpos, T.nk, P);
    const int32_t r = (int32_t)(P - T.kpos[k]), h = T.kh[k];
    if (r >= 4 && r + 4 <= 4 + T.ke[k] && (r + 4 <= 4 + h || r >= 8 + h)) return load4_unaligned<0>(I.frames + T.ksrc[k] + r - 4);
  }
  uint32_t w = 0;
#pragma unroll
  for (int c = 0; c < 4; c++)
    if (q + c < len) w |= acc_byte(T, I, j, q + c) << (8 * c);
  return w;
}

__global__ __launch_bounds__(GPX_BLOCK) void k_acc_copy(AccIn I, AccScratch X, AccOut O) {
  __shared__ AccTile T;
  __shared__ int32_t s_first[2];
  const long long total = *O.n_bytes;
  const long long lim = total < O.cap ? total : O.cap;
  const int32_t nF = *O.n_frames, nK = *X.n_members;
  for (long long base = (long long)blockIdx.x * GPX_WA_TILE; base < lim; base += (long long)gridDim.x * GPX_WA_TILE) {
    const long long end = base + GPX_WA_TILE < lim ? base + GPX_WA_TILE : lim;
    if (threadIdx.x < 64) {
      const int32_t f0 = wave_search(O.frame_off, nF, base);
      const int32_t k0 = wave_search(X.fpos, nK, base);
      if (threadIdx.x == 0) {
        s_first[0] = f0 < 0 ? 0 : f0;
        s_first[1] = k0 < 0 ? 0 : k0;
      }
    }
    __syncthreads();
    const int32_t f = s_first[0] + (int32_t)threadIdx.x, k = s_first[1] + (int32_t)threadIdx.x;
    const bool fin = threadIdx.x < GPX_WA_SPAN && f < nF && O.frame_off[f] < end;
    const bool kin = threadIdx.x < GPX_WA_SPAN && k < nK && X.fpos[k] < end;
    if (fin) {
      const int32_t j = threadIdx.x;
      const AccFrame F = X.fd[f];
      const long long off = O.frame_off[f];
      const int32_t len = O.frame_len[f];
      T.off[j] = off;
      T.len[j] = len;
      T.fit[j] = off + ((len + 3) & ~3) <= O.cap;
      T.src[j] = F.src;
      T.E[j] = F.E;
      T.H[j] = F.H;
      T.total[j] = F.total;
      T.slot[j] = I.slot[F.b];
      T.bnum[j] = I.bnum[F.b];
      T.bcoord[j] = I.bcoord[F.b];
      T.median[j] = I.median[F.b];
    }
    if (kin) {
      const int32_t j = threadIdx.x;
      const int32_t i = X.fsorted[k];
      const AccRec r = X.rec[i];
      T.kpos[j] = X.fpos[k];
      T.ksrc[j] = I.foff[I.r_frame[i]];
      T.kh[j] = r.h;
      T.ke[j] = r.e;
    }
    const int32_t cf = __syncthreads_count(fin), ck = __syncthreads_count(kin);
    if (threadIdx.x == 0) {
      T.nf = cf;
      T.nk = ck;
    }
    __syncthreads();
    const int32_t nf = T.nf;
#pragma unroll 1
    for (int c = 0; c < GPX_WA_TILE / (16 * GPX_BLOCK); c++) {
      const long long P = base + (long long)c * (16 * GPX_BLOCK) + 16 * (long long)threadIdx.x;
      if (P >= end) break;
      int32_t j = lds_search(T.off, nf, P);
      uint32_t w[4];
      bool wr[4];
#pragma unroll
      for (int d = 0; d < 4; d++) {
        const long long Q = P + 4 * d;
        while (j + 1 < nf && T.off[j + 1] <= Q) j++;
        const int32_t q = (int32_t)(Q - T.off[j]);
        wr[d] = Q < end && T.fit[j];
        w[d] = wr[d] && q < T.len[j] ? acc_dword(T, I, j, q) : 0u;
      }
      uint32_t* dst = (uint32_t*)(O.out + P);
      if (wr[0] && wr[1] && wr[2] && wr[3]) {
        *(uint4*)dst = make_uint4(w[0], w[1], w[2], w[3]);
      } else {
#pragma unroll
        for (int d = 0; d < 4; d++)
          if (wr[d]) dst[d] = w[d];
      }
    }
    __syncthreads(); /* T is reused by the next tile */
  }
}
