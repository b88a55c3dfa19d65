// Journal batches (include/gpx_journal.h): the ACCEPTs that must be logged, as one contiguous run of
// <be32 len><frame bytes> entries with one index row per entry - SQLPaxosLogger.journal()'s loop (SQLPaxosLogger.java:
// 965-1079) and FileLogger::logBatch (gigapaxos_amd/host/gpx_host.cpp) over frames that are already in HBM.
//
// A call is four launches on one stream, the scheme of gpx_scan.hip.h, gpx_timers.hip.h and gpx_wire_accept.hip.h; no
// workgroup ever waits for another one, there is no epoch or look-back word:
//
//   k_jr_tile     one lane per record, GPX_JR_TILE = 256 per workgroup: the selection (status == GPX_S_OK and
//                 GPX_R_TOLOG), the frame test (every index and range BEFORE any byte of a frame could be read), a
//                 block scan of the entry sizes 4 + len in 64 bits.  The tile's entries, refused frames and bytes go to
//                 tile_cnt / tile_bad / tile_bytes [tile], unconditionally.
//   k_jr_offsets  ONE workgroup: exclusive prefixes of tile_cnt and tile_bytes into tile_eoff / tile_boff, the sums into
//                 *counts.  Where a cap cuts, the first tile that does not fit whole is evaluated again here, one lane
//                 per record: n_done and bytes_done are exact.
//   k_jr_rows     one workgroup per tile that has a done entry: the tile's scan again on top of its bases, the e_* rows
//                 and one source descriptor (output position, source position, length) per done entry.
//   k_jr_copy     the hot one, parallel over OUTPUT bytes, never one lane per entry: 16 KB output tiles (k_acc_copy's
//                 scheme).  A wave-wide 64-ary search over the descriptors' positions finds the entry that holds the
//                 tile's first byte; the descriptors of the entries the tile overlaps are staged in LDS, in ROUNDS of
//                 GPX_JR_SPAN: a tile of empty frames overlaps 4,097 entries, and a round covers the 16-byte chunks up
//                 to (not including) the chunk that holds the start of its last staged descriptor, so a chunk never
//                 needs a descriptor that is not staged and every round moves on by at least 1,000 bytes.  Every lane
//                 assembles aligned 16-byte stores from unaligned source dwords (v_alignbyte), and never reads an
//                 aligned source word that holds none of the bytes it needs.
//
// New against k_acc_copy: entries are NOT padded.  An entry is at least 4 bytes, so an output dword touches at most two
// entries: the tail of one and (part of) the length prefix of the next; a prefix can straddle a dword, a 16-byte chunk
// and a tile.  jr_dword builds such a dword from at most three single source bytes and the two prefixes.
//
// Cache policy: the frame bytes and `out` are touched once and go through the stream_* helpers (GPX_NT_JOURNAL of
// GPX_NT_STREAMS, gpx_kernels.hip.h).  The descriptors and the per-tile words are hand-offs between the launches and the
// e_* rows are the caller's: plain.
//
// SCRATCH INVARIANT, as in gpx_scan.hip.h: every scratch word a call reads is one the SAME call wrote.  k_jr_offsets
// reads tile_cnt / tile_bad / tile_bytes [0, ntiles): each written unconditionally by its tile's workgroup.  k_jr_rows
// reads tile_eoff / tile_boff of its own tile (written for every tile) and counts->n_done.  k_jr_copy reads descriptors
// [0, n_done): k_jr_rows wrote exactly those.
//
// Bounds.  A descriptor index is below n_done <= n <= max_batch, the size of the descriptor columns.  A row index is
// below n_done <= cap_entries.  An output byte is below bytes_done <= cap_bytes.  A source byte lies inside a frame
// range that k_jr_tile's test accepted, i.e. inside the window [win_lo, win_hi) that `frames` holds; the aligned words
// jr_load4 reads hold at least one such byte.
#pragma once

#define GPX_JR_TILE GPX_BLOCK /* records per workgroup: one per lane */
#define GPX_JR_WAVES (GPX_BLOCK / 64)
#define GPX_JR_CTILE 16384    /* output bytes per workgroup step of k_jr_copy */
#define GPX_JR_SPAN GPX_BLOCK /* descriptors staged per round: one per lane */
#define GPX_JR_COUNT_ONLY_ 1  /* == GPX_JR_COUNT_ONLY of include/gpx_journal.h (checked in gpx_journal_dev.inc) */
#define GPX_JR_MAX_LEN 0x7ffffffbll /* INT32_MAX - 4: the prefix and the entry size fit 32 bits */

struct JrCounts { /* == gpx_journal_counts */
  int32_t n_entries, n_done, n_bad, reserved;
  long long n_bytes, bytes_done;
};

struct JrIn {
  const uint8_t* frames; /* device memory that holds bytes [win_lo, win_hi) of the caller's block; frames[0] = byte win_lo */
  long long win_lo, win_hi; /* the _dev form: [0, frames_bytes); the host twin: the window it staged */
  int32_t n_frames;
  const long long* frame_off;
  const int32_t *frame_len, *rec_frame;
  const int32_t *gidx, *slot, *bnum, *bcoord;
  const uint8_t *r_flags, *status;
  int32_t n, rec_base; /* record i of this launch is record rec_base + i of the caller's call (host twin: chunks) */
};

struct JrMem {
  int32_t *tile_cnt, *tile_bad, *tile_eoff; /* [tiles] */
  long long *tile_bytes, *tile_boff;        /* [tiles] */
  long long *d_pos, *d_src;                 /* [max_batch] per done entry: pos(e); its frame's first byte in the window */
  int32_t* d_len;                           /* [max_batch] */
};

struct JrOut {
  uint8_t* out;
  long long cap_bytes, base_offset;
  int32_t cap_entries;
  int32_t *e_rec, *e_gidx, *e_slot, *e_bnum, *e_bcoord;
  long long* e_off;
  int32_t* e_len;
};

struct JrRec {
  bool sel, bad; /* an entry; marked to log but refused */
  int32_t len;
  long long src; /* the frame's first byte in the caller's block */
};

/* Record i: selected? usable?  Nothing of `frames` is touched here: indices and ranges only. */
__device__ __forceinline__ JrRec jr_eval(const JrIn& I, long long i) {
  JrRec r{false, false, 0, 0};
  if (i >= I.n) return r;
  if (I.status[i] != GPX_S_OK || !(I.r_flags[i] & GPX_R_TOLOG)) return r;
  r.bad = true;
  const int32_t f = I.rec_frame ? I.rec_frame[i] : I.rec_base + (int32_t)i;
  if ((uint32_t)f >= (uint32_t)I.n_frames) return r;
  const long long s = I.frame_off[f];
  if (s < 0) return r;
  long long L;
  if (I.frame_len) {
    L = I.frame_len[f];
  } else {
    const long long e = I.frame_off[f + 1];
    if (e < s) return r;
    L = e - s; /* both non-negative: no overflow */
  }
  if (L < 0 || L > GPX_JR_MAX_LEN || s < I.win_lo || s > I.win_hi - L) return r;
  r.bad = false;
  r.sel = true;
  r.len = (int32_t)L;
  r.src = s;
  return r;
}

struct JrScan {
  int32_t ex_c, tot_c, tot_b; /* entries of the lanes below; of the workgroup; refused frames of the workgroup */
  long long ex_v, tot_v;      /* bytes of the lanes below; of the workgroup */
};

/* exclusive prefix over the workgroup's lanes of (c, v), the sums of c, b and v; every lane calls it */
__device__ __forceinline__ JrScan jr_scan(int32_t c, int32_t b, long long v) {
  __shared__ long long w_v[GPX_JR_WAVES];
  __shared__ int32_t w_c[GPX_JR_WAVES], w_b[GPX_JR_WAVES];
  const int32_t lane = (int32_t)threadIdx.x & 63, wave = (int32_t)threadIdx.x >> 6;
  int32_t ic = c, ib = b;
  long long iv = v; /* inclusive prefixes within the wave */
#pragma unroll
  for (int32_t d = 1; d < 64; d <<= 1) {
    const int32_t uc = __shfl_up(ic, d), ub = __shfl_up(ib, d);
    const long long uv = __shfl_up(iv, d);
    if (lane >= d) ic += uc, ib += ub, iv += uv;
  }
  if (lane == 63) w_c[wave] = ic, w_b[wave] = ib, w_v[wave] = iv;
  __syncthreads();
  JrScan r{ic - c, 0, 0, iv - v, 0};
#pragma unroll
  for (int32_t q = 0; q < GPX_JR_WAVES; q++) {
    if (q < wave) r.ex_c += w_c[q], r.ex_v += w_v[q];
    r.tot_c += w_c[q], r.tot_b += w_b[q], r.tot_v += w_v[q];
  }
  __syncthreads(); /* the words are rewritten by the next scan */
  return r;
}

__global__ __launch_bounds__(GPX_BLOCK) void k_jr_tile(JrIn I, JrMem M) {
  const JrRec r = jr_eval(I, (long long)blockIdx.x * GPX_JR_TILE + (long long)threadIdx.x);
  const JrScan S = jr_scan(r.sel, r.bad, r.sel ? 4ll + r.len : 0ll);
  if (threadIdx.x == 0) {
    M.tile_cnt[blockIdx.x] = S.tot_c;
    M.tile_bad[blockIdx.x] = S.tot_b;
    M.tile_bytes[blockIdx.x] = S.tot_v;
  }
}

/* one workgroup: the tiles' bases, the counts, and - where a cap cuts - the exact prefix that is done */
__global__ __launch_bounds__(GPX_BLOCK) void k_jr_offsets(int32_t ntiles, JrIn I, JrMem M, long long cap_bytes,
                                                         int32_t cap_entries, int32_t flags,
                                                         JrCounts* __restrict__ counts) {
  __shared__ int32_t w_cut[GPX_JR_WAVES], s_cut_e;
  __shared__ long long s_cut_b;
  const int32_t lane = (int32_t)threadIdx.x & 63, wave = (int32_t)threadIdx.x >> 6;
  int32_t run_c = 0, run_bad = 0, cut = INT32_MAX, cut_e = 0;
  long long run_v = 0, cut_b = 0;
  for (int32_t t0 = 0; t0 < ntiles; t0 += GPX_BLOCK) {
    const int32_t t = t0 + (int32_t)threadIdx.x;
    const int32_t c = t < ntiles ? M.tile_cnt[t] : 0, b = t < ntiles ? M.tile_bad[t] : 0;
    const long long v = t < ntiles ? M.tile_bytes[t] : 0;
    const JrScan S = jr_scan(c, b, v);
    const int32_t eo = run_c + S.ex_c; /* <= n: fits */
    const long long bo = run_v + S.ex_v;
    if (t < ntiles) {
      M.tile_eoff[t] = eo;
      M.tile_boff[t] = bo;
      /* the first tile that is not done whole; a lane's tiles come in ascending order */
      if (c > 0 && cut == INT32_MAX && (eo + c > cap_entries || bo + v > cap_bytes)) cut = t, cut_e = eo, cut_b = bo;
    }
    run_c += S.tot_c, run_bad += S.tot_b, run_v += S.tot_v;
  }
  int32_t first = cut;
#pragma unroll
  for (int32_t d = 1; d < 64; d <<= 1) first = min(first, __shfl_xor(first, d));
  if (lane == 0) w_cut[wave] = first;
  __syncthreads();
#pragma unroll
  for (int32_t q = 0; q < GPX_JR_WAVES; q++) first = min(first, w_cut[q]);
  int32_t n_done = run_c;
  long long bytes_done = run_v;
  if (first != INT32_MAX) { /* the same in every lane */
    if (cut == first) s_cut_e = cut_e, s_cut_b = cut_b;
    __syncthreads();
    const int32_t e0 = s_cut_e;
    const long long b0 = s_cut_b;
    const JrRec r = jr_eval(I, (long long)first * GPX_JR_TILE + (long long)threadIdx.x);
    const long long v = r.sel ? 4ll + r.len : 0ll;
    const JrScan S = jr_scan(r.sel, 0, v);
    /* done entries are a prefix: positions and ends only grow */
    const bool done = r.sel && e0 + S.ex_c < cap_entries && b0 + S.ex_v + v <= cap_bytes;
    const JrScan D = jr_scan(done, 0, done ? v : 0ll);
    n_done = e0 + D.tot_c;
    bytes_done = b0 + D.tot_v;
  }
  if (flags & GPX_JR_COUNT_ONLY_) n_done = 0, bytes_done = 0;
  if (threadIdx.x == 0) *counts = JrCounts{run_c, n_done, run_bad, 0, run_v, bytes_done};
}

__global__ __launch_bounds__(GPX_BLOCK) void k_jr_rows(JrIn I, JrMem M, JrOut O, const JrCounts* __restrict__ counts) {
  const int32_t n_done = counts->n_done, e0 = M.tile_eoff[blockIdx.x];
  if (e0 >= n_done) return; /* the whole workgroup: nothing of this tile is done */
  const long long i = (long long)blockIdx.x * GPX_JR_TILE + (long long)threadIdx.x;
  const JrRec r = jr_eval(I, i);
  const JrScan S = jr_scan(r.sel, 0, r.sel ? 4ll + r.len : 0ll);
  const int32_t e = e0 + S.ex_c;
  if (!r.sel || e >= n_done) return;
  const long long pos = M.tile_boff[blockIdx.x] + S.ex_v;
  if (O.e_rec) O.e_rec[e] = I.rec_base + (int32_t)i;
  if (O.e_gidx) O.e_gidx[e] = I.gidx[i];
  if (O.e_slot) O.e_slot[e] = I.slot[i];
  if (O.e_bnum) O.e_bnum[e] = I.bnum[i];
  if (O.e_bcoord) O.e_bcoord[e] = I.bcoord[i];
  O.e_off[e] = O.base_offset + pos;
  O.e_len[e] = r.len;
  M.d_pos[e] = pos;
  M.d_src[e] = r.src - I.win_lo;
  M.d_len[e] = r.len;
}

/* last index in [0, n) with a[index] <= key, or -1 (a ascending); the whole wave takes part, 64 samples per round:
 * log64(n) dependent loads (acc_wave_search of gpx_wire_accept.hip.h) */
__device__ __forceinline__ int32_t jr_wave_search(const long long* __restrict__ a, int32_t n, long long key) {
  const int32_t lane = (int32_t)threadIdx.x & 63;
  int32_t lo = -1, hi = n;
  while (hi - lo > 1) {
    const int32_t step = (hi - lo - 1 + 63) / 64;
    const int32_t idx = lo + 1 + lane * step;
    const bool le = idx < hi && a[idx] <= key;
    const int32_t c = __popcll(__ballot(le));
    const int32_t cand = lo + 1 + c * step;
    if (c > 0) lo = lo + 1 + (c - 1) * step;
    hi = cand < hi ? cand : hi;
  }
  return lo;
}

/* four bytes at an arbitrary address, memory order: the aligned words that hold them + v_alignbyte (no word is read
 * that holds none of the four) */
__device__ __forceinline__ uint32_t jr_load4(const uint8_t* p) {
  const uintptr_t a = (uintptr_t)p;
  const int32_t* q = (const int32_t*)(a & ~(uintptr_t)3);
  const uint32_t s = (uint32_t)(a & 3);
  const uint32_t lo = (uint32_t)stream_load4<GPX_NT_JOURNAL>(q);
  const uint32_t hi = s ? (uint32_t)stream_load4<GPX_NT_JOURNAL>(q + 1) : 0u;
  return __builtin_amdgcn_alignbyte(hi, lo, s);
}

struct JrTile { /* LDS: one round of descriptors */
  long long pos[GPX_JR_SPAN], src[GPX_JR_SPAN];
  int32_t len[GPX_JR_SPAN];
};

/* The output dword at position Q, which lies inside staged entry k (pos[k] <= Q < pos[k] + 4 + len[k]); ns entries are
 * staged.  Bytes of the entry behind k come from its prefix alone (it is at least 4 bytes long); where that entry is not
 * staged it starts at or beyond the end of what the caller stores, and those bytes stay 0. */
__device__ __forceinline__ uint32_t jr_dword(const JrTile& T, const uint8_t* frames, int32_t k, int32_t ns, long long Q) {
  const long long r = Q - T.pos[k], L = 4ll + T.len[k];
  if (r >= 4 && r + 4 <= L) return jr_load4(frames + T.src[k] + (r - 4));
  uint32_t w = 0;
  if (r < 4) w = __builtin_bswap32((uint32_t)T.len[k]) >> (8 * (int32_t)r); /* be32(len), bytes r .. 3 */
  const long long b0 = r > 4 ? r : 4, b1 = r + 4 < L ? r + 4 : L;
  for (long long o = b0; o < b1; o++) w |= (uint32_t)frames[T.src[k] + (o - 4)] << (8 * (int32_t)(o - r));
  if (r + 4 > L && k + 1 < ns) w |= __builtin_bswap32((uint32_t)T.len[k + 1]) << (8 * (int32_t)(L - r));
  return w;
}

__global__ __launch_bounds__(GPX_BLOCK) void k_jr_copy(const uint8_t* __restrict__ frames, JrMem M,
                                                      uint8_t* __restrict__ out, const JrCounts* __restrict__ counts) {
  __shared__ JrTile T;
  __shared__ int32_t s_first;
  const long long lim = counts->bytes_done;
  const int32_t nE = counts->n_done;
  for (long long base = (long long)blockIdx.x * GPX_JR_CTILE; base < lim; base += (long long)gridDim.x * GPX_JR_CTILE) {
    const long long end = base + GPX_JR_CTILE < lim ? base + GPX_JR_CTILE : lim;
    if (threadIdx.x < 64) {
      const int32_t j0 = jr_wave_search(M.d_pos, nE, base); /* pos(0) = 0 <= base: never -1 */
      if (threadIdx.x == 0) s_first = j0 < 0 ? 0 : j0;
    }
    __syncthreads();
    int32_t j = s_first; /* the entry that holds byte lo */
    long long lo = base;
    while (lo < end) { /* rounds: lo, hi, j and ns are the same in every lane */
      const int32_t e = j + (int32_t)threadIdx.x;
      bool in = false;
      if (e < nE) {
        const long long p = M.d_pos[e];
        in = p < end;
        if (in) {
          T.pos[threadIdx.x] = p;
          T.src[threadIdx.x] = M.d_src[e];
          T.len[threadIdx.x] = M.d_len[e];
        }
      }
      const int32_t ns = __syncthreads_count(in); /* positions ascend: the staged ones are the first ns */
      /* a full round may be cut short by what is not staged: stop in front of the chunk of its last descriptor */
      long long hi = end;
      if (ns == GPX_JR_SPAN) {
        const long long h = T.pos[GPX_JR_SPAN - 1] & ~15ll; /* >= pos[1] + 4 * (SPAN - 2) - 15 > lo */
        hi = h < hi ? h : hi;
      }
      for (long long P = lo + 16 * (long long)threadIdx.x; P < hi; P += 16 * GPX_BLOCK) {
        int32_t k = 0, kh = ns; /* the last staged entry with pos <= P: pos[0] <= lo <= P */
        while (kh - k > 1) {
          const int32_t mid = (k + kh) >> 1;
          if (T.pos[mid] <= P) k = mid;
          else kh = mid;
        }
        uint32_t w[4];
#pragma unroll
        for (int32_t d = 0; d < 4; d++) {
          const long long Q = P + 4 * d;
          while (k + 1 < ns && T.pos[k + 1] <= Q) k++;
          w[d] = Q < end ? jr_dword(T, frames, k, ns, Q) : 0u;
        }
        if (P + 16 <= end) {
          stream_store16<GPX_NT_JOURNAL>((I4*)(out + P), mk4((int32_t)w[0], (int32_t)w[1], (int32_t)w[2], (int32_t)w[3]));
        } else { /* the last chunk of the call: nothing at or beyond out + bytes_done */
#pragma unroll
          for (int32_t d = 0; d < 4; d++) {
            const long long Q = P + 4 * d;
            if (Q + 4 <= end) {
              stream_store4<GPX_NT_JOURNAL>((uint32_t*)(out + Q), w[d]);
            } else {
              for (int32_t c = 0; c < 4; c++)
                if (Q + c < end) out[Q + c] = (uint8_t)(w[d] >> (8 * c));
            }
          }
        }
      }
      /* the next round starts at the entry that holds byte hi; T is restaged only after every lane is here */
      const int32_t below = __syncthreads_count((int32_t)threadIdx.x < ns && T.pos[threadIdx.x] <= hi);
      j += below - 1;
      lo = hi;
    }
  }
}
