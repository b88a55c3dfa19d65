// The byte-run core of the control plane: what the packers that assemble ONE contiguous byte stream from unaligned
// pieces of other buffers have in common - the journal batches (gpx_journal.hip.h), the journal compaction
// (gpx_journal_gc.hip.h) and, for its searches and its unaligned load, the ACCEPT packer (gpx_wire_accept.hip.h).  A
// family's header holds what is its own: the evaluation, what a descriptor holds, how one 16-byte chunk is produced.
//
// A journal call is four launches on one stream, and no workgroup ever waits for another one:
//
//   k_*_tile     one lane per record, GPX_BLOCK per workgroup: the evaluation (every index and range BEFORE any source
//                byte could be read) and a block scan of the entry sizes in 64 bits (block_scan64).  The tile's sums go
//                to its per-tile words, unconditionally.
//   k_*_offsets  ONE workgroup: the exclusive prefixes of the per-tile words, the sums into the call's counts.  Where a
//                cap cuts, the first tile that is not done whole (caps_cut, caps_first_cut) is evaluated again, one
//                lane per record (caps_done): what is done is exact, and a prefix of the call's entries.
//   k_*_rows     one workgroup per tile that has a done entry: the tile's scan again on top of its bases, the caller's
//                rows and the source descriptors (output position, source position, ...), ascending in position.
//   k_*_copy     the hot one (copy_runs), parallel over OUTPUT bytes, never one lane per entry: tiles of GPX_BYTES_TILE
//                output bytes in a persistent loop.  A wave-wide 64-ary search over the descriptors' positions
//                (wave_search) finds the descriptor that holds the tile's first byte; the descriptors the tile overlaps
//                are staged in LDS in ROUNDS of GPX_BYTES_SPAN, every lane produces aligned 16-byte chunks from the
//                staged descriptors (lds_search, then the family's chunk) and stores them; the call's last chunk is
//                stored dword-wise, then byte-wise: nothing at or beyond out + bytes_done is written.
//
// THE ROUND-ADVANCE ARGUMENT.  A tile may overlap more descriptors than a round stages (a piece is at least 4 bytes:
// 4,097 in 16 KB).  A round that staged a full GPX_BYTES_SPAN covers the chunks up to, not including, the chunk that
// holds the start of its LAST staged descriptor: hi = pos[SPAN - 1] & ~15.  So a chunk never needs a descriptor behind
// the staged ones - except for bytes at or beyond `end`, and those are never stored.  And every round moves on: slot 0
// is the descriptor that holds byte lo, so pos[1] > lo; pieces are at least 4 bytes, so pos[SPAN - 1] >= pos[1] +
// 4 * (SPAN - 2) and hi > lo + 4 * (SPAN - 2) - 15, about 1,000 bytes.  The next round starts at the staged descriptor
// that holds byte hi: the last with pos <= hi, `below - 1` behind j, and below >= 1 because pos[0] <= lo <= hi.
//
// SOURCE READS.  No aligned word is read that holds none of the wanted bytes (load4_unaligned reads its second word only
// when the address is unaligned), so a source block need only be padded to the alignment of the widest load its family
// uses.
//
// SCRATCH INVARIANT, as in gpx_compact.hip.h: every scratch word a call reads is one the SAME call wrote.  k_*_offsets
// reads the per-tile words [0, ntiles): each written unconditionally by its tile's workgroup.  k_*_rows reads the bases
// of its own tile (written for every tile) and the counts.  k_*_copy reads descriptors [0, the done count): k_*_rows
// wrote exactly those.
//
// Bounds.  A descriptor index is below the done count <= n <= max_batch, the size of the descriptor columns.  A row
// index is below n_done <= cap_entries.  An output byte is below bytes_done <= cap_bytes.  A source byte lies inside a
// range the family's evaluation accepted.
//
// Everything here is inlined into its kernel, sized at compile time and kept in registers: no array is indexed by a
// run-time value, so none of these kernels has scratch memory.
// Needs: stream_load4, stream_store4, stream_store16, I4, mk4 (gpx_kernels.hip.h).
#pragma once

#define GPX_BYTES_WAVES (GPX_BLOCK / 64)
#define GPX_BYTES_TILE 16384     /* output bytes per workgroup step of copy_runs */
#define GPX_BYTES_SPAN GPX_BLOCK /* descriptors staged per round: one per lane */

/* last index in [0, n) with a[index] <= key, or -1 (a ascending); the whole wave takes part, 64 samples per round:
 * log64(n) dependent loads */
__device__ __forceinline__ int32_t wave_search(const long long* __restrict__ a, int32_t n, long long key) {
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

/* last index in [0, n) of an LDS array with s[index] <= key (s[0] <= key) */
__device__ __forceinline__ int32_t lds_search(const long long* s, int32_t n, long long key) {
  int32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int32_t mid = (lo + hi) >> 1;
    if (s[mid] <= key) lo = mid;
    else hi = mid;
  }
  return lo;
}

/* four bytes at an arbitrary address, memory order: the aligned words that hold them + v_alignbyte (no word is read
 * that holds none of the four).  BIT: the stream of GPX_NT_STREAMS the bytes belong to, 0 for plain loads. */
template <int BIT>
__device__ __forceinline__ uint32_t load4_unaligned(const uint8_t* p) {
  const uintptr_t a = (uintptr_t)p;
  const int32_t* q = (const int32_t*)(a & ~(uintptr_t)3);
  const uint32_t s = (uint32_t)(a & 3);
  const uint32_t lo = (uint32_t)stream_load4<BIT>(q);
  const uint32_t hi = s ? (uint32_t)stream_load4<BIT>(q + 1) : 0u;
  return __builtin_amdgcn_alignbyte(hi, lo, s);
}

struct Scan64 {
  int32_t ex_c, tot_c, tot_b; /* entries of the lanes below; of the workgroup; a second count of the workgroup */
  long long ex_v, tot_v;      /* bytes of the lanes below; of the workgroup */
};

/* exclusive prefix over the workgroup's lanes of (c, v), the sums of c, b and v; every lane calls it */
__device__ __forceinline__ Scan64 block_scan64(int32_t c, int32_t b, long long v) {
  __shared__ long long w_v[GPX_BYTES_WAVES];
  __shared__ int32_t w_c[GPX_BYTES_WAVES], w_b[GPX_BYTES_WAVES];
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
  Scan64 r{ic - c, 0, 0, iv - v, 0};
#pragma unroll
  for (int32_t q = 0; q < GPX_BYTES_WAVES; q++) {
    if (q < wave) r.ex_c += w_c[q], r.ex_v += w_v[q];
    r.tot_c += w_c[q], r.tot_b += w_b[q], r.tot_v += w_v[q];
  }
  __syncthreads(); /* the words are rewritten by the next scan */
  return r;
}

/* THE CAPS RULE.  Entries are done in order while BOTH caps hold: entry number below cap_entries, last byte at or below
 * cap_bytes.  Positions and ends only grow, so the done entries are a prefix of the call's, and a tile that fits whole
 * is done whole.
 *
 * Is the tile of c entries and v bytes whose bases are (eo, bo) cut, i.e. not done whole?  (eo + c <= n: fits) */
__device__ __forceinline__ bool caps_cut(int32_t c, long long v, int32_t eo, long long bo, int32_t cap_entries,
                                         long long cap_bytes) {
  return c > 0 && (eo + c > cap_entries || bo + v > cap_bytes);
}

/* The first cut tile of the call, INT32_MAX for none: the same in every lane.  `cut` is the lowest cut tile the lane
 * has seen (INT32_MAX: none) and b, x[] that tile's bases; on return b and x[] are the bases of the first cut tile in
 * every lane (unchanged where there is none).  Every lane of the ONE workgroup calls it, once per kernel.  (`cut` by
 * reference: by value the two offsets kernels come out with 8 more VGPRs than they had.) */
template <int NX>
__device__ __forceinline__ int32_t caps_first_cut(const int32_t& cut, long long& b, int32_t (&x)[NX]) {
  __shared__ int32_t w_cut[GPX_BYTES_WAVES], s_x[NX];
  __shared__ long long s_b;
  const int32_t lane = (int32_t)threadIdx.x & 63, wave = (int32_t)threadIdx.x >> 6;
  int32_t first = cut;
#pragma unroll
  for (int32_t d = 1; d < 64; d <<= 1) first = min(first, __shfl_xor(first, d));
  if (lane == 0) w_cut[wave] = first;
  __syncthreads();
#pragma unroll
  for (int32_t q = 0; q < GPX_BYTES_WAVES; q++) first = min(first, w_cut[q]);
  if (first != INT32_MAX) { /* the same in every lane */
    if (cut == first) {
      s_b = b;
#pragma unroll
      for (int k = 0; k < NX; k++) s_x[k] = x[k];
    }
    __syncthreads();
    b = s_b;
#pragma unroll
    for (int k = 0; k < NX; k++) x[k] = s_x[k];
  }
  return first;
}

/* The cut tile again, one lane per record: is the lane's entry (sel, v bytes) done, on top of the tile's bases (e0, b0)?
 * Done entries are a prefix: positions and ends only grow.  Every lane of the workgroup calls it (a scan). */
__device__ __forceinline__ bool caps_done(bool sel, long long v, int32_t e0, long long b0, int32_t cap_entries,
                                          long long cap_bytes) {
  const Scan64 S = block_scan64(sel, 0, v);
  return sel && e0 + S.ex_c < cap_entries && b0 + S.ex_v + v <= cap_bytes;
}

/* THE COPY SKELETON: out[0, lim) from the nD descriptors whose output positions d_pos[] ascend from 0, pieces of at
 * least 4 bytes.  The family F gives
 *   F::Tile                         its LDS block of one round, with long long pos[GPX_BYTES_SPAN]
 *   f.stage(T, e, s)                descriptor e into slot s of T, all but pos
 *   f.chunk(T, P, Pe, k, ns, w)     the four dwords of the chunk [P, Pe), Pe <= P + 16: k is the last of the ns staged
 *                                   descriptors with pos <= P; dwords and bytes at or beyond Pe are not stored
 * and the skeleton the rest.  lo, hi, j and ns are the same in every lane. */
template <class F>
__device__ __forceinline__ void copy_runs(const F& f, const long long* __restrict__ d_pos, int32_t nD,
                                          uint8_t* __restrict__ out, long long lim) {
  __shared__ typename F::Tile T;
  __shared__ int32_t s_first;
  for (long long base = (long long)blockIdx.x * GPX_BYTES_TILE; base < lim; base += (long long)gridDim.x * GPX_BYTES_TILE) {
    const long long end = base + GPX_BYTES_TILE < lim ? base + GPX_BYTES_TILE : lim;
    if (threadIdx.x < 64) {
      const int32_t j0 = wave_search(d_pos, nD, base); /* pos(0) = 0 <= base: never -1 */
      if (threadIdx.x == 0) s_first = j0 < 0 ? 0 : j0;
    }
    __syncthreads();
    int32_t j = s_first; /* the descriptor that holds byte lo */
    long long lo = base;
    while (lo < end) {
      const int32_t e = j + (int32_t)threadIdx.x;
      bool in = false;
      if (e < nD) {
        const long long p = d_pos[e];
        in = p < end;
        if (in) {
          T.pos[threadIdx.x] = p;
          f.stage(T, e, (int32_t)threadIdx.x);
        }
      }
      const int32_t ns = __syncthreads_count(in); /* positions ascend: the staged ones are the first ns */
      /* a full round may be cut short by what is not staged: stop in front of the chunk of its last descriptor */
      long long hi = end;
      if (ns == GPX_BYTES_SPAN) {
        const long long h = T.pos[GPX_BYTES_SPAN - 1] & ~15ll; /* > lo: the round-advance argument */
        hi = h < hi ? h : hi;
      }
      for (long long P = lo + 16 * (long long)threadIdx.x; P < hi; P += 16 * GPX_BLOCK) {
        const long long Pe = P + 16 < end ? P + 16 : end;
        uint32_t w[4];
        f.chunk(T, P, Pe, lds_search(T.pos, ns, P), ns, w); /* pos[0] <= lo <= P */
        if (Pe == P + 16) {
          stream_store16<GPX_NT_JOURNAL>((I4*)(out + P), mk4((int32_t)w[0], (int32_t)w[1], (int32_t)w[2], (int32_t)w[3]));
        } else { /* the last chunk of the call: nothing at or beyond out + lim */
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
      /* the next round starts at the descriptor that holds byte hi; T is restaged only after every lane is here */
      const int32_t below = __syncthreads_count((int32_t)threadIdx.x < ns && T.pos[threadIdx.x] <= hi);
      j += below - 1;
      lo = hi;
    }
  }
}
