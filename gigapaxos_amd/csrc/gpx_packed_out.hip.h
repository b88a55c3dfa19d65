/*
 * gpx_packed_out.hip.h — proposals and decisions as packed records in one buffer (include/gpx_packed_out.h): the
 * writing and the reading of one entry (host and device share them), the two streaming kernels that make a packed
 * buffer of the plain output columns, the kernel that moves it through a host mapping, and the host-side packers
 * and unpackers.
 *
 * A lane takes four consecutive entries: 16-byte loads of the int32 columns, one 32-bit load of the byte column,
 * 16-byte stores of the records (two per lane for decisions, one for proposals) or of the columns.  Rows are numbered
 * in entry order by two launches: k_po_count leaves the rows every workgroup needs (and the reference entry in the
 * header), k_po_write adds up the counts in front of its workgroup - as k_emit_dec16 does for buckets - decides the
 * form from the total and writes.  Every word either kernel reads was written by this call or by the call that made
 * the columns: no epoch tag, no wrap branch.
 */
#pragma once
#include <string.h>

#include "../../include/gpx_packed_out.h"
#include "gpx_kernels.hip.h"

#define GPX_PO_QUAD (4 * GPX_BLOCK) /* entries of one workgroup */

/* the reference of a call (include/gpx_packed_out.h, the packing rule): header words 4 .. 7 */
struct PoRef {
  int32_t bnum, bcoord;
  uint32_t base_slot, base_cp;
};
/* the plain columns a pack kernel reads; gidx only for decisions, b = d_kind / status */
struct PoSrc {
  const int32_t *gidx, *slot, *bnum, *bcoord, *cp;
  const uint8_t* b;
};

/* WRITING one entry: does it fit a delta record, and the delta bits of its word */
__host__ __device__ __forceinline__ bool po_fits(const PoRef& R, int32_t bnum, int32_t bcoord, int32_t slot, int32_t cp,
                                                 uint32_t& w) {
  const uint32_t ds = (uint32_t)slot - R.base_slot, dp = (uint32_t)cp - R.base_cp;
  w = (ds & 255u) | (dp & 255u) << 8;
  return bnum == R.bnum && bcoord == R.bcoord && ds < 256u && dp < 256u;
}
/* READING one delta record: (slot, median_cp, kind / status) */
__host__ __device__ __forceinline__ void po_delta(const PoRef& R, uint32_t w, int32_t& slot, int32_t& cp, uint8_t& b) {
  slot = (int32_t)(R.base_slot + (w & 255u));
  cp = (int32_t)(R.base_cp + ((w >> 8) & 255u));
  b = (uint8_t)((w >> 16) & 255u);
}
/* bytes a buffer with this header uses, or -1 */
__host__ __device__ __forceinline__ int64_t po_size(int32_t form, int32_t kind, int32_t n, int32_t n_exc) {
  if (n < 0 || n_exc < 0 || (kind != GPX_PO_DECISIONS && kind != GPX_PO_PROPOSALS)) return -1;
  const int64_t S = ((int64_t)4 * n + 31) & ~(int64_t)31;
  if (form == GPX_PO_RECORDS)
    return 32 + (kind == GPX_PO_DECISIONS ? (((int64_t)8 * n + 31) & ~(int64_t)31) : S) + (int64_t)32 * n_exc;
  if (form == GPX_PO_COLUMNS && n_exc == 0)
    return 32 + (kind == GPX_PO_DECISIONS ? 5 : 4) * S + (((int64_t)n + 31) & ~(int64_t)31);
  return -1;
}

/* ---- device ---------------------------------------------------------------------------------------------- */
/* The reference among the first min(n, 64) entries, by the whole workgroup (a broadcast read of 64 entries). */
__device__ __forceinline__ PoRef po_reference(int32_t n, const PoSrc& S) {
  __shared__ int32_t s_bn[GPX_PO_REF_WINDOW], s_bc[GPX_PO_REF_WINDOW], s_key[GPX_PO_REF_WINDOW];
  __shared__ PoRef s_ref;
  const int32_t m = n < GPX_PO_REF_WINDOW ? n : GPX_PO_REF_WINDOW, tid = threadIdx.x;
  if (tid < m) s_bn[tid] = S.bnum[tid], s_bc[tid] = S.bcoord[tid];
  __syncthreads();
  if (tid < m) {
    int32_t cnt = 0, first = -1;
    for (int32_t j = 0; j < m; j++) {
      const bool eq = s_bn[j] == s_bn[tid] && s_bc[j] == s_bc[tid];
      cnt += eq;
      first = (eq && first < 0) ? j : first;
    }
    /* more occurrences win; among equals the earlier first occurrence */
    s_key[tid] = first == tid ? cnt * GPX_PO_REF_WINDOW + (GPX_PO_REF_WINDOW - 1 - tid) : -1;
  }
  __syncthreads();
  if (tid == 0) {
    PoRef R{0, 0, 0u, 0u};
    int32_t best = -1;
    for (int32_t j = 0; j < m; j++) best = s_key[j] > best ? s_key[j] : best;
    if (best >= 0) {
      const int32_t i = GPX_PO_REF_WINDOW - 1 - (best & (GPX_PO_REF_WINDOW - 1));
      R = PoRef{s_bn[i], s_bc[i], (uint32_t)S.slot[i] - 128u, (uint32_t)S.cp[i] - 128u};
    }
    s_ref = R;
  }
  __syncthreads();
  return s_ref;
}

/* a lane's four entries 4 t .. 4 t + 3: 16-byte loads where all four exist, entry by entry at the end of the call
 * (nothing at or beyond entry n is read); v[j] = (gidx, slot, bnum, bcoord, median_cp, byte) */
template <int KIND>
__device__ __forceinline__ void po_load(const PoSrc& S, int32_t t, int32_t n, int32_t (&v)[4][6]) {
  const int64_t i0 = (int64_t)4 * t;
  if (i0 + 3 < n) {
    const int4 sl = ((const int4*)S.slot)[t], bn = ((const int4*)S.bnum)[t], bc = ((const int4*)S.bcoord)[t],
               cp = ((const int4*)S.cp)[t];
    const uint32_t b = ((const uint32_t*)S.b)[t];
    int4 g = make_int4(0, 0, 0, 0);
    if (KIND == GPX_PO_DECISIONS) g = ((const int4*)S.gidx)[t];
    v[0][0] = g.x, v[1][0] = g.y, v[2][0] = g.z, v[3][0] = g.w;
    v[0][1] = sl.x, v[1][1] = sl.y, v[2][1] = sl.z, v[3][1] = sl.w;
    v[0][2] = bn.x, v[1][2] = bn.y, v[2][2] = bn.z, v[3][2] = bn.w;
    v[0][3] = bc.x, v[1][3] = bc.y, v[2][3] = bc.z, v[3][3] = bc.w;
    v[0][4] = cp.x, v[1][4] = cp.y, v[2][4] = cp.z, v[3][4] = cp.w;
#pragma unroll
    for (int j = 0; j < 4; j++) v[j][5] = (int32_t)((b >> (8 * j)) & 255u);
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int64_t i = i0 + j;
      const bool in = i < n;
      v[j][0] = (in && KIND == GPX_PO_DECISIONS) ? S.gidx[i] : 0;
      v[j][1] = in ? S.slot[i] : 0;
      v[j][2] = in ? S.bnum[i] : 0;
      v[j][3] = in ? S.bcoord[i] : 0;
      v[j][4] = in ? S.cp[i] : 0;
      v[j][5] = in ? (int32_t)S.b[i] : 0;
    }
  }
}

/* the call's entry count: the device count of a decisions call (clamped to the capacity), or the capacity itself */
__device__ __forceinline__ int32_t po_count_of(const int32_t* __restrict__ n_dev, int32_t cap) {
  int32_t n = n_dev ? *n_dev : cap;
  n = n < 0 ? 0 : n;
  return n > cap ? cap : n;
}

/* launch 1: counts[workgroup] = rows its GPX_PO_QUAD entries need; workgroup 0 leaves the reference in header words
 * 4 .. 7 (one 16-byte store) */
template <int KIND>
__global__ __launch_bounds__(GPX_BLOCK) void k_po_count(const int32_t* __restrict__ n_dev, int32_t cap, PoSrc S,
                                                       int32_t* __restrict__ counts, int4* __restrict__ hdr) {
  __shared__ int32_t s_w[GPX_BLOCK / 64];
  const int32_t n = po_count_of(n_dev, cap);
  const PoRef R = po_reference(n, S);
  const int32_t t = blockIdx.x * GPX_BLOCK + threadIdx.x;
  int32_t c = 0;
  if ((int64_t)4 * t < n) {
    int32_t v[4][6];
    po_load<KIND>(S, t, n, v);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      uint32_t w;
      c += ((int64_t)4 * t + j < n) && !po_fits(R, v[j][2], v[j][3], v[j][1], v[j][4], w);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t s = 0;
#pragma unroll
    for (int w = 0; w < GPX_BLOCK / 64; w++) s += s_w[w];
    counts[blockIdx.x] = s;
    if (blockIdx.x == 0) hdr[1] = make_int4(R.bnum, R.bcoord, (int32_t)R.base_slot, (int32_t)R.base_cp);
  }
}

/* zero words from the end of what the last lane of an area wrote to the area's 32-byte boundary */
__device__ __forceinline__ void po_zero_to(uint8_t* area, int64_t from, int64_t to) {
  for (int64_t o = from; o < to; o += 4) *(uint32_t*)(area + o) = 0u;
}

/* launch 2: the form from the total, then the records and rows, or the columns */
template <int KIND>
__global__ __launch_bounds__(GPX_BLOCK) void k_po_write(const int32_t* __restrict__ n_dev, int32_t cap, PoSrc S,
                                                       const int32_t* __restrict__ counts, uint8_t* out) {
  __shared__ int32_t s_b[GPX_BLOCK / 64], s_t[GPX_BLOCK / 64], s_w[GPX_BLOCK / 64];
  constexpr int NC = KIND == GPX_PO_DECISIONS ? 5 : 4;
  const int32_t n = po_count_of(n_dev, cap);
  const int32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int4 rv = ((const int4*)out)[1]; /* k_po_count's */
  const PoRef R{rv.x, rv.y, (uint32_t)rv.z, (uint32_t)rv.w};
  /* rows in front of this workgroup, and in the whole call */
  int32_t before = 0, total = 0;
  for (int32_t j = tid; j < (int32_t)gridDim.x; j += GPX_BLOCK) {
    const int32_t c = counts[j];
    total += c;
    before += j < (int32_t)blockIdx.x ? c : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o), total += __shfl_xor(total, o);
  if (lane == 0) s_b[wv] = before, s_t[wv] = total;
  __syncthreads();
  before = total = 0;
#pragma unroll
  for (int w = 0; w < GPX_BLOCK / 64; w++) before += s_b[w], total += s_t[w];
  const bool records = total <= n / GPX_PO_EXC_DIV;
  if (blockIdx.x == 0 && tid == 0)
    ((int4*)out)[0] = make_int4(records ? GPX_PO_RECORDS : GPX_PO_COLUMNS, KIND, n, records ? total : 0);

  const int32_t t = blockIdx.x * GPX_BLOCK + tid;
  const int64_t i0 = (int64_t)4 * t;
  int32_t v[4][6];
  uint32_t w[4];
  bool need[4];
#pragma unroll
  for (int j = 0; j < 4; j++) need[j] = false, w[j] = 0u;
  if (i0 < n) {
    po_load<KIND>(S, t, n, v);
#pragma unroll
    for (int j = 0; j < 4; j++) need[j] = (i0 + j < n) && !po_fits(R, v[j][2], v[j][3], v[j][1], v[j][4], w[j]);
  }
  /* this lane's first row: the rows of the lanes in front of it in the workgroup, entry order */
  int32_t below = 0, wave_rows = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const unsigned long long mk = __ballot(need[j]);
    below += __popcll(mk & ((1ull << lane) - 1ull));
    wave_rows += __popcll(mk);
  }
  if (lane == 0) s_w[wv] = wave_rows;
  __syncthreads();
  int32_t r = before + below;
#pragma unroll
  for (int k = 0; k < GPX_BLOCK / 64; k++) r += k < wv ? s_w[k] : 0;
  if (i0 >= n) return;

  const bool last = i0 + 4 >= n;              /* the lane that holds the call's last entry */
  const int64_t S4 = ((int64_t)4 * n + 31) & ~(int64_t)31; /* R(4 n) */
  if (records) {
    uint32_t word[4];
    int4* rows = (int4*)(out + 32 + (KIND == GPX_PO_DECISIONS ? (((int64_t)8 * n + 31) & ~(int64_t)31) : S4));
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t b = KIND == GPX_PO_DECISIONS ? ((uint32_t)v[j][5] & 3u) : ((uint32_t)v[j][5] & 255u);
      word[j] = (i0 + j < n) ? (w[j] | b << 16) : 0u;
      if (need[j]) {
        word[j] = GPX_PO_EXC_BIT | (uint32_t)r;
        rows[2 * (int64_t)r] = KIND == GPX_PO_DECISIONS ? make_int4(v[j][2], v[j][3], v[j][1], v[j][4])
                                                        : make_int4(v[j][1], v[j][2], v[j][3], v[j][4]);
        rows[2 * (int64_t)r + 1] = make_int4(v[j][5], 0, 0, 0);
        r++;
      }
    }
    if (KIND == GPX_PO_DECISIONS) { /* 32 bytes per lane: the area ends with the last lane's */
      uint4* rec = (uint4*)(out + 32) + 2 * (int64_t)t;
      rec[0] = make_uint4((uint32_t)v[0][0], word[0], (uint32_t)v[1][0], word[1]);
      rec[1] = make_uint4((uint32_t)v[2][0], word[2], (uint32_t)v[3][0], word[3]);
    } else {
      ((uint4*)(out + 32))[t] = make_uint4(word[0], word[1], word[2], word[3]);
      if (last) po_zero_to(out + 32, 16 * ((int64_t)t + 1), S4);
    }
  } else {
#pragma unroll
    for (int k = 0; k < NC; k++) {
      const int c = KIND == GPX_PO_DECISIONS ? k : k + 1; /* proposals have no gidx column */
      uint8_t* col = out + 32 + k * S4;
      ((int4*)col)[t] = make_int4(v[0][c], v[1][c], v[2][c], v[3][c]);
      if (last) po_zero_to(col, 16 * ((int64_t)t + 1), S4);
    }
    uint8_t* bcol = out + 32 + NC * S4;
    ((uint32_t*)bcol)[t] = (uint32_t)v[0][5] | (uint32_t)v[1][5] << 8 | (uint32_t)v[2][5] << 16 | (uint32_t)v[3][5] << 24;
    if (last) po_zero_to(bcol, 4 * ((int64_t)t + 1), ((int64_t)n + 31) & ~(int64_t)31);
  }
}
/* workgroups of a pack launch over up to `cap` entries */
inline int po_grid(int32_t cap) { return cap > 0 ? (int)(((int64_t)cap + GPX_PO_QUAD - 1) / GPX_PO_QUAD) : 1; }

/* The staged buffer through the caller's host mapping: the length comes from the staged header, on the device, so
 * exactly gpx_packed_out_size bytes cross the link without a host round trip (as k_copy_out does with the count);
 * 16 bytes per lane.  Every area of the format is a multiple of 32 bytes, so there is no tail. */
__global__ __launch_bounds__(256) void k_po_copy_out(const uint4* __restrict__ stage, uint4* __restrict__ dst,
                                                     int64_t dst_bytes) {
  const int4 h = *(const int4*)stage;
  int64_t sz = po_size(h.x, h.y, h.z, h.w);
  sz = sz < 32 ? 32 : sz;
  sz = sz > dst_bytes ? (dst_bytes & ~(int64_t)15) : sz;
  const int64_t nv = sz >> 4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) dst[i] = stage[i];
}

/* ---- host helpers (no device call) ------------------------------------------------------------------------ */
inline PoRef po_reference_host(int32_t n, const int32_t* bnum, const int32_t* bcoord, const int32_t* slot,
                               const int32_t* cp) {
  const int32_t m = std::min<int32_t>(n, GPX_PO_REF_WINDOW);
  int32_t best = -1, best_cnt = 0;
  for (int32_t i = 0; i < m; i++) {
    bool first = true;
    for (int32_t j = 0; j < i && first; j++) first = !(bnum[j] == bnum[i] && bcoord[j] == bcoord[i]);
    if (!first) continue;
    int32_t cnt = 0;
    for (int32_t j = i; j < m; j++) cnt += bnum[j] == bnum[i] && bcoord[j] == bcoord[i];
    if (cnt > best_cnt) best = i, best_cnt = cnt;
  }
  if (best < 0) return PoRef{0, 0, 0u, 0u};
  return PoRef{bnum[best], bcoord[best], (uint32_t)slot[best] - 128u, (uint32_t)cp[best] - 128u};
}

template <int KIND>
int po_pack_host(int32_t n, const int32_t* gidx, const int32_t* slot, const int32_t* bnum, const int32_t* bcoord,
                 const int32_t* cp, const uint8_t* b, void* out, size_t out_bytes) {
  constexpr bool DEC = KIND == GPX_PO_DECISIONS;
  if (n < 0 || !out) return GPX_EINVAL;
  if (n > 0 && (!slot || !bnum || !bcoord || !cp || !b || (DEC && !gidx))) return GPX_EINVAL;
  if (out_bytes < GPX_PACKED_OUT_BYTES(n)) return GPX_ECAPACITY;
  if (DEC)
    for (int32_t i = 0; i < n; i++)
      if (b[i] > 3) return GPX_EINVAL;
  const PoRef R = po_reference_host(n, bnum, bcoord, slot, cp);
  int64_t need = 0;
  uint32_t w;
  for (int32_t i = 0; i < n; i++) need += !po_fits(R, bnum[i], bcoord[i], slot[i], cp[i], w);
  const bool records = need <= n / GPX_PO_EXC_DIV;
  gpx_packed_out_hdr H{records ? GPX_PO_RECORDS : GPX_PO_COLUMNS, KIND, n, records ? (int32_t)need : 0, R.bnum, R.bcoord,
                       (int32_t)R.base_slot, (int32_t)R.base_cp};
  uint8_t* o = (uint8_t*)out;
  const size_t used = (size_t)po_size(H.form, H.kind, H.n, H.n_exc);
  memset(o, 0, used);
  memcpy(o, &H, sizeof(H));
  const size_t S4 = GPX_PO_R(4 * (size_t)n);
  if (records) {
    uint8_t* rec = o + 32;
    uint8_t* rows = o + 32 + (DEC ? GPX_PO_R(8 * (size_t)n) : S4);
    int32_t r = 0;
    for (int32_t i = 0; i < n; i++) {
      uint32_t word;
      if (po_fits(R, bnum[i], bcoord[i], slot[i], cp[i], word)) {
        word |= (uint32_t)b[i] << 16;
      } else {
        word = GPX_PO_EXC_BIT | (uint32_t)r;
        const int32_t row[8] = {DEC ? bnum[i] : slot[i], DEC ? bcoord[i] : bnum[i], DEC ? slot[i] : bcoord[i], cp[i],
                                (int32_t)b[i], 0, 0, 0};
        memcpy(rows + 32 * (size_t)r, row, 32);
        r++;
      }
      if (DEC) {
        const uint32_t pair[2] = {(uint32_t)gidx[i], word};
        memcpy(rec + 8 * (size_t)i, pair, 8);
      } else {
        memcpy(rec + 4 * (size_t)i, &word, 4);
      }
    }
  } else {
    const int32_t* cols[5] = {gidx, slot, bnum, bcoord, cp};
    constexpr int NC = DEC ? 5 : 4;
    for (int k = 0; k < NC; k++) memcpy(o + 32 + k * S4, cols[DEC ? k : k + 1], 4 * (size_t)n);
    memcpy(o + 32 + NC * S4, b, (size_t)n);
  }
  return (int)need;
}

template <int KIND>
int po_unpack_host(const void* buf, size_t bytes, int32_t cap, int32_t* gidx, int32_t* slot, int32_t* bnum,
                   int32_t* bcoord, int32_t* cp, uint8_t* b, int32_t* n_out) {
  constexpr bool DEC = KIND == GPX_PO_DECISIONS;
  if (!buf || !n_out || cap < 0 || bytes < sizeof(gpx_packed_out_hdr)) return GPX_EINVAL;
  gpx_packed_out_hdr H;
  memcpy(&H, buf, sizeof(H));
  if (H.kind != KIND) return GPX_EINVAL;
  const int64_t used = po_size(H.form, H.kind, H.n, H.n_exc);
  if (used < 0 || (uint64_t)used > bytes) return GPX_EINVAL;
  const int32_t n = H.n;
  if (n > cap) return GPX_ECAPACITY;
  if (n > 0 && (!slot || !bnum || !bcoord || !cp || !b || (DEC && !gidx))) return GPX_EINVAL;
  const uint8_t* o = (const uint8_t*)buf;
  const size_t S4 = GPX_PO_R(4 * (size_t)n);
  if (H.form == GPX_PO_COLUMNS) {
    int32_t* cols[5] = {gidx, slot, bnum, bcoord, cp};
    constexpr int NC = DEC ? 5 : 4;
    for (int k = 0; k < NC; k++) memcpy(cols[DEC ? k : k + 1], o + 32 + k * S4, 4 * (size_t)n);
    memcpy(b, o + 32 + NC * S4, (size_t)n);
    *n_out = n;
    return GPX_OK;
  }
  const uint8_t* rec = o + 32;
  const uint8_t* rows = o + 32 + (DEC ? GPX_PO_R(8 * (size_t)n) : S4);
  auto word_of = [&](int32_t i) {
    uint32_t w;
    memcpy(&w, rec + (DEC ? 8 * (size_t)i + 4 : 4 * (size_t)i), 4);
    return w;
  };
  for (int32_t i = 0; i < n; i++) { /* the whole buffer first */
    const uint32_t w = word_of(i);
    if (w & GPX_PO_EXC_BIT) {
      if ((w & ~GPX_PO_EXC_BIT) >= (uint32_t)H.n_exc) return GPX_EINVAL;
    } else if (w & (DEC ? GPX_PO_DEC_RESERVED : GPX_PO_PROP_RESERVED)) {
      return GPX_EINVAL;
    }
  }
  const PoRef R{H.bnum, H.bcoord, (uint32_t)H.base_slot, (uint32_t)H.base_cp};
  for (int32_t i = 0; i < n; i++) {
    const uint32_t w = word_of(i);
    if (DEC) memcpy(&gidx[i], rec + 8 * (size_t)i, 4);
    if (w & GPX_PO_EXC_BIT) {
      int32_t row[8];
      memcpy(row, rows + 32 * (size_t)(w & ~GPX_PO_EXC_BIT), 32);
      bnum[i] = DEC ? row[0] : row[1], bcoord[i] = DEC ? row[1] : row[2], slot[i] = DEC ? row[2] : row[0];
      cp[i] = row[3], b[i] = (uint8_t)row[4];
    } else {
      bnum[i] = R.bnum, bcoord[i] = R.bcoord;
      po_delta(R, w, slot[i], cp[i], b[i]);
    }
  }
  *n_out = n;
  return GPX_OK;
}

extern "C" {

int64_t gpx_packed_out_size(const void* buf) {
  if (!buf) return GPX_EINVAL;
  gpx_packed_out_hdr H;
  memcpy(&H, buf, sizeof(H));
  const int64_t s = po_size(H.form, H.kind, H.n, H.n_exc);
  return s < 0 ? GPX_EINVAL : s;
}

int gpx_decisions_pack(int32_t n, const int32_t* d_gidx, const int32_t* d_slot, const int32_t* d_bnum,
                       const int32_t* d_bcoord, const int32_t* d_median_cp, const uint8_t* d_kind, void* out,
                       size_t out_bytes) {
  return po_pack_host<GPX_PO_DECISIONS>(n, d_gidx, d_slot, d_bnum, d_bcoord, d_median_cp, d_kind, out, out_bytes);
}
int gpx_proposals_pack(int32_t n, const int32_t* slot, const int32_t* bnum, const int32_t* bcoord,
                       const int32_t* median_cp, const uint8_t* status, void* out, size_t out_bytes) {
  return po_pack_host<GPX_PO_PROPOSALS>(n, nullptr, slot, bnum, bcoord, median_cp, status, out, out_bytes);
}
int gpx_decisions_unpack(const void* buf, size_t bytes, int32_t cap, int32_t* d_gidx, int32_t* d_slot,
                         int32_t* d_bnum, int32_t* d_bcoord, int32_t* d_median_cp, uint8_t* d_kind, int32_t* n_out) {
  return po_unpack_host<GPX_PO_DECISIONS>(buf, bytes, cap, d_gidx, d_slot, d_bnum, d_bcoord, d_median_cp, d_kind, n_out);
}
int gpx_proposals_unpack(const void* buf, size_t bytes, int32_t cap, int32_t* slot, int32_t* bnum, int32_t* bcoord,
                         int32_t* median_cp, uint8_t* status, int32_t* n_out) {
  return po_unpack_host<GPX_PO_PROPOSALS>(buf, bytes, cap, nullptr, slot, bnum, bcoord, median_cp, status, n_out);
}

} /* extern "C" */
