/*
 * gpx_packed.hip.h — accept-reply votes as packed 8-byte records (include/gpx_packed.h): the reading of one record
 * (host and device share it), the streaming kernel that turns a packed batch into the six int32 columns every
 * accept-reply path takes, and the host-side packer.
 *
 * k_votes_unpack moves 8 bytes in and 24 out per vote; a lane takes four consecutive records (two 16-byte loads) and
 * stores each column 16 bytes at a time, so a wave reads 2 KB of records and writes 1 KB per column.  Exception rows
 * (at most one vote in four, usually under 1 %: include/gpx_packed.h) are gathered by the lanes that hold them, 32
 * bytes as two 16-byte loads; nothing branches around the stores.
 */
#pragma once
#include "../../include/gpx_packed.h"
#include "gpx_kernels.hip.h"

/* the header fields of a gpx_packed_votes the kernel needs, by value */
struct PackedHdr {
  int32_t n, n_exc, bnum, bcoord;
  uint32_t base_slot, base_cp, base_acc;
};
inline PackedHdr packed_hdr(const gpx_packed_votes& pv) {
  return PackedHdr{pv.n, pv.n_exc, pv.bnum, pv.bcoord, (uint32_t)pv.base_slot, (uint32_t)pv.base_cp,
                   (uint32_t)pv.base_acceptor};
}

/* One record -> v = (gidx, bnum, bcoord, slot, acceptor, max_cp): THE definition of include/gpx_packed.h. */
__host__ __device__ __forceinline__ void packed_vote(const PackedHdr& H, const int32_t* __restrict__ exc, uint32_t g,
                                                     uint32_t w, int32_t (&v)[6]) {
  /* a delta record: selects, no branch (a reserved bit makes it malformed) */
  const bool ok = (w & GPX_PACKED_RESERVED) == 0;
  v[0] = ok ? (int32_t)g : -1;
  v[1] = ok ? H.bnum : 0;
  v[2] = ok ? H.bcoord : 0;
  v[3] = ok ? (int32_t)(H.base_slot + (w & 255u)) : 0;
  v[4] = ok ? (int32_t)(H.base_acc + ((w >> 16) & 255u)) : 0;
  v[5] = ok ? (int32_t)(H.base_cp + ((w >> 8) & 255u)) : 0;
  if (w & GPX_PACKED_EXC_BIT) {
    const uint32_t r = w & ~GPX_PACKED_EXC_BIT;
    if (r < (uint32_t)H.n_exc) {
#ifdef __HIP_DEVICE_COMPILE__
      const int4 a = ((const int4*)exc)[2 * (size_t)r], b = ((const int4*)exc)[2 * (size_t)r + 1];
      v[0] = (int32_t)g, v[1] = a.x, v[2] = a.y, v[3] = a.z, v[4] = a.w, v[5] = b.x;
#else /* host rows may sit at any 4-byte alignment */
      const int32_t* row = exc + 8 * (size_t)r;
      v[0] = (int32_t)g, v[1] = row[0], v[2] = row[1], v[3] = row[2], v[4] = row[3], v[5] = row[4];
#endif
    } else {
      v[0] = -1, v[1] = v[2] = v[3] = v[4] = v[5] = 0;
    }
  }
}

/* lanes [0, n / 4): four records each, 16-byte loads and stores (rec, exc and the columns 16-byte aligned);
 * lanes [n / 4, n / 4 + n % 4): one record of the tail each */
__global__ __launch_bounds__(GPX_BLOCK) void k_votes_unpack(PackedHdr H, const uint4* __restrict__ rec,
                                                           const int32_t* __restrict__ exc, int4* __restrict__ gidx,
                                                           int4* __restrict__ bnum, int4* __restrict__ bcoord,
                                                           int4* __restrict__ slot, int4* __restrict__ acceptor,
                                                           int4* __restrict__ max_cp) {
  const int32_t t = blockIdx.x * GPX_BLOCK + threadIdx.x;
  const int32_t n4 = H.n >> 2;
  if (t < n4) {
    const uint4 p = rec[2 * (size_t)t], q = rec[2 * (size_t)t + 1];
    int32_t v[4][6];
    packed_vote(H, exc, p.x, p.y, v[0]);
    packed_vote(H, exc, p.z, p.w, v[1]);
    packed_vote(H, exc, q.x, q.y, v[2]);
    packed_vote(H, exc, q.z, q.w, v[3]);
    gidx[t] = make_int4(v[0][0], v[1][0], v[2][0], v[3][0]);
    bnum[t] = make_int4(v[0][1], v[1][1], v[2][1], v[3][1]);
    bcoord[t] = make_int4(v[0][2], v[1][2], v[2][2], v[3][2]);
    slot[t] = make_int4(v[0][3], v[1][3], v[2][3], v[3][3]);
    acceptor[t] = make_int4(v[0][4], v[1][4], v[2][4], v[3][4]);
    max_cp[t] = make_int4(v[0][5], v[1][5], v[2][5], v[3][5]);
  } else if (t < n4 + (H.n & 3)) {
    const size_t i = 4 * (size_t)n4 + (size_t)(t - n4);
    const uint32_t* r32 = (const uint32_t*)rec;
    int32_t v[6];
    packed_vote(H, exc, r32[2 * i], r32[2 * i + 1], v);
    ((int32_t*)gidx)[i] = v[0];
    ((int32_t*)bnum)[i] = v[1];
    ((int32_t*)bcoord)[i] = v[2];
    ((int32_t*)slot)[i] = v[3];
    ((int32_t*)acceptor)[i] = v[4];
    ((int32_t*)max_cp)[i] = v[5];
  }
}
/* lanes of a k_votes_unpack launch over n >= 1 votes */
inline int64_t votes_unpack_lanes(int32_t n) { return (int64_t)(n >> 2) + (n & 3); }

/* ---- host helpers (no device call) ------------------------------------------------------------------------ */
extern "C" {

int gpx_votes_pack(int32_t n, const int32_t* gidx, const int32_t* bnum, const int32_t* bcoord, const int32_t* slot,
                   const int32_t* acceptor, const int32_t* max_cp, uint32_t* rec_out, int32_t* exc_out,
                   int32_t exc_cap, gpx_packed_votes* out) {
  if (n < 0 || exc_cap < 0 || !out || (exc_cap > 0 && !exc_out)) return GPX_EINVAL;
  if (n > 0 && (!gidx || !bnum || !bcoord || !slot || !acceptor || !max_cp || !rec_out)) return GPX_EINVAL;
  /* Boyer-Moore majority candidate of the ballots */
  int32_t cb = 0, cc = 0;
  int64_t cnt = 0;
  for (int32_t i = 0; i < n; i++) {
    if (cnt == 0)
      cb = bnum[i], cc = bcoord[i], cnt = 1;
    else
      cnt += (bnum[i] == cb && bcoord[i] == cc) ? 1 : -1;
  }
  uint32_t bs = 0, bp = 0, ba = 0;
  for (int32_t i = 0; i < n; i++)
    if (bnum[i] == cb && bcoord[i] == cc) {
      bs = (uint32_t)slot[i] - 128u, bp = (uint32_t)max_cp[i] - 128u, ba = (uint32_t)acceptor[i] - 128u;
      break;
    }
  int64_t need = 0;
  for (int32_t i = 0; i < n; i++) {
    const uint32_t ds = (uint32_t)slot[i] - bs, dp = (uint32_t)max_cp[i] - bp, da = (uint32_t)acceptor[i] - ba;
    rec_out[2 * (size_t)i] = (uint32_t)gidx[i];
    if (bnum[i] == cb && bcoord[i] == cc && ds < 256u && dp < 256u && da < 256u) {
      rec_out[2 * (size_t)i + 1] = ds | dp << 8 | da << 16;
    } else {
      rec_out[2 * (size_t)i + 1] = GPX_PACKED_EXC_BIT | (uint32_t)need;
      if (need < exc_cap) {
        int32_t* row = exc_out + 8 * (size_t)need;
        row[0] = bnum[i], row[1] = bcoord[i], row[2] = slot[i], row[3] = acceptor[i], row[4] = max_cp[i];
        row[5] = row[6] = row[7] = 0;
      }
      need++;
    }
  }
  out->n = n;
  out->n_exc = (int32_t)std::min<int64_t>(need, exc_cap);
  out->bnum = cb, out->bcoord = cc;
  out->base_slot = (int32_t)bs, out->base_cp = (int32_t)bp, out->base_acceptor = (int32_t)ba;
  out->reserved = 0;
  out->rec = rec_out;
  out->exc = exc_out;
  return (int)need;
}

int gpx_votes_unpack(const gpx_packed_votes* pv, int32_t* gidx, int32_t* bnum, int32_t* bcoord, int32_t* slot,
                     int32_t* acceptor, int32_t* max_cp) {
  if (!pv || pv->n < 0 || pv->n_exc < 0 || (pv->n_exc > 0 && !pv->exc)) return GPX_EINVAL;
  if (pv->n > 0 && (!pv->rec || !gidx || !bnum || !bcoord || !slot || !acceptor || !max_cp)) return GPX_EINVAL;
  const PackedHdr H = packed_hdr(*pv);
  for (int32_t i = 0; i < pv->n; i++) {
    int32_t v[6];
    packed_vote(H, pv->exc, pv->rec[2 * (size_t)i], pv->rec[2 * (size_t)i + 1], v);
    gidx[i] = v[0], bnum[i] = v[1], bcoord[i] = v[2], slot[i] = v[3], acceptor[i] = v[4], max_cp[i] = v[5];
  }
  return GPX_OK;
}

} /* extern "C" */
