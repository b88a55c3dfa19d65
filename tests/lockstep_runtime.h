// The stand-in runtime of the lockstep CPU emulations (tests/*_emulation.cpp): what a kernel header of
// gigapaxos_amd/csrc takes from HIP and, of gpx_kernels.hip.h, the two scans - the same names, the same meaning.  One
// std::thread per lane of a workgroup of GPX_BLOCK = 256 lanes, a std::barrier for __syncthreads and one per wave for
// the wave collectives, one workgroup at a time, so a `__shared__` array (a static) is that workgroup's LDS.  Every
// lane of a workgroup (wave) has to reach a block (wave) collective, as on the device.  An emulation includes this
// first, then its fake engine side, then the real headers, unmodified.
#pragma once
#include <algorithm>
#include <barrier>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
#define __restrict__
#define GPX_BLOCK 256
struct Dim3 { unsigned x, y, z; };
static thread_local Dim3 threadIdx, blockIdx, gridDim;
static std::barrier<>* g_block_bar;
static std::barrier<>* g_wave_bar[GPX_BLOCK / 64];
static long long g_wave_val[GPX_BLOCK / 64][64];
static int g_block_val[GPX_BLOCK];
using std::max;
using std::min;

static void __syncthreads() { g_block_bar->arrive_and_wait(); }
static int __syncthreads_count(bool p) {
  g_block_val[threadIdx.x] = p;
  g_block_bar->arrive_and_wait();
  int c = 0;
  for (int q = 0; q < GPX_BLOCK; q++) c += g_block_val[q];
  g_block_bar->arrive_and_wait();
  return c;
}
static int __syncthreads_or(bool p) { return __syncthreads_count(p) != 0; }
static unsigned long long __ballot(bool p) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  g_wave_val[w][l] = p;
  g_wave_bar[w]->arrive_and_wait();
  unsigned long long m = 0;
  for (int q = 0; q < 64; q++) m |= (unsigned long long)(g_wave_val[w][q] != 0) << q;
  g_wave_bar[w]->arrive_and_wait();
  return m;
}
template <class T> static T shfl_from(T v, int src_lane, bool valid) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  g_wave_val[w][l] = (long long)v;
  g_wave_bar[w]->arrive_and_wait();
  const T r = valid ? (T)g_wave_val[w][src_lane] : v;
  g_wave_bar[w]->arrive_and_wait();
  return r;
}
template <class T> static T __shfl_up(T v, int d) { const int l = threadIdx.x & 63; return shfl_from(v, l - d, l - d >= 0); }
template <class T> static T __shfl_xor(T v, int d) { const int l = threadIdx.x & 63; return shfl_from(v, l ^ d, true); }
static uint32_t __builtin_amdgcn_mbcnt_lo(uint32_t m, uint32_t acc) {
  const int l = threadIdx.x & 63;
  return acc + __builtin_popcount(l >= 32 ? m : (m & ((1u << l) - 1u)));
}
static uint32_t __builtin_amdgcn_mbcnt_hi(uint32_t m, uint32_t acc) {
  const int l = threadIdx.x & 63;
  return acc + (l <= 32 ? 0 : __builtin_popcount(m & ((1u << (l - 32)) - 1u)));
}
static int __popcll(unsigned long long m) { return __builtin_popcountll(m); }
static int32_t atomicAdd(int32_t* p, int32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }

/* gpx_kernels.hip.h's scans */
static int32_t wave_incscan(int32_t v) {
  const int l = threadIdx.x & 63;
  int32_t x = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t y = __shfl_up(x, d);
    if (l >= d) x += y;
  }
  return x;
}
static int32_t block_exscan(int32_t v, int32_t* total) {
  static int32_t wsum[GPX_BLOCK / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int32_t x = wave_incscan(v);
  if (lane == 63) wsum[wid] = x;
  __syncthreads();
  int32_t base = 0, tot = 0;
  for (int w = 0; w < GPX_BLOCK / 64; w++) {
    if (w < wid) base += wsum[w];
    tot += wsum[w];
  }
  __syncthreads();
  *total = tot;
  return base + x - v;
}

/* body() once per lane of each of `grid` workgroups */
template <class F>
static void launch(int grid, F body) {
  std::barrier<> bb(GPX_BLOCK), w0(64), w1(64), w2(64), w3(64);
  g_block_bar = &bb;
  g_wave_bar[0] = &w0, g_wave_bar[1] = &w1, g_wave_bar[2] = &w2, g_wave_bar[3] = &w3;
  std::vector<std::thread> th;
  for (int t = 0; t < GPX_BLOCK; t++)
    th.emplace_back([=] {
      for (int b = 0; b < grid; b++) { /* one workgroup at a time: the static arrays are its LDS */
        threadIdx = Dim3{(unsigned)t, 0, 0};
        blockIdx = Dim3{(unsigned)b, 0, 0};
        gridDim = Dim3{(unsigned)grid, 1, 1};
        body();
        g_block_bar->arrive_and_wait();
      }
    });
  for (auto& x : th) x.join();
}

// exact-size heap blocks: AddressSanitizer sees every index past an end
template <class T> static T* blk(size_t n, int fill) {
  T* p = (T*)malloc(std::max<size_t>(n, 1) * sizeof(T));
  memset(p, fill, std::max<size_t>(n, 1) * sizeof(T));
  return p;
}
