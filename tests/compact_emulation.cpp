// Lockstep CPU emulation of the tile-compaction core, gigapaxos_amd/csrc/gpx_compact.hip.h (tests/test_scan_hits_abi.py
// compiles and runs this with AddressSanitizer and UBSan): the real header, unmodified, over tests/lockstep_runtime.h,
// each piece against a plain loop.  Every buffer is a heap block of its exact size.  What the six families build from
// these pieces is in their own emulations (tests/{scan,sweep,timers,checkpoint,delta}_emulation.cpp).
#include <cstdio>
#include <utility>

#include "lockstep_runtime.h"

#include "gpx_compact.hip.h"

static void fail(const char* what, long a, long b, long c) {
  printf("%s: (%ld, %ld, %ld)\n", what, a, b, c);
  exit(1);
}
static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { return (g_rng = g_rng * 1664525u + 1013904223u) >> 8; }

// ---- tile_count: a tile kernel's passes over n entries whose N predicates are the low bits of bits[i] ----
template <int N>
static void k_count(int32_t n, const uint8_t* bits, int32_t* before, int32_t* total) {
  __shared__ int32_t w[2][N][GPX_COMPACT_WAVES]; /* two sets, used alternately, as the 1,024-entry tiles do */
  for (int32_t pass = 0; pass * GPX_BLOCK < n; pass++) {
    const int32_t i = pass * GPX_BLOCK + (int32_t)threadIdx.x;
    bool p[N];
    for (int k = 0; k < N; k++) p[k] = i < n && ((bits[i] >> k) & 1);
    const TileCount<N> c = tile_count(w[pass & 1], p);
    for (int k = 0; k < N; k++) {
      if (i < n) before[(size_t)i * N + k] = c.before[k];
      if (threadIdx.x == 7) total[pass * N + k] = c.total[k];
    }
  }
}
template <int N>
static void count_case(int32_t n) {
  const int32_t passes = (n + GPX_BLOCK - 1) / GPX_BLOCK;
  uint8_t* bits = blk<uint8_t>(n, 0);
  int32_t *before = blk<int32_t>((size_t)n * N, 0xA5), *total = blk<int32_t>(passes * N, 0xA5);
  for (int32_t i = 0; i < n; i++) bits[i] = (uint8_t)(i % 64 == 63 || i % 64 == 0 ? 0xF : rnd() % 5 ? rnd() & 0xF : 0);
  launch(1, [&] { k_count<N>(n, bits, before, total); });
  for (int32_t pass = 0; pass < passes; pass++)
    for (int k = 0; k < N; k++) {
      int32_t seen = 0;
      for (int32_t i = pass * GPX_BLOCK; i < std::min(n, (pass + 1) * GPX_BLOCK); i++) {
        if (before[(size_t)i * N + k] != seen) fail("tile_count: before", i, k, before[(size_t)i * N + k]);
        seen += (bits[i] >> k) & 1;
      }
      if (total[pass * N + k] != seen) fail("tile_count: total", pass, k, total[pass * N + k]);
    }
  free(bits), free(before), free(total);
}

// ---- tile_offsets: NP prefixed and NS summed words per tile; every lane reports the sums it got ----
template <int NP, int NS>
static void k_offsets(int32_t ntiles, const int32_t* cnt, int32_t* off, int32_t* sums) {
  int32_t sum[NP + NS];
  tile_offsets<NP, NS>(
      ntiles,
      [&](int32_t t, int32_t(&v)[NP + NS]) {
        for (int k = 0; k < NP + NS; k++) v[k] = cnt[(size_t)t * (NP + NS) + k];
      },
      [&](int32_t t, const int32_t(&o)[NP], const int32_t(&v)[NP + NS]) {
        for (int k = 0; k < NP; k++) off[(size_t)t * NP + k] = o[k];
        if (v[NP + NS - 1] != cnt[(size_t)t * (NP + NS) + NP + NS - 1]) fail("tile_offsets: the words handed to store", t, 0, 0);
      },
      sum);
  for (int k = 0; k < NP + NS; k++) sums[threadIdx.x * (NP + NS) + k] = sum[k];
}
template <int NP, int NS>
static void offsets_case() {
  const int NW = NP + NS, NT = 6;
  const int32_t ntiles[NT] = {0, 1, 255, 256, 257, 600};
  int32_t *cnt[NT], *off[NT], *sums[NT];
  for (int c = 0; c < NT; c++) {
    cnt[c] = blk<int32_t>((size_t)ntiles[c] * NW, 0), off[c] = blk<int32_t>((size_t)ntiles[c] * NP, 0xA5);
    sums[c] = blk<int32_t>(GPX_BLOCK * NW, 0xA5);
    for (int32_t q = 0; q < ntiles[c] * NW; q++) cnt[c][q] = rnd() % 3 ? (int32_t)(rnd() % 1025) : 0;
  }
  launch(1, [&] { /* one workgroup, the six calls one after the other over the same LDS */
    for (int c = 0; c < NT; c++) k_offsets<NP, NS>(ntiles[c], cnt[c], off[c], sums[c]);
  });
  for (int c = 0; c < NT; c++) {
    int32_t run[NW] = {};
    for (int32_t t = 0; t < ntiles[c]; t++)
      for (int k = 0; k < NW; k++) {
        if (k < NP && off[c][(size_t)t * NP + k] != run[k]) fail("tile_offsets: prefix", ntiles[c], t, k);
        run[k] += cnt[c][(size_t)t * NW + k];
      }
    for (int32_t l = 0; l < GPX_BLOCK; l++)
      for (int k = 0; k < NW; k++)
        if (sums[c][l * NW + k] != run[k]) fail("tile_offsets: sum", ntiles[c], l, k);
    free(cnt[c]), free(off[c]), free(sums[c]);
  }
}
template <int... I>
static void all_offsets(std::integer_sequence<int, I...>) {
  (offsets_case<I / 4 + 1, I % 4>(), ...); /* 1 to 3 prefixed, 0 to 3 summed */
}

// ---- cap_cut: a tile of c entries of weight 1 or 2 whose rows begin at off, cap at every position ----
static void cut_case(int32_t c, int32_t off) {
  int32_t* w = blk<int32_t>(c, 0);
  int32_t rows = 0;
  for (int32_t j = 0; j < c; j++) rows += w[j] = 1 + (j % 3 == 1 || rnd() % 4 == 0);
  const int32_t lo = off - 2, ncap = rows + 5; /* below the first row .. past the last: every middle of a two-row entry */
  CapCut* got = blk<CapCut>((size_t)ncap * GPX_BLOCK, 0xA5);
  launch(1, [&] {
    const int32_t j = (int32_t)threadIdx.x;
    for (int32_t q = 0; q < ncap; q++) got[(size_t)q * GPX_BLOCK + j] = cap_cut(off, j < c ? w[j] : 0, lo + q);
  });
  for (int32_t q = 0; q < ncap; q++) {
    int32_t n = 0, r = 0;
    while (n < c && off + r + w[n] <= lo + q) r += w[n++];
    for (int32_t l = 0; l < GPX_BLOCK; l++)
      if (got[(size_t)q * GPX_BLOCK + l].n != n || got[(size_t)q * GPX_BLOCK + l].rows != r) fail("cap_cut", lo + q, l, n);
  }
  free(w), free(got);
}

int main() {
  for (int32_t n : {5, 2 * GPX_BLOCK, 3 * GPX_BLOCK + 77, 4 * GPX_BLOCK - 1}) count_case<2>(n), count_case<4>(n);
  printf("tile_count: ok\n");
  all_offsets(std::make_integer_sequence<int, 12>{});
  printf("tile_offsets: ok\n");
  cut_case(66, 1000), cut_case(1, 0); /* entries in two waves; a tile of one entry */
  printf("cap_cut: ok\n");
  return 0;
}
