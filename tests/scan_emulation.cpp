// Lockstep CPU emulation of the compaction kernels of gigapaxos_amd/csrc/gpx_scan.hip.h (tests/test_scan_hits_abi.py
// compiles and runs this with AddressSanitizer): the real header, unmodified, over a stand-in for the per-group
// evaluation.  One std::thread per lane of a workgroup, barriers for __syncthreads and for the wave collectives, one
// workgroup at a time.  The scratch block starts as garbage and every call runs twice over it; every buffer is a heap
// block of its exact size, so an index past an end is a sanitizer report.  What this cannot show is what only the GPU
// has: the compiler's code, memory ordering between launches, and the real evaluation (tests/test_scan_hits_gpu.py).
#include <algorithm>
#include <barrier>
#include <cassert>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "lockstep_runtime.h"

// ---- the fake engine side ----
#define GPX_S_OK 0
#define GPX_S_NOGROUP 1
#define GPX_S_STOPPED 2
#define GPX_RUN_NO 0
#define GPX_POKE_NONE 0
#define GPX_GAP_HIT_SYNC 1
#define GPX_GAP_HIT_MISSING 2
#define GPX_GAP_HIT_AHEAD 4
#define GPX_MAX_NODE_LIST 16
struct NodeLists { int32_t n_down, n_long, down[16], longdead[16]; };
struct DevState { int32_t G; const uint8_t* hit; };
static int32_t jsub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
struct ElectionRow { int32_t run, p_bnum, p_first, status; };
static ElectionRow election_scan_row(const DevState& S, int32_t g, const NodeLists&, int32_t) {
  if ((uint32_t)g >= (uint32_t)S.G) return ElectionRow{0, 0, 0, GPX_S_NOGROUP};
  return S.hit[g] ? ElectionRow{1 + g % 4, g * 3, g * 5 + 1, GPX_S_OK} : ElectionRow{0, 0, 0, GPX_S_OK};
}
struct PokeRow { uint8_t poke, flags, status; int32_t slot, bnum, bcoord, median_cp; uint32_t heard; };
template <int K> static PokeRow poke_scan_row(const DevState& S, int32_t g) {
  if ((uint32_t)g >= (uint32_t)S.G) return PokeRow{0, 0, GPX_S_NOGROUP, 0, 0, 0, 0, 0};
  if (!S.hit[g]) return PokeRow{0, 0, GPX_S_OK, 0, 0, 0, 0, 0};
  return PokeRow{(uint8_t)(1 + g % 2), (uint8_t)(g % 3 == 0), GPX_S_OK, g + 1, g + 2, g + 3, g + 4, (uint32_t)g * 7u};
}
struct GapRow { int32_t first_slot, max_committed; unsigned long long missing; int32_t should_sync, status; };
static GapRow gap_scan_row(const DevState& S, int32_t g, int32_t, int32_t, int32_t) {
  if ((uint32_t)g >= (uint32_t)S.G) return GapRow{0, 0, 0, 0, GPX_S_NOGROUP};
  if (!S.hit[g]) return GapRow{g, g - 1, 0, 0, GPX_S_OK};
  return GapRow{g, g + 2, 0x8000000000000003ull + (unsigned long long)g, 1, g % 11 == 5 ? GPX_S_STOPPED : GPX_S_OK};
}
static uint8_t election_begin_group(const DevState&, int32_t g, int32_t b) { return (uint8_t)((g + b) & 3); }

#include "gpx_compact.hip.h"
#include "gpx_scan.hip.h"


template <class E, class Check>
static void run(const char* what, int32_t G, int32_t n, const int32_t* gidx, const std::vector<uint8_t>& hit, E ev, int32_t cap,
                size_t scan_cap_entries, Check check) {
  const size_t tiles_cap = scan_cap_entries / GPX_SCAN_TILE_;
  const size_t tl = (tiles_cap * 4 + 255) & ~(size_t)255;
  const size_t bytes = 26 * scan_cap_entries + 3 * tl + 256;
  char* base = blk<char>(bytes, 0xEE); /* garbage: a call may read only what it wrote */
  ScanScratch X{base, (uint32_t)scan_cap_entries, (uint32_t)tl};
  ScanCounts* counts = (ScanCounts*)(base + 26 * scan_cap_entries + 3 * tl);
  DevState S{G, hit.data()};
  ScanOut O{};
  for (int q = 0; q < 6; q++) O.i32[q] = blk<int32_t>(cap, 0xA5);
  for (int q = 0; q < 2; q++) O.u8[q] = blk<uint8_t>(cap, 0xA5);
  O.u64 = blk<unsigned long long>(cap, 0xA5);
  const int ntiles = (n + GPX_SCAN_TILE_ - 1) / GPX_SCAN_TILE_;
  for (int round = 0; round < (ntiles <= 4 ? 2 : 1); round++) { /* the small calls twice over the same scratch */
    launch(ntiles, [&] { k_scan_tile<E>(S, n, gidx, ev, X); });
    launch(1, [&] { k_scan_offsets(ntiles, X, counts); });
    if (cap > 0) launch(ntiles, [&] { k_scan_move<E>(X, O, cap); });
  }
  // the expected answer
  std::vector<int32_t> idx;
  int32_t nog = 0;
  for (int32_t i = 0; i < n; i++) {
    const int32_t g = gidx ? gidx[i] : i;
    auto r = ev.eval(S, g);
    if (ev.nogroup(r)) nog++;
    if (ev.hit(r)) idx.push_back(i);
  }
  if (counts->n_hits != (int32_t)idx.size() || counts->n_nogroup != nog || counts->reserved[0] || counts->reserved[1]) {
    printf("%s: counts %d %d, want %zu %d\n", what, counts->n_hits, counts->n_nogroup, idx.size(), nog);
    exit(1);
  }
  const int32_t k = std::min<int32_t>((int32_t)idx.size(), cap);
  for (int32_t j = 0; j < cap; j++) {
    if (j < k) {
      const int32_t g = gidx ? gidx[idx[j]] : idx[j];
      if (O.i32[0][j] != g || !check(O, j, ev.eval(S, g))) {
        printf("%s: entry %d wrong (gidx %d, want %d)\n", what, j, O.i32[0][j], g);
        exit(1);
      }
    } else if (O.i32[0][j] != (int32_t)0xA5A5A5A5 || O.u8[0][j] != 0xA5 || O.i32[1][j] != (int32_t)0xA5A5A5A5) {
      printf("%s: entry %d written beyond the hits\n", what, j);
      exit(1);
    }
  }
  printf("%s: ok, %d hits of %d, %d no-group, cap %d\n", what, counts->n_hits, n, nog, cap);
  for (int q = 0; q < 6; q++) free(O.i32[q]);
  for (int q = 0; q < 2; q++) free(O.u8[q]);
  free(O.u64);
  free(base);
}

int main() {
  const int32_t T = GPX_SCAN_TILE_, G = 3 * T + 17;
  const size_t scan_cap = 4 * (size_t)T;
  std::vector<uint8_t> none(G, 0), all(G, 1), edges(G, 0), hole(G, 0), sparse(G, 0);
  for (int g : {0, 63, 64, 255, 256, T - 1, T, 2 * T - 1, 2 * T, 3 * T, 3 * T + 16}) edges[g] = 1;
  for (int g = 0; g < T; g++) hole[g] = hole[2 * T + g] = 1;
  for (int g = 0; g < G; g++) sparse[g] = (g * 2654435761u >> 7) % 97 == 0;
  auto ce = [](const ScanOut& O, int j, const ElectionRow& r) {
    return O.u8[0][j] == r.run && O.i32[1][j] == r.p_bnum && O.i32[2][j] == r.p_first;
  };
  auto cp = [](const ScanOut& O, int j, const PokeRow& r) {
    return O.u8[0][j] == r.poke && O.i32[1][j] == r.slot && O.i32[2][j] == r.bnum && O.i32[3][j] == r.bcoord &&
           O.i32[4][j] == r.median_cp && O.u8[1][j] == r.flags && (uint32_t)O.i32[5][j] == r.heard;
  };
  auto cg = [](const ScanOut& O, int j, const GapRow& r) {
    return O.i32[1][j] == r.first_slot && O.i32[2][j] == r.max_committed && O.u64[j] == r.missing && O.u8[0][j] == r.should_sync;
  };
  ScanElection se{};
  const char* names[] = {"all", "none", "sparse", "edges", "hole"};
  const std::vector<uint8_t>* hs[] = {&all, &none, &sparse, &edges, &hole};
  for (int s = 0; s < 5; s++) {
    char w[64];
    snprintf(w, sizeof w, "election %s", names[s]);
    run(w, G, G, nullptr, *hs[s], se, G, scan_cap, ce);
    if (s < 2) continue;
    snprintf(w, sizeof w, "poke %s", names[s]);
    run(w, G, G, nullptr, *hs[s], ScanPoke<4>{}, G, scan_cap, cp);
    snprintf(w, sizeof w, "gap %s", names[s]);
    run(w, G, G, nullptr, *hs[s], ScanGap{1, 0, 64, GPX_GAP_HIT_SYNC | GPX_GAP_HIT_MISSING | GPX_GAP_HIT_AHEAD}, G, scan_cap, cg);
  }
  // short capacities
  for (int32_t cap : {T + 5, 1, 0}) run("election all, short", G, G, nullptr, all, se, cap, scan_cap, ce);
  run("gap, every live group, cap 20", G, G, nullptr, sparse, ScanGap{1, 0, 64, 0}, 20, scan_cap, cg);
  // listed: not a multiple of 64, duplicates, out of range
  std::vector<int32_t> lst;
  for (int i = 0; i < 1531; i++) lst.push_back(i % 7 == 3 ? -1 : i % 11 == 0 ? G + i : (i * 37) % G);
  run("poke listed", G, (int32_t)lst.size(), lst.data(), hole, ScanPoke<16>{}, (int32_t)lst.size(), scan_cap, cp);
  run("n = 5", G, 5, lst.data(), all, se, 5, scan_cap, ce);
  run("n = 0", G, 0, nullptr, all, se, 0, scan_cap, ce);
  // many tiles: more than one round of k_scan_offsets
  const int32_t big = 257 * T + 1;
  std::vector<uint8_t> bh(big);
  for (int g = 0; g < big; g++) bh[g] = (g * 2654435761u >> 9) % 5 == 0;
  run("election 257 tiles + 1", big, big, nullptr, bh, se, big, 258 * (size_t)T, ce);
  // the counted begin
  {
    ScanCounts c{37, 0, {0, 0}};
    std::vector<int32_t> g(64), b(64);
    for (int i = 0; i < 64; i++) g[i] = i * 3, b[i] = i;
    uint8_t* st = blk<uint8_t>(50, 0xA5);
    DevState S{G, all.data()};
    launch(1, [&] { k_scan_election_begin(S, 50, &c, g.data(), b.data(), st); });
    for (int i = 0; i < 50; i++) assert(st[i] == (i < 37 ? ((g[i] + b[i]) & 3) : 0xA5));
    c.n_hits = 1000;
    launch(1, [&] { k_scan_election_begin(S, 50, &c, g.data(), b.data(), st); });
    for (int i = 0; i < 50; i++) assert(st[i] == ((g[i] + b[i]) & 3));
    free(st);
    printf("counted begin: ok\n");
  }
  return 0;
}
