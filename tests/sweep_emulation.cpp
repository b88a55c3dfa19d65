// Lockstep CPU emulation of the kernels of gigapaxos_amd/csrc/gpx_sweep.hip.h (tests/test_pause_sweep_abi.py compiles
// and runs this with AddressSanitizer): the real header, unmodified, over a stand-in for the per-group evaluation, the
// restore row and the pause.  One std::thread per lane of a workgroup, barriers for __syncthreads and for the wave
// collectives, one workgroup at a time.  The parked columns and per-tile words start as garbage, the idle words as
// zeros (as the engine allocates them) and live on from call to call; every buffer is a heap block of its exact size,
// so an index past an end is a sanitizer report.  The expected answer is a plain loop over the rules of
// include/gpx_sweep.h.  What this cannot show is what only the GPU has: the compiler's code, memory ordering between
// launches, and the real evaluation (tests/test_pause_sweep_gpu.py).
#include <algorithm>
#include <barrier>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "lockstep_runtime.h"

// ---- the fake engine side: kind[g] and sigv[g] ARE the group; pausing makes it dead ----
#define SWEEP_NOGROUP 0
#define SWEEP_BUSY 1
#define SWEEP_CAUGHT 2
struct SweepRow { int32_t kind; uint32_t sig; };
struct DevState { int32_t G; uint8_t* kind; const uint32_t* sigv; uint32_t* g_flags; int32_t* pauses; };
struct gpx_hri { int32_t w[25]; };
struct NameCopies { int32_t tag; };
static SweepRow sweep_eval(const DevState& S, int32_t g) {
  if ((uint32_t)g >= (uint32_t)S.G || S.kind[g] == SWEEP_NOGROUP) return SweepRow{SWEEP_NOGROUP, 0u};
  return SweepRow{S.kind[g], S.sigv[g]};
}
static void fill_hri_dev(const DevState& S, int32_t g, uint32_t gf, gpx_hri* out) {
  gpx_hri r;
  for (int q = 0; q < 25; q++) r.w[q] = g * 31 + q + (int32_t)gf + (S.kind[g] == SWEEP_CAUGHT ? 0 : 1000000);
  *out = r;
}
static void group_retire_apply(const DevState& S, int32_t g, const NameCopies& names) {
  if (names.tag != 77 || S.kind[g] != SWEEP_CAUGHT) {
    printf("pause of group %d, which is not live and caught up\n", g);
    exit(1);
  }
  S.kind[g] = SWEEP_NOGROUP;
  S.g_flags[g] = 0;
  S.pauses[g]++;
}

#include "gpx_compact.hip.h"
#include "gpx_sweep.hip.h"


struct Table { /* one engine: groups, idle words, scratch; and the reference's idle words */
  int32_t G;
  std::vector<uint8_t> kind;
  std::vector<uint32_t> sigv, gflags, ref_sig;
  std::vector<int32_t> pauses;
  std::vector<uint8_t> ref_age;
  SweepMem M;
  size_t tiles;
  Table(int32_t G_, size_t tiles_) : G(G_), kind(G_), sigv(G_), gflags(G_), ref_sig(G_, 0), pauses(G_, 0), ref_age(G_, 0), tiles(tiles_) {
    for (int g = 0; g < G; g++) sigv[g] = (uint32_t)g * 2654435761u | 1u, gflags[g] = 1u | (3u << 8);
    M.sig = blk<uint32_t>(G, 0), M.age = blk<uint8_t>(G, 0);
    M.park_g = blk<int32_t>(tiles * GPX_SWEEP_TILE, 0xEE), M.park_age = blk<uint8_t>(tiles * GPX_SWEEP_TILE, 0xEE);
    M.tile_hits = blk<int32_t>(tiles, 0xEE), M.tile_nog = blk<int32_t>(tiles, 0xEE);
    M.tile_busy = blk<int32_t>(tiles, 0xEE), M.tile_off = blk<int32_t>(tiles, 0xEE);
  }
  ~Table() {
    free(M.sig), free(M.age), free(M.park_g), free(M.park_age);
    free(M.tile_hits), free(M.tile_nog), free(M.tile_busy), free(M.tile_off);
  }
};

static void fail(const char* what, const char* msg, long a = 0, long b = 0) {
  printf("%s: %s (%ld, %ld)\n", what, msg, a, b);
  exit(1);
}

static int32_t run(const char* what, Table& T, int32_t n, const int32_t* gidx, int32_t min_age, int32_t flags, int32_t cap) {
  const bool peek = flags & GPX_SWEEP_PEEK_, hold = flags & GPX_SWEEP_HOLD_;
  // the expected answer, by the rules of include/gpx_sweep.h
  std::vector<int32_t> hit_g;
  std::vector<uint8_t> hit_age;
  std::vector<uint32_t> want_sig = T.ref_sig;
  std::vector<uint8_t> want_age = T.ref_age, want_kind = T.kind;
  int32_t nog = 0, bsy = 0;
  for (int32_t i = 0; i < n; i++) {
    const int32_t g = gidx ? gidx[i] : i;
    const bool in = (uint32_t)g < (uint32_t)T.G;
    if (!in || T.kind[g] == SWEEP_NOGROUP) {
      nog++;
      if (in) want_sig[g] = 0, want_age[g] = 0;
    } else if (T.kind[g] == SWEEP_BUSY) {
      bsy++;
      want_age[g] = 0;
    } else {
      int32_t a = 0;
      if (T.sigv[g] == T.ref_sig[g]) a = hold ? T.ref_age[g] : std::min(T.ref_age[g] + 1, 255);
      want_sig[g] = T.sigv[g], want_age[g] = (uint8_t)a;
      if (a >= min_age) hit_g.push_back(g), hit_age.push_back((uint8_t)a);
    }
  }
  const int32_t k = std::min<int32_t>((int32_t)hit_g.size(), cap);
  if (peek) {
    want_sig = T.ref_sig, want_age = T.ref_age;
  } else {
    for (int32_t j = 0; j < k; j++) want_sig[hit_g[j]] = 0, want_age[hit_g[j]] = 0, want_kind[hit_g[j]] = SWEEP_NOGROUP;
  }
  // the rows as they would be built BEFORE any pause
  std::vector<gpx_hri> want_rows(k);
  DevState S{T.G, T.kind.data(), T.sigv.data(), T.gflags.data(), T.pauses.data()};
  for (int32_t j = 0; j < k; j++) fill_hri_dev(S, hit_g[j], T.gflags[hit_g[j]], &want_rows[j]);
  std::fill(T.pauses.begin(), T.pauses.end(), 0);
  const std::vector<uint8_t> kind_before = T.kind;
  std::vector<int32_t> want_pauses(T.G, 0);
  for (int32_t j = 0; j < k && !peek; j++) want_pauses[hit_g[j]] = 1;

  int32_t* o_g = blk<int32_t>(cap, 0xA5);
  uint8_t* o_a = blk<uint8_t>(cap, 0xA5);
  gpx_hri* o_r = blk<gpx_hri>(cap, 0xA5);
  SweepCounts* counts = blk<SweepCounts>(1, 0xA5);
  const int ntiles = (n + GPX_SWEEP_TILE - 1) / GPX_SWEEP_TILE;
  if ((size_t)ntiles > T.tiles) fail(what, "more tiles than the table's scratch holds");
  launch(ntiles, [&] { k_sweep_tile(S, n, gidx, min_age, flags, T.M); });
  if (T.kind != kind_before || std::count(T.pauses.begin(), T.pauses.end(), 0) != T.G) /* the offsets are not known yet */
    fail(what, "a group was paused by the first launch");
  launch(1, [&] { k_sweep_offsets(ntiles, T.M, cap, flags, counts); });
  if (ntiles && cap > 0) launch(ntiles, [&] { k_sweep_move(S, T.M, NameCopies{77}, cap, flags, o_g, o_a, o_r); });

  if (counts->n_hits != (int32_t)hit_g.size() || counts->n_nogroup != nog || counts->n_busy != bsy ||
      counts->n_paused != (peek ? 0 : k)) {
    printf("%s: counts %d %d %d %d, want %zu %d %d %d\n", what, counts->n_hits, counts->n_nogroup, counts->n_busy,
           counts->n_paused, hit_g.size(), nog, bsy, peek ? 0 : k);
    exit(1);
  }
  gpx_hri sentinel;
  memset(&sentinel, 0xA5, sizeof sentinel);
  for (int32_t j = 0; j < cap; j++) {
    if (j < k) {
      if (o_g[j] != hit_g[j] || o_a[j] != hit_age[j] || memcmp(&o_r[j], &want_rows[j], sizeof(gpx_hri))) fail(what, "entry wrong", j, o_g[j]);
    } else if (o_g[j] != (int32_t)0xA5A5A5A5 || o_a[j] != 0xA5 || memcmp(&o_r[j], &sentinel, sizeof sentinel)) {
      fail(what, "entry written beyond the hits", j);
    }
  }
  for (int32_t g = 0; g < T.G; g++) {
    if (T.kind[g] != want_kind[g]) fail(what, "wrong group paused or left alive", g, T.kind[g]);
    if (T.pauses[g] != want_pauses[g]) fail(what, "pause count", g, T.pauses[g]);
    if (T.M.sig[g] != want_sig[g] || T.M.age[g] != want_age[g]) fail(what, "idle words", g, T.M.age[g]);
  }
  T.ref_sig = want_sig, T.ref_age = want_age;
  printf("%s: ok, %d hits of %d, %d no-group, %d busy, cap %d, paused %d\n", what, counts->n_hits, n, nog, bsy, cap,
         counts->n_paused);
  const int32_t found = counts->n_hits;
  free(o_g), free(o_a), free(o_r), free(counts);
  return found;
}

int main() {
  const int32_t T = GPX_SWEEP_TILE, G = 3 * T + 17, P = GPX_SWEEP_PEEK_, H = GPX_SWEEP_HOLD_;
  std::vector<uint8_t> none(G, 0), all(G, 1), edges(G, 0), hole(G, 0), sparse(G, 0);
  for (int g : {0, 63, 64, 255, 256, T - 1, T, 2 * T - 1, 2 * T, 3 * T - 1, 3 * T, 3 * T + 16}) edges[g] = 1;
  for (int g = 0; g < T; g++) hole[g] = hole[2 * T + g] = 1;
  for (int g = 0; g < G; g++) sparse[g] = (g * 2654435761u >> 7) % 97 == 0;
  const char* names[] = {"all", "none", "sparse", "edges", "hole"};
  const std::vector<uint8_t>* hs[] = {&all, &none, &sparse, &edges, &hole};
  // every hit set: the groups outside the set are busy (every 5th) or change between the sweeps; groups G .. G + 7 are dead
  for (int s = 0; s < 5; s++) {
    Table t(G + 8, 4);
    for (int g = 0; g < G + 8; g++) t.kind[g] = g >= G ? SWEEP_NOGROUP : ((*hs[s])[g] || g % 5) ? SWEEP_CAUGHT : SWEEP_BUSY;
    char w[80];
    snprintf(w, sizeof w, "%s, first sweep", names[s]);
    if (run(w, t, G + 8, nullptr, 1, 0, G + 8) != 0) fail(w, "a first sweep at min_age 1 has hits");
    for (int g = 0; g < G; g++)
      if (!(*hs[s])[g]) t.sigv[g] += 2; /* activity */
    snprintf(w, sizeof w, "%s, peek", names[s]);
    run(w, t, G + 8, nullptr, 1, P, G + 8);
    snprintf(w, sizeof w, "%s, second sweep", names[s]);
    run(w, t, G + 8, nullptr, 1, 0, G + 8);
    snprintf(w, sizeof w, "%s, after", names[s]);
    run(w, t, G + 8, nullptr, 0, P | H, G + 8);
  }
  // cap cuts on the 'all' table: pausing happens only below cap, a HOLD call takes the next ones
  {
    Table t(G, 4);
    std::fill(t.kind.begin(), t.kind.end(), (uint8_t)SWEEP_CAUGHT);
    run("cuts: first sweep", t, G, nullptr, 1, 0, 0);
    run("cuts: cap 0", t, G, nullptr, 1, 0, 0);
    run("cuts: cap 1", t, G, nullptr, 1, H, 1);
    run("cuts: cap T + 5", t, G, nullptr, 1, H, T + 5);
    run("cuts: cap = hits - 1", t, G, nullptr, 1, H, G - 1 - (T + 5) - 1);
    if (run("cuts: the last one", t, G, nullptr, 1, H, 5) != 1) fail("cuts", "one hit was to be left");
    if (run("cuts: nothing left", t, G, nullptr, 0, 0, G) != 0) fail("cuts", "a paused group hit again");
  }
  // forced pause (min_age 0) with a cap that ends inside tile 1, ages saturating at 255
  {
    Table t(G, 4);
    for (int g = 0; g < G; g++) t.kind[g] = g % 7 ? SWEEP_CAUGHT : SWEEP_BUSY;
    run("saturation: first", t, G, nullptr, 1, 0, G);
    for (int g = 0; g < G; g++) t.M.age[g] = t.ref_age[g] = (uint8_t)(g % 7 ? 250 + g % 6 : 0);
    run("saturation: 250..255 + 1", t, G, nullptr, 255, P, G);
    run("saturation: counted", t, G, nullptr, 255, 0, 0);
    run("forced, cap T + 100", t, G, nullptr, 0, 0, T + 100);
  }
  // listed: not a multiple of 64, distinct, with dead and out-of-range entries
  {
    Table t(G, 4);
    for (int g = 0; g < G; g++) t.kind[g] = g % 11 == 3 ? SWEEP_NOGROUP : g % 4 == 1 ? SWEEP_BUSY : SWEEP_CAUGHT;
    std::vector<int32_t> lst;
    for (int i = 0; i < 1531; i++) lst.push_back(i % 97 == 5 ? -1 - i : i % 89 == 7 ? G + i : (int32_t)(((int64_t)i * 37) % G));
    run("listed: first", t, (int32_t)lst.size(), lst.data(), 1, 0, (int32_t)lst.size());
    run("listed: second, cap 100", t, (int32_t)lst.size(), lst.data(), 1, 0, 100);
    run("listed: n = 5", t, 5, lst.data() + 100, 0, 0, 5);
    run("n = 0", t, 0, nullptr, 0, 0, 0);
  }
  // many tiles: more than one round of k_sweep_offsets
  {
    const int32_t big = 257 * T + 1;
    Table t(big, 258);
    for (int g = 0; g < big; g++) t.kind[g] = (g * 2654435761u >> 9) % 5 == 0 ? SWEEP_CAUGHT : g % 3 ? SWEEP_BUSY : SWEEP_NOGROUP;
    run("258 tiles: forced, cap = half", t, big, nullptr, 0, 0, big / 10);
  }
  return 0;
}
