// Lockstep CPU emulation of the kernels of gigapaxos_amd/csrc/gpx_timers.hip.h (tests/test_retransmit_sweep_abi.py
// compiles and runs this with AddressSanitizer): the real header, unmodified, over a stand-in for poke_scan_row.  One
// std::thread per lane of a workgroup, barriers for __syncthreads and for the wave collectives, one workgroup at a time.
// The parked columns and per-tile words start as garbage, the timer words as zeros (as the engine allocates them) and
// live on from call to call; every buffer is a heap block of its exact size, so an index past an end is a sanitizer
// report.  The expected answer is a plain loop over the rules of include/gpx_timers.h.  What this cannot show is what
// only the GPU has: the compiler's code, memory ordering between launches, and the real evaluation
// (tests/test_retransmit_sweep_gpu.py).
#include <algorithm>
#include <barrier>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "lockstep_runtime.h"

// ---- the fake engine side: the columns below ARE the groups' poke rows; evals counts the evaluations per group ----
#define GPX_S_OK 0
#define GPX_S_NOGROUP 1
#define GPX_POKE_NONE 0
#define GPX_POKE_ACCEPT 1
#define GPX_POKE_PREPARE 2
struct PokeRow {
  uint8_t poke, flags, status;
  int32_t slot, bnum, bcoord, median_cp;
  uint32_t heard;
};
struct DevState {
  int32_t G;
  const uint8_t *live, *poke;
  const int32_t *slot, *bnum;
  const uint32_t* heard;
};
template <int KMAX>
static PokeRow poke_scan_row(const DevState& S, int32_t g) {
  if ((uint32_t)g >= (uint32_t)S.G || !S.live[g]) return PokeRow{GPX_POKE_NONE, 0, GPX_S_NOGROUP, 0, 0, 0, 0, 0u};
  if (S.poke[g] == GPX_POKE_NONE) return PokeRow{GPX_POKE_NONE, 0, GPX_S_OK, 0, 0, 0, 0, 0u};
  return PokeRow{S.poke[g], (uint8_t)(g & 1), GPX_S_OK, S.slot[g], S.bnum[g], 100 + g % KMAX, S.slot[g] - 1 - g % 3, S.heard[g]};
}

#include "gpx_compact.hip.h"
#include "gpx_timers.hip.h"


struct Table { /* one engine: groups, timer words, scratch; and the reference's timer words */
  int32_t G;
  std::vector<uint8_t> live, poke;
  std::vector<int32_t> slot, bnum;
  std::vector<uint32_t> heard, ref_key;
  std::vector<int32_t> ref_since;
  std::vector<uint8_t> ref_count;
  RtxMem M;
  size_t tiles;
  Table(int32_t G_, size_t tiles_)
      : G(G_), live(G_, 1), poke(G_, GPX_POKE_ACCEPT), slot(G_), bnum(G_, 0), heard(G_, 0), ref_key(G_, 0), ref_since(G_, 0),
        ref_count(G_, 0), tiles(tiles_) {
    for (int g = 0; g < G; g++) slot[g] = g * 7 - 1000;
    M.key = blk<uint32_t>(G, 0), M.since = blk<int32_t>(G, 0), M.count = blk<uint8_t>(G, 0);
    M.park_g = blk<int32_t>(tiles * GPX_RTX_TILE, 0xEE), M.park_wait = blk<int32_t>(tiles * GPX_RTX_TILE, 0xEE);
    M.park_count = blk<uint8_t>(tiles * GPX_RTX_TILE, 0xEE);
    M.tile_hits = blk<int32_t>(tiles, 0xEE), M.tile_nog = blk<int32_t>(tiles, 0xEE);
    M.tile_wait = blk<int32_t>(tiles, 0xEE), M.tile_off = blk<int32_t>(tiles, 0xEE);
  }
  ~Table() {
    free(M.key), free(M.since), free(M.count), free(M.park_g), free(M.park_wait), free(M.park_count);
    free(M.tile_hits), free(M.tile_nog), free(M.tile_wait), free(M.tile_off);
  }
  DevState state() const { return DevState{G, live.data(), poke.data(), slot.data(), bnum.data(), heard.data()}; }
};

static void fail(const char* what, const char* msg, long a = 0, long b = 0) {
  printf("%s: %s (%ld, %ld)\n", what, msg, a, b);
  exit(1);
}

struct Hit { int32_t g, waited; uint8_t count; PokeRow r; };

template <int KMAX>
static int32_t run(const char* what, Table& T, int32_t n, const int32_t* gidx, int32_t now, const RtxCfg& cfg, int32_t flags,
                   int32_t cap) {
  const bool peek = flags & GPX_RTX_PEEK_;
  const DevState S = T.state();
  // the expected answer, by the rules of include/gpx_timers.h
  std::vector<Hit> hits;
  std::vector<uint32_t> want_key = T.ref_key;
  std::vector<int32_t> want_since = T.ref_since;
  std::vector<uint8_t> want_count = T.ref_count;
  int32_t nog = 0, waiting = 0;
  for (int32_t i = 0; i < n; i++) {
    const int32_t g = gidx ? gidx[i] : i;
    const bool in = (uint32_t)g < (uint32_t)T.G;
    const PokeRow r = poke_scan_row<KMAX>(S, g);
    if (r.status == GPX_S_NOGROUP) {
      nog++;
      if (in) want_key[g] = 0, want_since[g] = 0, want_count[g] = 0;
    } else if (r.poke == GPX_POKE_NONE) {
      want_key[g] = 0, want_count[g] = 0;
    } else {
      waiting++;
      const uint32_t k = rtx_key(r.poke, r.slot, r.bnum, r.bcoord);
      if (k != T.ref_key[g]) {
        want_key[g] = k, want_since[g] = now, want_count[g] = 0;
      } else {
        const int32_t waited = (int32_t)((uint32_t)now - (uint32_t)T.ref_since[g]);
        const int32_t* tab = r.poke == GPX_POKE_PREPARE ? cfg.prepare_ms : cfg.accept_ms;
        if (waited > tab[std::min<int32_t>(T.ref_count[g], cfg.n_steps - 1)])
          hits.push_back(Hit{g, waited, (uint8_t)std::min(T.ref_count[g] + 1, 255), r});
      }
    }
  }
  const int32_t k = std::min<int32_t>((int32_t)hits.size(), cap);
  if (peek) {
    want_key = T.ref_key, want_since = T.ref_since, want_count = T.ref_count;
  } else {
    for (int32_t j = 0; j < k; j++) want_count[hits[j].g] = hits[j].count, want_since[hits[j].g] = now;
  }

  int32_t *o_g = blk<int32_t>(cap, 0xA5), *o_sl = blk<int32_t>(cap, 0xA5), *o_bn = blk<int32_t>(cap, 0xA5);
  int32_t *o_bc = blk<int32_t>(cap, 0xA5), *o_md = blk<int32_t>(cap, 0xA5), *o_wt = blk<int32_t>(cap, 0xA5);
  uint8_t *o_pk = blk<uint8_t>(cap, 0xA5), *o_fl = blk<uint8_t>(cap, 0xA5), *o_ct = blk<uint8_t>(cap, 0xA5);
  uint32_t* o_hd = blk<uint32_t>(cap, 0xA5);
  RtxCounts* counts = blk<RtxCounts>(1, 0xA5);
  const RtxOut O{o_g, o_pk, o_sl, o_bn, o_bc, o_md, o_fl, o_hd, o_ct, o_wt};
  const int ntiles = (n + GPX_RTX_TILE - 1) / GPX_RTX_TILE;
  if ((size_t)ntiles > T.tiles) fail(what, "more tiles than the table's scratch holds");
  launch(ntiles, [&] { k_rtx_tile<KMAX>(S, n, gidx, now, cfg, flags, T.M); });
  for (int32_t j = 0; j < (int32_t)hits.size(); j++) /* which hits fit is not known yet */
    if (T.M.count[hits[j].g] != T.ref_count[hits[j].g] || T.M.since[hits[j].g] != T.ref_since[hits[j].g])
      fail(what, "a hit was re-armed by the first launch", hits[j].g);
  launch(1, [&] { k_rtx_offsets(ntiles, T.M, cap, flags, counts); });
  if (ntiles && cap > 0) launch(ntiles, [&] { k_rtx_move<KMAX>(S, T.M, now, cap, flags, O); });

  if (counts->n_hits != (int32_t)hits.size() || counts->n_nogroup != nog || counts->n_waiting != waiting ||
      counts->n_fired != (peek ? 0 : k)) {
    printf("%s: counts %d %d %d %d, want %zu %d %d %d\n", what, counts->n_hits, counts->n_nogroup, counts->n_waiting,
           counts->n_fired, hits.size(), nog, waiting, peek ? 0 : k);
    exit(1);
  }
  const int32_t s4 = (int32_t)0xA5A5A5A5;
  for (int32_t j = 0; j < cap; j++) {
    if (j < k) {
      const Hit& h = hits[j];
      if (o_g[j] != h.g || o_pk[j] != h.r.poke || o_sl[j] != h.r.slot || o_bn[j] != h.r.bnum || o_bc[j] != h.r.bcoord ||
          o_md[j] != h.r.median_cp || o_fl[j] != h.r.flags || o_hd[j] != h.r.heard || o_ct[j] != h.count || o_wt[j] != h.waited)
        fail(what, "entry wrong", j, o_g[j]);
    } else if (o_g[j] != s4 || o_pk[j] != 0xA5 || o_sl[j] != s4 || o_bn[j] != s4 || o_bc[j] != s4 || o_md[j] != s4 ||
               o_fl[j] != 0xA5 || o_hd[j] != 0xA5A5A5A5u || o_ct[j] != 0xA5 || o_wt[j] != s4) {
      fail(what, "entry written beyond the hits", j);
    }
  }
  for (int32_t g = 0; g < T.G; g++)
    if (T.M.key[g] != want_key[g] || T.M.since[g] != want_since[g] || T.M.count[g] != want_count[g])
      fail(what, "timer words", g, T.M.count[g]);
  T.ref_key = want_key, T.ref_since = want_since, T.ref_count = want_count;
  printf("%s: ok, %d hits of %d, %d no-group, %d waiting, cap %d, fired %d\n", what, counts->n_hits, n, nog, waiting, cap,
         counts->n_fired);
  const int32_t found = counts->n_hits;
  free(o_g), free(o_sl), free(o_bn), free(o_bc), free(o_md), free(o_wt), free(o_pk), free(o_fl), free(o_ct), free(o_hd);
  free(counts);
  return found;
}

int main() {
  const int32_t T = GPX_RTX_TILE, G = 3 * T + 17, P = GPX_RTX_PEEK_;
  RtxCfg cfg;
  memset(&cfg, 0x7f, sizeof cfg); /* entries at and beyond n_steps are never read: garbage there */
  cfg.n_steps = 3;
  for (int c = 0; c < 3; c++) cfg.accept_ms[c] = 100 + 50 * c, cfg.prepare_ms[c] = 40 + 30 * c;
  std::vector<uint8_t> none(G, 0), all(G, 1), edges(G, 0), hole(G, 0), sparse(G, 0);
  for (int g : {0, 63, 64, 255, 256, T - 1, T, 2 * T - 1, 2 * T, 3 * T - 1, 3 * T, 3 * T + 16}) edges[g] = 1;
  for (int g = 0; g < T; g++) hole[g] = hole[2 * T + g] = 1;
  for (int g = 0; g < G; g++) sparse[g] = (g * 2654435761u >> 7) % 97 == 0;
  const char* names[] = {"all", "none", "sparse", "edges", "hole"};
  const std::vector<uint8_t>* hs[] = {&all, &none, &sparse, &edges, &hole};
  // every hit set: ACCEPTs and (every third) PREPAREs; outside the set every 5th group waits for nothing, the others
  // decide between the sweeps (a new key); groups G .. G + 7 are dead
  for (int s = 0; s < 5; s++) {
    Table t(G + 8, 4);
    for (int g = 0; g < G + 8; g++) {
      t.live[g] = g < G;
      t.poke[g] = ((*hs[s])[g % G] || g % 5) ? (g % 3 ? GPX_POKE_ACCEPT : GPX_POKE_PREPARE) : GPX_POKE_NONE;
    }
    char w[80];
    snprintf(w, sizeof w, "%s, first sweep", names[s]);
    if (run<4>(w, t, G + 8, nullptr, 5000, cfg, 0, G + 8) != 0) fail(w, "a first sweep has hits");
    for (int g = 0; g < G; g++) {
      if (!(*hs[s])[g]) t.slot[g] += 1; /* decided: the head of line moved */
      t.heard[g] = 1u + (uint32_t)g % 3; /* replies: not part of the key */
    }
    snprintf(w, sizeof w, "%s, not yet due", names[s]);
    if (run<4>(w, t, G + 8, nullptr, 5040, cfg, P, G + 8) != 0) fail(w, "due at the threshold itself");
    snprintf(w, sizeof w, "%s, peek", names[s]);
    run<4>(w, t, G + 8, nullptr, 5101, cfg, P, G + 8);
    snprintf(w, sizeof w, "%s, second sweep", names[s]);
    run<4>(w, t, G + 8, nullptr, 5101, cfg, 0, G + 8);
    snprintf(w, sizeof w, "%s, third sweep", names[s]);
    run<4>(w, t, G + 8, nullptr, 5202, cfg, 0, G + 8);
    snprintf(w, sizeof w, "%s, after", names[s]);
    run<4>(w, t, G + 8, nullptr, 5600, cfg, P, G + 8);
  }
  // cap cuts on the 'all' table: re-arming happens only below cap, the next call takes the next ones
  {
    Table t(G, 4);
    run<8>("cuts: first sweep", t, G, nullptr, -50, cfg, 0, 0);
    run<8>("cuts: cap 0", t, G, nullptr, 100, cfg, 0, 0);
    run<8>("cuts: cap 1", t, G, nullptr, 100, cfg, 0, 1);
    run<8>("cuts: cap T + 5", t, G, nullptr, 100, cfg, 0, T + 5);
    run<8>("cuts: cap = hits - 1", t, G, nullptr, 101, cfg, 0, G - 1 - (T + 5) - 1);
    if (run<8>("cuts: the last one", t, G, nullptr, 102, cfg, 0, 5) != 1) fail("cuts", "one hit was to be left");
    if (run<8>("cuts: nothing left", t, G, nullptr, 103, cfg, 0, G) != 0) fail("cuts", "a re-armed wait hit again");
  }
  // counts saturating at 255, the threshold index stopping at n_steps - 1; the clock wrapping and stepping back
  {
    Table t(G, 4);
    const int32_t late = INT32_MAX - 20;
    for (int g = 0; g < G; g++) t.poke[g] = g % 3 ? GPX_POKE_ACCEPT : GPX_POKE_PREPARE;
    run<16>("saturation: first", t, G, nullptr, late, cfg, 0, G);
    for (int g = 0; g < G; g++) t.M.count[g] = t.ref_count[g] = (uint8_t)(250 + g % 6);
    if (run<16>("clock: stepped back", t, G, nullptr, late - 1000, cfg, 0, G) != 0) fail("clock", "a negative wait hit");
    if (run<16>("clock: at the last threshold", t, G, nullptr, (int32_t)((uint32_t)late + 200u), cfg, 0, G) != G / 3 + 1)
      fail("clock", "the PREPAREs, and only they, were to be due across the wrap");
    run<16>("saturation: 250..255 + 1, cap T + 100", t, G, nullptr, (int32_t)((uint32_t)late + 500u), cfg, 0, T + 100);
    run<16>("saturation: the rest", t, G, nullptr, (int32_t)((uint32_t)late + 500u), cfg, 0, G);
  }
  // listed: not a multiple of 64, distinct, with dead and out-of-range entries
  {
    Table t(G, 4);
    for (int g = 0; g < G; g++) t.live[g] = g % 11 != 3, t.poke[g] = g % 4 == 1 ? GPX_POKE_NONE : g % 4 == 2 ? GPX_POKE_PREPARE : GPX_POKE_ACCEPT;
    std::vector<int32_t> lst;
    for (int i = 0; i < 1531; i++) lst.push_back(i % 97 == 5 ? -1 - i : i % 89 == 7 ? G + i : (int32_t)(((int64_t)i * 37) % G));
    run<4>("listed: first", t, (int32_t)lst.size(), lst.data(), 7, cfg, 0, (int32_t)lst.size());
    for (int g = 0; g < G; g += 2) t.bnum[g] += 1; /* a higher ballot: a new wait */
    run<4>("listed: second, cap 100", t, (int32_t)lst.size(), lst.data(), 200, cfg, 0, 100);
    run<4>("listed: third", t, (int32_t)lst.size(), lst.data(), 400, cfg, 0, (int32_t)lst.size());
    run<4>("listed: n = 5", t, 5, lst.data() + 100, 900, cfg, 0, 5);
    run<4>("n = 0", t, 0, nullptr, 900, cfg, 0, 0);
  }
  // many tiles: more than one round of k_rtx_offsets
  {
    const int32_t big = 257 * T + 1;
    Table t(big, 258);
    for (int g = 0; g < big; g++) t.live[g] = g % 3 != 0, t.poke[g] = (g * 2654435761u >> 9) % 5 == 0 ? GPX_POKE_ACCEPT : GPX_POKE_NONE;
    run<4>("258 tiles: first", t, big, nullptr, 0, cfg, 0, 0);
    run<4>("258 tiles: cap = a tenth", t, big, nullptr, 1000, cfg, 0, big / 10);
  }
  return 0;
}
