// Lockstep CPU emulation of the kernels of gigapaxos_amd/csrc/gpx_delta.hip.h and of the functions of gpx_image.hip.h they
// are built from (tests/test_group_delta_abi.py compiles and runs this with AddressSanitizer and UBSan): the real
// headers, unmodified, over a table whose columns have the engine's names.  One std::thread per lane of a workgroup,
// barriers for __syncthreads and for the wave collectives, one workgroup at a time (the scheme of
// tests/sweep_emulation.cpp).  Scratch starts as garbage, the marks as zeros (as the engine allocates them) and live on
// from call to call; every buffer is a heap block of its exact size, so an index past an end is a sanitizer report.
// The expected answer is a plain loop over the rules of include/gpx_delta.h: the mark of a group is "its canonical
// rows at the export that last wrote it" (canon_rows below restates include/gpx_image.h word by word), changed means
// "the rows differ".  What this cannot show is what only the GPU has: the compiler's code and memory ordering between
// launches (tests/test_group_delta_gpu.py).
#include <algorithm>
#include <barrier>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "lockstep_runtime.h"

/* what gpx_kernels.hip.h gives the two headers: the same names, the same meaning */
struct __attribute__((aligned(16))) I4 { int32_t x, y, z, w; };
static I4 mk4(int32_t x, int32_t y, int32_t z, int32_t w) { return I4{x, y, z, w}; }
#define GF_EXISTS 1u
#define GF_STOPPED 2u
#define GF_HASCOORD 4u
#define GF_PREPARING 8u
#define GF_K(f) (((f) >> 8) & 0xffu)
#define PR_PRESENT 0x10000u
#define PR_STOP 0x20000u
#define RF_PRESENT 1
#define RF_STOP 2
#define RF_HASVALUE 4
#define AF_MASK 0xffu
#define CF_SHIFT 8
#define CO_PRESENT 0x100
struct DevState {
  int32_t G, kmax, W, my_id;
  uint32_t flags;
  uint32_t* g_flags;
  int32_t* g_version;
  int32_t *a_slot, *a_bnum, *a_bcoord, *a_gc;
  int32_t *c_bnum, *c_bcoord, *c_next, *c_pcount;
  int32_t* members;
  int32_t* node_slots;
  uint32_t* p_ring;
  I4* acc_ring;
  I4* com_ring;
  uint32_t* c_wait;
  I4* co_ring;
  int64_t* co_handle;
  int64_t* p_handle;
};
struct NameCopies { /* the wire codec's copies of (exists, version) */
  uint8_t* exists;
  int32_t* version;
  void set(int32_t g, bool ex, bool set_version, int32_t v) const {
    exists[g] = ex ? 1 : 0;
    if (set_version) version[g] = v;
  }
};
static void group_retire_apply(const DevState& S, int32_t g, const NameCopies& names) {
  S.g_flags[g] = 0;
  names.set(g, false, false, 0);
}

#include "gpx_delta.h"
#include "gpx_compact.hip.h"
#include "gpx_image.hip.h"
#include "gpx_delta.hip.h"

static void fail(const char* what, const char* msg, long a = 0, long b = 0) {
  printf("%s: %s (%ld, %ld)\n", what, msg, a, b);
  exit(1);
}
static uint32_t g_rng = 12345u;
static uint32_t rnd() {
  g_rng = g_rng * 1664525u + 1013904223u;
  return g_rng >> 8;
}
static int32_t junk() { return (int32_t)(rnd() | 0x1000u); } /* never zero */

typedef std::vector<int32_t> Rows; /* one or two rows of stride_w words */

struct Table { /* one engine: the state columns, the wire codec's copies, the sweep's idle words, marks and scratch */
  int32_t G, K, W, ME = 100, stride_w;
  bool elect;
  DevState S;
  NameCopies names;
  ImageIdle idle;
  DeltaMem M;
  ImageMem IM;
  size_t tiles;
  std::vector<Rows> ref; /* the model's marks: the rows at the export that last wrote the group; empty = mark 0 */
  std::vector<void*> owned;
  template <class T> T* mk(size_t n, int fill) {
    T* p = blk<T>(n, fill);
    owned.push_back(p);
    return p;
  }
  Table(const Table&) = delete;
  ~Table() {
    for (void* p : owned) free(p);
  }
  Table(int32_t G_, int32_t K_, int32_t W_, bool elect_, size_t tiles_) : G(G_), K(K_), W(W_), elect(elect_), tiles(tiles_), ref(G_) {
    stride_w = image_stride_words(K, W);
    S.G = G, S.kmax = K, S.W = W, S.my_id = ME, S.flags = 0;
    S.g_flags = mk<uint32_t>(G, 0), S.g_version = mk<int32_t>(G, 0x11);
    S.a_slot = mk<int32_t>(G, 0x11), S.a_bnum = mk<int32_t>(G, 0x11), S.a_bcoord = mk<int32_t>(G, 0x11), S.a_gc = mk<int32_t>(G, 0x11);
    S.c_bnum = mk<int32_t>(G, 0x11), S.c_bcoord = mk<int32_t>(G, 0x11), S.c_next = mk<int32_t>(G, 0x11), S.c_pcount = mk<int32_t>(G, 0x11);
    S.members = mk<int32_t>((size_t)K * G, 0x11), S.node_slots = mk<int32_t>((size_t)K * G, 0x11);
    S.p_ring = mk<uint32_t>((size_t)W * G, 0), S.acc_ring = mk<I4>((size_t)W * G, 0), S.com_ring = mk<I4>((size_t)W * G, 0x11);
    S.c_wait = elect ? mk<uint32_t>(G, 0x11) : nullptr;
    S.co_ring = elect ? mk<I4>((size_t)W * G, 0) : nullptr;
    S.co_handle = elect ? mk<int64_t>((size_t)W * G, 0x11) : nullptr;
    S.p_handle = elect ? mk<int64_t>((size_t)W * G, 0x11) : nullptr;
    names.exists = mk<uint8_t>(G, 0), names.version = mk<int32_t>(G, 0);
    idle.sig = mk<uint32_t>(G, 0x33), idle.age = mk<uint8_t>(G, 0x33);
    const size_t cap = tiles * GPX_IMAGE_TILE;
    M.marks = mk<unsigned long long>(G, 0);
    M.park = mk<int32_t>(cap, 0xEE), M.park_sig = mk<unsigned long long>(cap, 0xEE), M.park_gone = mk<int32_t>(cap, 0xEE);
    M.tile_live = mk<int32_t>(tiles, 0xEE), M.tile_chg = mk<int32_t>(tiles, 0xEE), M.tile_rows = mk<int32_t>(tiles, 0xEE);
    M.tile_gone = mk<int32_t>(tiles, 0xEE), M.tile_off = mk<int32_t>(tiles, 0xEE), M.tile_goff = mk<int32_t>(tiles, 0xEE);
    M.tile_xoff = mk<int32_t>(tiles, 0xEE);
    IM.park = IM.tile_live = IM.tile_rows = IM.tile_off = IM.tile_goff = nullptr; /* the image export's: not used here */
    IM.desc = mk<uint8_t>(2 * cap, 0xEE), IM.src = mk<int32_t>(2 * cap, 0xEE);
  }
  bool live(int32_t g) const { return (S.g_flags[g] & GF_EXISTS) != 0; }

  /* group g into a random VALID state (one gpx_group_import would take), with stale words wherever the state defines
   * none: under clear present bits, beyond k, in the coordinator words of a group without a coordinator, in the
   * election words of a group that is not running */
  void fill(int32_t g, int mode = -1) {
    const int64_t Gq = G;
    const int32_t k = 1 + (int32_t)(rnd() % (uint32_t)K);
    const bool hc = mode >= 0 ? mode >= 1 : rnd() % 2, prep = elect && hc && (mode >= 0 ? mode == 2 : rnd() % 3 == 0);
    const bool full = mode >= 0; /* every entry present, k = K: every word of the rows is live state */
    const int32_t kk = full ? K : k;
    S.g_version[g] = (int32_t)(rnd() % 7), S.a_slot[g] = (int32_t)rnd(), S.a_bnum[g] = (int32_t)(rnd() % 9);
    S.a_bcoord[g] = ME + (int32_t)(rnd() % 3), S.a_gc[g] = (int32_t)rnd() - 5;
    const int32_t c_next = (int32_t)(rnd() * 977u), pc = full ? W : (int32_t)(rnd() % (uint32_t)(W + 1));
    S.c_bnum[g] = hc ? (int32_t)(rnd() % 9) : junk(), S.c_bcoord[g] = hc ? ME : junk();
    S.c_next[g] = hc ? c_next : junk(), S.c_pcount[g] = hc ? pc : junk();
    for (int32_t j = 0; j < K; j++) {
      S.members[j * Gq + g] = j < kk ? ME + j : junk();
      S.node_slots[j * Gq + g] = (hc && j < kk) ? (int32_t)rnd() : junk();
    }
    for (int32_t x = 0; x < W; x++) S.p_ring[x * Gq + g] = hc ? (rnd() & 0xffffu) | 0x40000u : (uint32_t)junk();
    if (hc)
      for (int32_t d = 1; d <= pc; d++) {
        const int32_t x = (int32_t)(((uint32_t)c_next - (uint32_t)d) & (uint32_t)(W - 1));
        S.p_ring[x * Gq + g] = (rnd() & 0xffffu) | PR_PRESENT | (rnd() % 4 == 0 ? PR_STOP : 0u) | (rnd() % 2 ? 0x40000u : 0u);
      }
    for (int32_t x = 0; x < W; x++) {
      const bool ap = full || rnd() % 2, cp = full || rnd() % 2;
      const uint32_t af = ap ? (RF_PRESENT | (rnd() % 2 ? RF_STOP : 0) | (rnd() % 2 ? 0x10u : 0u)) : (rnd() & 0xfeu);
      const uint32_t cf = cp ? (RF_PRESENT | (rnd() % 2 ? RF_STOP : 0) | (rnd() % 2 ? RF_HASVALUE : 0) | (rnd() % 2 ? 0x20u : 0u)) : (rnd() & 0xfeu);
      S.acc_ring[x * Gq + g] = mk4(ap ? (int32_t)(rnd() % 1000u) * W + x : junk(), ap ? (int32_t)(rnd() % 9) : junk(), ap ? ME : junk(),
                                   (int32_t)(af | (cf << CF_SHIFT) | ((rnd() & 0xffu) << 16)));
      S.com_ring[x * Gq + g] = cp ? mk4((int32_t)(rnd() % 1000u) * W + x, (int32_t)(rnd() % 9), ME, (int32_t)rnd()) : mk4(junk(), junk(), junk(), junk());
    }
    if (elect) {
      S.c_wait[g] = prep ? rnd() & 7u : (uint32_t)junk();
      for (int32_t x = 0; x < W; x++) {
        const bool cop = prep && (full || rnd() % 2);
        S.co_ring[x * Gq + g] = cop ? mk4((int32_t)(rnd() % 1000u) * W + x, (int32_t)(rnd() % 9), ME, (int32_t)(CO_PRESENT | (rnd() & 3u) | (rnd() % 2 ? 0x200u : 0u)))
                                    : mk4(junk(), junk(), junk(), junk() & ~CO_PRESENT);
        S.co_handle[x * Gq + g] = ((int64_t)junk() << 32) | (uint32_t)junk();
        S.p_handle[x * Gq + g] = ((int64_t)junk() << 32) | (uint32_t)junk();
      }
    }
    S.g_flags[g] = GF_EXISTS | (rnd() % 4 == 0 ? GF_STOPPED : 0u) | (hc ? GF_HASCOORD : 0u) | (prep ? GF_PREPARING : 0u) | ((uint32_t)kk << 8);
    names.exists[g] = 1, names.version[g] = S.g_version[g];
  }
  void kill(int32_t g) { S.g_flags[g] = 0, names.exists[g] = 0; }

  /* include/gpx_image.h, restated: the rows of live group g, padding included */
  Rows canon_rows(int32_t g) const {
    const int64_t Gq = G;
    const uint32_t gf = S.g_flags[g];
    const bool hc = gf & GF_HASCOORD, prep = (gf & GF_PREPARING) && S.c_wait;
    const int32_t k = std::min<int32_t>(GF_K(gf), K);
    Rows r((prep ? 2 : 1) * (size_t)stride_w, 0);
    r[0] = 1, r[1] = 1;
    r[2] = (int32_t)(1u | ((gf & GF_STOPPED) ? 2u : 0u) | (hc ? 4u : 0u) | (prep ? 8u | 16u : 0u) | (GF_K(gf) << 8));
    r[3] = ME, r[4] = K | (W << 16), r[5] = g, r[6] = S.g_version[g];
    r[7] = S.a_slot[g], r[8] = S.a_bnum[g], r[9] = S.a_bcoord[g], r[10] = S.a_gc[g];
    if (hc) r[11] = S.c_bnum[g], r[12] = S.c_bcoord[g], r[13] = S.c_next[g], r[14] = S.c_pcount[g];
    int32_t o = 16;
    for (int32_t j = 0; j < K; j++) r[o + j] = j < k ? S.members[j * Gq + g] : 0;
    o += K;
    for (int32_t j = 0; j < K; j++) r[o + j] = (hc && j < k) ? S.node_slots[j * Gq + g] : 0;
    o += K;
    for (int32_t x = 0; x < W; x++) {
      const uint32_t e = S.p_ring[x * Gq + g];
      r[o + x] = (hc && (e & 0x10000u)) ? (int32_t)(e & 0x3ffffu) : 0;
    }
    o += W;
    for (int32_t x = 0; x < W; x++) {
      const I4 a = S.acc_ring[x * Gq + g], c = S.com_ring[x * Gq + g];
      const uint32_t af = (uint32_t)a.w & 0xffu, cf = ((uint32_t)a.w >> 8) & 0xffu;
      if (af & 1u) r[o + 4 * x] = a.x, r[o + 4 * x + 1] = a.y, r[o + 4 * x + 2] = a.z;
      r[o + 4 * x + 3] = (int32_t)(((af & 1u) ? af & 3u : 0u) | ((cf & 1u) ? (cf & 7u) << 8 : 0u));
      if (cf & 1u) r[o + 4 * W + 4 * x] = c.x, r[o + 4 * W + 4 * x + 1] = c.y, r[o + 4 * W + 4 * x + 2] = c.z, r[o + 4 * W + 4 * x + 3] = c.w;
    }
    if (prep) {
      int32_t* q = r.data() + stride_w;
      q[0] = 1, q[1] = 2, q[5] = g, q[6] = (int32_t)S.c_wait[g];
      for (int32_t x = 0; x < W; x++) {
        const I4 c = S.co_ring[x * Gq + g];
        if (c.w & 0x100) {
          q[16 + 4 * x] = c.x, q[16 + 4 * x + 1] = c.y, q[16 + 4 * x + 2] = c.z, q[16 + 4 * x + 3] = c.w & 0x103;
          const uint64_t h = (uint64_t)S.co_handle[x * Gq + g];
          q[16 + 4 * W + 2 * x] = (int32_t)(uint32_t)h, q[16 + 4 * W + 2 * x + 1] = (int32_t)(uint32_t)(h >> 32);
        }
        if (S.p_ring[x * Gq + g] & 0x10000u) {
          const uint64_t h = (uint64_t)S.p_handle[x * Gq + g];
          q[16 + 6 * W + 2 * x] = (int32_t)(uint32_t)h, q[16 + 6 * W + 2 * x + 1] = (int32_t)(uint32_t)(h >> 32);
        }
      }
    }
    return r;
  }
  /* the engine word behind word wi of row `row` of a group whose every word is live state (fill(g, 2)), and a bit of it
   * that a canonical row shows; null for the words that are no state (format, kind, my_id, shape, gidx, reserved, k) */
  int32_t* word_behind(int32_t g, int32_t row, int32_t wi, int32_t* bit) {
    const int64_t Gq = G;
    *bit = 0x40;
    if (row == 0) {
      int32_t* hdr[16] = {0, 0, 0, 0, 0, 0, S.g_version, S.a_slot, S.a_bnum, S.a_bcoord, S.a_gc, S.c_bnum, S.c_bcoord, S.c_next, S.c_pcount, 0};
      if (wi == 2) return *bit = (int32_t)GF_STOPPED, (int32_t*)&S.g_flags[g];
      if (wi < 16) return hdr[wi] ? hdr[wi] + g : nullptr;
      wi -= 16;
      if (wi < K) return &S.members[wi * Gq + g];
      wi -= K;
      if (wi < K) return &S.node_slots[wi * Gq + g];
      wi -= K;
      if (wi < W) return *bit = 1, (int32_t*)&S.p_ring[wi * Gq + g]; /* one vote: the responded mask alone */
      wi -= W;
      if (wi < 4 * W) return *bit = (wi & 3) == 3 ? RF_STOP : 0x40, &((int32_t*)&S.acc_ring[(wi >> 2) * Gq + g])[wi & 3];
      wi -= 4 * W;
      if (wi < 4 * W) return &((int32_t*)&S.com_ring[(wi >> 2) * Gq + g])[wi & 3];
      return nullptr;
    }
    if (wi == 6) return *bit = 1, (int32_t*)&S.c_wait[g];
    if (wi < 16) return nullptr;
    wi -= 16;
    if (wi < 4 * W) return *bit = (wi & 3) == 3 ? GPX_PV_STOP : 0x40, &((int32_t*)&S.co_ring[(wi >> 2) * Gq + g])[wi & 3];
    wi -= 4 * W;
    if (wi < 2 * W) return &((int32_t*)&S.co_handle[(wi >> 1) * Gq + g])[wi & 1];
    wi -= 2 * W;
    if (wi < 2 * W) return &((int32_t*)&S.p_handle[(wi >> 1) * Gq + g])[wi & 1];
    return nullptr;
  }
  /* every word of group g anywhere, as it is: what "exactly as it was" compares */
  std::vector<int64_t> raw(int32_t g) const {
    const int64_t Gq = G;
    std::vector<int64_t> v = {S.g_flags[g], S.g_version[g], S.a_slot[g], S.a_bnum[g], S.a_bcoord[g], S.a_gc[g], S.c_bnum[g], S.c_bcoord[g],
                              S.c_next[g], S.c_pcount[g], names.exists[g], names.version[g], idle.sig[g], idle.age[g], (int64_t)M.marks[g]};
    for (int32_t j = 0; j < K; j++) v.push_back(S.members[j * Gq + g]), v.push_back(S.node_slots[j * Gq + g]);
    for (int32_t x = 0; x < W; x++) {
      const I4 a = S.acc_ring[x * Gq + g], c = S.com_ring[x * Gq + g];
      for (int32_t q : {(int32_t)S.p_ring[x * Gq + g], a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w}) v.push_back(q);
      if (elect) {
        const I4 o = S.co_ring[x * Gq + g];
        for (int64_t q : {(int64_t)o.x, (int64_t)o.y, (int64_t)o.z, (int64_t)o.w, S.co_handle[x * Gq + g], S.p_handle[x * Gq + g]}) v.push_back(q);
      }
    }
    if (elect) v.push_back(S.c_wait[g]);
    return v;
  }
};

struct Exported {
  std::vector<int32_t> rows, gone, groups; /* the rows written, the gone list, the groups written */
  DeltaCounts counts;
};

/* one export call against the rules of include/gpx_delta.h */
static Exported run(const char* what, Table& T, int32_t n, const int32_t* gidx, int32_t flags, int32_t cap, int32_t cap_gone) {
  const bool evict = flags & GPX_DELTA_EVICT, full = flags & GPX_DELTA_FULL;
  const int32_t sw = T.stride_w;
  std::vector<int32_t> chg, gone;
  std::vector<Rows> chg_rows;
  int32_t n_live = 0, n_rows = 0;
  for (int32_t i = 0; i < n; i++) {
    const int32_t g = gidx ? gidx[i] : i;
    if ((uint32_t)g >= (uint32_t)T.G) continue;
    if (T.live(g)) {
      n_live++;
      Rows r = T.canon_rows(g);
      if (full || r != T.ref[g]) n_rows += (int32_t)r.size() / sw, chg.push_back(g), chg_rows.push_back(std::move(r));
    } else if (!T.ref[g].empty()) {
      gone.push_back(g);
    }
  }
  Exported want;
  for (size_t j = 0; j < chg.size(); j++) { /* the longest prefix whose rows all fit */
    if ((int64_t)want.rows.size() + (int64_t)chg_rows[j].size() > (int64_t)cap * sw) break;
    want.rows.insert(want.rows.end(), chg_rows[j].begin(), chg_rows[j].end());
    want.groups.push_back(chg[j]);
  }
  want.gone.assign(gone.begin(), gone.begin() + std::min<size_t>(gone.size(), (size_t)cap_gone));
  want.counts = DeltaCounts{n_live, (int32_t)chg.size(), n_rows, (int32_t)want.groups.size(), (int32_t)want.rows.size() / sw,
                            (int32_t)gone.size(), (int32_t)want.gone.size(), 0};
  std::vector<std::vector<int64_t>> before(T.G);
  for (int32_t g = 0; g < T.G; g++) before[g] = T.raw(g);

  int32_t* o_rows = cap ? blk<int32_t>((size_t)cap * sw, 0xA5) : nullptr;
  int32_t* o_gone = cap_gone ? blk<int32_t>(cap_gone, 0xA5) : nullptr;
  DeltaCounts* counts = blk<DeltaCounts>(1, 0xA5);
  const int ntiles = (n + GPX_IMAGE_TILE - 1) / GPX_IMAGE_TILE;
  if ((size_t)ntiles > T.tiles) fail(what, "more tiles than the table's scratch holds");
  launch(ntiles, [&] { k_delta_tile(T.S, n, gidx, 0, flags, T.M); });
  for (int32_t g = 0; g < T.G; g++) /* what fits is not known yet */
    if (T.raw(g) != before[g]) fail(what, "a mark or a group changed in the first launch", g);
  launch(1, [&] { k_delta_offsets(ntiles, T.M, cap, cap_gone, counts); });
  if (ntiles && (cap > 0 || cap_gone > 0))
    launch(ntiles, [&] { k_delta_move(T.S, T.M, T.names, T.idle, cap, cap_gone, flags, o_rows, o_gone); });

  if (memcmp(counts, &want.counts, sizeof(DeltaCounts))) {
    const DeltaCounts &a = *counts, &b = want.counts;
    printf("%s: counts %d %d %d %d %d %d %d %d, want %d %d %d %d %d %d %d %d\n", what, a.n_live, a.n_changed, a.n_rows, a.n_done,
           a.n_rows_done, a.n_gone, a.n_gone_done, a.reserved, b.n_live, b.n_changed, b.n_rows, b.n_done, b.n_rows_done, b.n_gone,
           b.n_gone_done, b.reserved);
    exit(1);
  }
  for (size_t q = 0; q < (size_t)cap * sw; q++)
    if (o_rows[q] != (q < want.rows.size() ? want.rows[q] : (int32_t)0xA5A5A5A5)) fail(what, "row word wrong or written beyond the last row", q / sw, q % sw);
  for (int32_t q = 0; q < cap_gone; q++)
    if (o_gone[q] != (q < (int32_t)want.gone.size() ? want.gone[q] : (int32_t)0xA5A5A5A5)) fail(what, "gone entry", q, o_gone[q]);
  /* marks and state: the groups written take their rows as mark (EVICT: die, mark 0, idle words 0), the gone ones
   * written lose theirs, nothing else anywhere changes */
  std::vector<char> wr(T.G, 0), gn(T.G, 0);
  for (size_t j = 0; j < want.groups.size(); j++) {
    const int32_t g = want.groups[j];
    wr[g] = 1;
    if (evict) T.ref[g].clear();
    else T.ref[g].assign(chg_rows[j].begin(), chg_rows[j].end());
  }
  for (int32_t g : want.gone) gn[g] = 1, T.ref[g].clear();
  for (int32_t g = 0; g < T.G; g++) {
    std::vector<int64_t> now = T.raw(g), was = before[g];
    if ((T.M.marks[g] != 0) != !T.ref[g].empty()) fail(what, "mark zero / non-zero", g, (long)T.M.marks[g]);
    if (wr[g] || gn[g]) was[14] = now[14];
    if (wr[g] && evict) {
      if (now[0] != 0 || now[10] != 0 || now[12] != 0 || now[13] != 0) fail(what, "an evicted group lives on", g);
      was[0] = was[10] = was[12] = was[13] = 0;
    }
    if (now != was) fail(what, "a word of a group, its mark or its idle words changed", g);
  }
  printf("%s: ok, %d live, %d changed (%d rows), %d written (%d rows), %d gone, %d listed\n", what, n_live, (int)chg.size(), n_rows,
         want.counts.n_done, want.counts.n_rows_done, want.counts.n_gone, want.counts.n_gone_done);
  free(o_rows), free(o_gone), free(counts);
  return want;
}

/* one apply call: rows / gidx as the call takes them, the statuses the rules of include/gpx_image.h and gpx_delta.h give */
static void apply(const char* what, Table& T, const std::vector<int32_t>& rows, const int32_t* gidx, const std::vector<uint8_t>& want_st,
                  const std::vector<int32_t>& gone) {
  const int32_t sw = T.stride_w, n_rows = (int32_t)rows.size() / sw, n_gone = (int32_t)gone.size();
  std::vector<std::vector<int64_t>> before(T.G);
  for (int32_t g = 0; g < T.G; g++) before[g] = T.raw(g);
  int32_t* d_rows = blk<int32_t>(rows.size(), 0);
  memcpy(d_rows, rows.data(), rows.size() * 4);
  int32_t* d_gone = blk<int32_t>(n_gone, 0);
  if (n_gone) memcpy(d_gone, gone.data(), gone.size() * 4);
  uint8_t *st = blk<uint8_t>(n_rows, 0xA5), *gst = blk<uint8_t>(n_gone, 0xA5);
  const int ntiles = (n_rows + GPX_IMAGE_TILE - 1) / GPX_IMAGE_TILE;
  if ((size_t)ntiles > 2 * T.tiles) fail(what, "more rows than the table's scratch holds");
  launch(ntiles, [&] { k_delta_rows<false>(T.S, T.IM, T.names, T.idle, n_rows, d_rows, gidx, st); });
  for (int32_t g = 0; g < T.G; g++)
    if (T.raw(g) != before[g]) fail(what, "the checking pass wrote state", g);
  launch(ntiles, [&] { k_delta_rows<true>(T.S, T.IM, T.names, T.idle, n_rows, d_rows, gidx, st); });
  launch((n_gone + GPX_BLOCK - 1) / GPX_BLOCK, [&] { k_delta_gone(T.S, T.names, T.idle, n_gone, d_gone, gst); });
  std::vector<char> touched(T.G, 0);
  int taken = 0;
  for (int32_t j = 0; j < n_rows; j++) {
    if (st[j] != want_st[j]) fail(what, "status", j, st[j]);
    const int32_t* r = &rows[(size_t)j * sw];
    if (st[j] != GPX_S_OK || r[1] != GPX_IMAGE_MAIN) continue;
    const int32_t dest = gidx ? gidx[j] : r[5];
    const bool cont = (r[2] & GPX_IMG_F_CONTINUED) != 0;
    Rows now = T.canon_rows(dest), in(r, r + (cont ? 2 : 1) * sw);
    in[5] = dest;
    if (cont) in[sw + 5] = dest;
    if (now != in) fail(what, "the group taken is not the group of the rows", j, dest);
    if (!T.names.exists[dest] || T.names.version[dest] != r[6] || T.idle.sig[dest] || T.idle.age[dest]) fail(what, "the copies or the idle words of a group taken", dest);
    if (!cont && T.elect) { /* the election words are the group's too */
      bool z = T.S.c_wait[dest] == 0;
      for (int32_t x = 0; x < T.W; x++) {
        const I4 c = T.S.co_ring[(int64_t)x * T.G + dest];
        z = z && !(c.x | c.y | c.z | c.w) && !T.S.co_handle[(int64_t)x * T.G + dest] && !T.S.p_handle[(int64_t)x * T.G + dest];
      }
      if (!z) fail(what, "election words left behind under a group without an election", dest);
    }
    touched[dest] = 1, taken++;
  }
  int retired = 0;
  for (int32_t i = 0; i < n_gone; i++) {
    const int32_t g = gone[i];
    const bool ok = (uint32_t)g < (uint32_t)T.G && (before[g][0] & GF_EXISTS);
    if (gst[i] != (ok ? GPX_S_OK : GPX_S_NOGROUP)) fail(what, "gone status", i, gst[i]);
    if (!ok) continue;
    std::vector<int64_t> was = before[g];
    was[0] = was[10] = was[12] = was[13] = 0;
    if (T.raw(g) != was) fail(what, "a retired group", g);
    touched[g] = 1, retired++;
  }
  for (int32_t g = 0; g < T.G; g++)
    if (!touched[g] && T.raw(g) != before[g]) fail(what, "a group no row was taken for changed: a refused row wrote", g);
  printf("%s: ok, %d rows, %d groups taken, %d retired of %d\n", what, n_rows, taken, retired, n_gone);
  free(d_rows), free(d_gone), free(st), free(gst);
}

static void shape(int32_t K, int32_t W) {
  const int32_t T = GPX_IMAGE_TILE, G = 3 * T + 17;
  char w[120];
  auto name = [&](const char* s) { return snprintf(w, sizeof w, "K%d W%d %s", K, W, s), w; };
  // every changed set on three tiles: baseline, nothing happened, state words change in the set, stale words everywhere
  std::vector<uint8_t> none(G, 0), all(G, 1), edges(G, 0), hole(G, 0), sparse(G, 0);
  for (int g : {0, 63, 64, 255, 256, T - 1, T, 2 * T - 1, 2 * T, 3 * T - 1, 3 * T, 3 * T + 16}) edges[g] = 1;
  for (int g = 0; g < T; g++) hole[g] = hole[2 * T + g] = 1;
  for (int g = 0; g < G; g++) sparse[g] = (g * 2654435761u >> 7) % 97 == 0;
  const char* names[] = {"all", "none", "sparse", "edges", "hole"};
  const std::vector<uint8_t>* hs[] = {&all, &none, &sparse, &edges, &hole};
  for (int s = 0; s < 5; s++) {
    Table t(G + 8, K, W, true, 4);
    for (int g = 0; g < G; g++)
      if (g % 13 != 5 || (*hs[s])[g]) t.fill(g);
    char v[160];
    snprintf(v, sizeof v, "%s: count only", name(names[s]));
    run(v, t, G + 8, nullptr, 0, 0, 0);
    snprintf(v, sizeof v, "%s: first export", name(names[s]));
    if (run(v, t, G + 8, nullptr, 0, 2 * G, G).counts.n_changed == 0) fail(v, "nothing to write");
    snprintf(v, sizeof v, "%s: nothing happened", name(names[s]));
    if (run(v, t, G + 8, nullptr, 0, 2 * G, G).counts.n_changed != 0) fail(v, "changed");
    for (int g = 0; g < G; g++) {
      if ((*hs[s])[g]) {
        t.fill(g); /* a new state (the version alone makes it another one) */
        t.S.g_version[g] += 8;
      } else if (t.live(g)) { /* only words the state does not define */
        const std::vector<int64_t> was = t.raw(g);
        Rows r0 = t.canon_rows(g);
        for (int x = 0; x < W; x++) {
          I4& a = t.S.acc_ring[(int64_t)x * t.G + g];
          if (!(a.w & RF_PRESENT)) a.x = junk(), a.y = junk(), a.w ^= 0x10;
          if (!((a.w >> CF_SHIFT) & RF_PRESENT)) t.S.com_ring[(int64_t)x * t.G + g].w = junk();
          if (!(t.S.p_ring[(int64_t)x * t.G + g] & PR_PRESENT)) t.S.p_ring[(int64_t)x * t.G + g] ^= 0x41u;
          t.S.p_ring[(int64_t)x * t.G + g] ^= 0x80000u;
          if (!(t.S.g_flags[g] & GF_PREPARING)) t.S.co_ring[(int64_t)x * t.G + g].x = junk(), t.S.p_handle[(int64_t)x * t.G + g] = junk();
        }
        if (!(t.S.g_flags[g] & GF_HASCOORD)) t.S.c_next[g] = junk(), t.S.node_slots[g] = junk();
        if (GF_K(t.S.g_flags[g]) < (uint32_t)K) t.S.members[(int64_t)(K - 1) * t.G + g] = junk();
        if (t.raw(g) == was || t.canon_rows(g) != r0) fail(v, "the stale words of the test");
      }
    }
    snprintf(v, sizeof v, "%s: delta", name(names[s]));
    Exported e = run(v, t, G + 8, nullptr, 0, 2 * G, G);
    if (e.counts.n_changed != (int32_t)std::count(hs[s]->begin(), hs[s]->end(), 1)) fail(v, "the changed set");
    snprintf(v, sizeof v, "%s: FULL", name(names[s]));
    if (run(v, t, G + 8, nullptr, GPX_DELTA_FULL, 2 * G, G).counts.n_done != e.counts.n_live) fail(v, "a baseline writes every live group");
    snprintf(v, sizeof v, "%s: after", name(names[s]));
    if (run(v, t, G + 8, nullptr, 0, 2 * G, G).counts.n_changed != 0) fail(v, "changed");
  }
  // every word of both rows, one group each: a word the signature left out is a change nobody reports
  {
    const int32_t rw = image_row_words(K, W), cw = 16 + 8 * W;
    Table t(G, K, W, true, 4);
    for (int g = 0; g < G; g++) t.fill(g, 2);
    run(name("words: baseline"), t, G, nullptr, 0, 2 * G, 0);
    int32_t expect = 0;
    for (int g = 0; g < G; g++) {
      const int32_t wi = g % (rw + cw);
      int32_t bit;
      int32_t* p = t.word_behind(g, wi >= rw, wi >= rw ? wi - rw : wi, &bit);
      if (!p) continue;
      Rows r0 = t.canon_rows(g);
      *p ^= bit;
      Rows r1 = t.canon_rows(g);
      int32_t d = 0, at = -1;
      for (size_t q = 0; q < r0.size(); q++)
        if (r0[q] != r1[q]) d++, at = (int32_t)q;
      if (d != 1 || at != (wi >= rw ? t.stride_w + wi - rw : wi)) fail("words", "the test's own map of the rows", g, at);
      expect++;
    }
    if (run(name("words: one word each"), t, G, nullptr, 0, 2 * G, 0).counts.n_changed != expect || expect < G / 2) fail("words", "changed", expect);
  }
  // caps: inside a tile, on a tile's edge, one row short of a two-row group; repeated calls until nothing is left
  {
    Table t(G, K, W, true, 4);
    for (int g = 0; g < G; g++) t.fill(g, g % 3 == 1 ? 2 : g % 2);
    std::vector<int32_t> need(G + 1, 0); /* rows before group g */
    for (int g = 0; g < G; g++) need[g + 1] = need[g] + (g % 3 == 1 ? 2 : 1);
    run(name("caps: cap 0 counts"), t, G, nullptr, 0, 0, 0);
    if (run(name("caps: inside tile 0"), t, G, nullptr, 0, need[100], 0).counts.n_done != 100) fail("caps", "inside a tile");
    if (run(name("caps: on the edge of tile 0"), t, G, nullptr, 0, need[T] - need[100], 0).counts.n_done != T - 100) fail("caps", "on an edge");
    /* group T + 3 needs two rows and one is left: it and the one-row groups behind it stay */
    Exported e = run(name("caps: between a group's two rows"), t, G, nullptr, 0, need[T + 4] - need[T] - 1, 0);
    if (e.counts.n_done != 3 || e.counts.n_rows_done != 4) fail("caps", "between two rows", e.counts.n_done);
    e = run(name("caps: exactly tile 1 and half of tile 2"), t, G, nullptr, 0, need[2 * T + 77] - need[T + 3], 0);
    if (e.counts.n_done != T + 74) fail("caps", "across an edge", e.counts.n_done);
    int calls = 0;
    while (run(name("caps: the rest, 50 rows a call"), t, G, nullptr, 0, 50, 0).counts.n_changed > 0)
      if (++calls > 20) fail("caps", "does not end");
  }
  // gone: dead groups that carry a mark, cap_gone cuts; a dead group without a mark is nothing
  {
    Table t(G, K, W, true, 4);
    for (int g = 0; g < G; g++)
      if (g % 5) t.fill(g);
    run(name("gone: baseline"), t, G, nullptr, 0, 2 * G, 0);
    int32_t dead = 0;
    for (int g = 0; g < G; g += 3)
      if (t.live(g)) t.kill(g), dead++;
    if (run(name("gone: counted"), t, G, nullptr, 0, 0, 0).counts.n_gone != dead) fail("gone", "count");
    if (run(name("gone: cap_gone 0, rows only"), t, G, nullptr, 0, 2 * G, 0).counts.n_gone != dead) fail("gone", "count");
    run(name("gone: cap_gone 1"), t, G, nullptr, 0, 0, 1);
    run(name("gone: cap_gone inside tile 0"), t, G, nullptr, 0, 0, 40);
    run(name("gone: cap_gone into tile 2"), t, G, nullptr, 0, 0, (dead - 41) * 3 / 4);
    if (run(name("gone: the rest"), t, G, nullptr, 0, 2 * G, G).counts.n_gone_done != dead - 41 - (dead - 41) * 3 / 4) fail("gone", "rest");
    if (run(name("gone: none left"), t, G, nullptr, 0, 2 * G, G).counts.n_gone != 0) fail("gone", "reported twice");
    for (int g = 0; g < G; g += 3) t.fill(g); /* created again: changed, not gone */
    Exported e = run(name("gone: created again"), t, G, nullptr, 0, 2 * G, G);
    if (e.counts.n_gone != 0 || e.counts.n_changed != (G + 2) / 3) fail("gone", "created again");
  }
  // EVICT: the groups written die, with their marks; not gone afterwards; a cut leaves the rest alive
  {
    Table t(G, K, W, true, 4);
    for (int g = 0; g < G; g++) t.fill(g, g % 3 == 1 ? 2 : g % 2);
    run(name("evict: baseline"), t, G, nullptr, 0, 2 * G, 0);
    for (int g = 0; g < G; g += 2) t.S.a_slot[g] += 1;
    Exported e = run(name("evict: cut inside tile 1"), t, G, nullptr, GPX_DELTA_EVICT, 250, 0);
    if (e.counts.n_done == 0 || e.counts.n_done >= e.counts.n_changed) fail("evict", "cut");
    e = run(name("evict: the rest"), t, G, nullptr, GPX_DELTA_EVICT, 2 * G, G);
    if (e.counts.n_gone != 0 || e.counts.n_done != e.counts.n_changed) fail("evict", "rest");
    e = run(name("evict: after"), t, G, nullptr, 0, 2 * G, G);
    if (e.counts.n_changed != 0 || e.counts.n_gone != 0 || e.counts.n_live != G / 2) fail("evict", "after");
    run(name("evict: FULL | EVICT"), t, G, nullptr, GPX_DELTA_FULL | GPX_DELTA_EVICT, 2 * G, G);
    if (run(name("evict: empty table"), t, G, nullptr, 0, 2 * G, G).counts.n_live != 0) fail("evict", "empty");
  }
  // listed: unordered, partial, with dead and out-of-range entries; unlisted groups keep their marks
  {
    Table t(G, K, W, true, 4);
    for (int g = 0; g < G; g++)
      if (g % 11 != 3) t.fill(g);
    std::vector<int32_t> lst;
    for (int i = 0; i < 531; i++) lst.push_back(i % 97 == 5 ? -1 - i : i % 89 == 7 ? G + i : (int32_t)(((int64_t)i * 37) % G));
    run(name("listed: first"), t, (int32_t)lst.size(), lst.data(), 0, 2 * G, G);
    if (run(name("listed: again"), t, (int32_t)lst.size(), lst.data(), 0, 2 * G, G).counts.n_changed != 0) fail("listed", "changed");
    for (int g = 0; g < G; g += 7)
      if (t.live(g)) g % 2 ? t.kill(g) : t.fill(g);
    run(name("listed: delta, cap 20 and cap_gone 3"), t, (int32_t)lst.size(), lst.data(), 0, 20, 3);
    run(name("listed: n = 5"), t, 5, lst.data() + 100, GPX_DELTA_FULL, 10, 5);
    run(name("n = 0"), t, 0, nullptr, 0, 0, 0);
    run(name("listed: the table"), t, G, nullptr, 0, 2 * G, G);
  }
  // apply: onto free rows, onto live ones (replaced), rows that are refused, the gone list
  {
    Table a(G, K, W, true, 4), b(G, K, W, true, 4), c(G, K, W, false, 4);
    for (int g = 0; g < G; g++) {
      if (g % 7 != 2) a.fill(g);
      if (g % 3 != 1) b.fill(g); /* other groups, other states, election words in use */
      if (g % 3 != 1) c.fill(g);
    }
    Exported e = run(name("apply: the source's baseline"), a, G, nullptr, GPX_DELTA_FULL, 2 * G, 0);
    std::vector<uint8_t> ok(e.rows.size() / a.stride_w, GPX_S_OK);
    std::vector<int32_t> gone;
    for (int g = 0; g < G; g++)
      if (g % 7 == 2) gone.push_back(g);
    gone.push_back(-3), gone.push_back(G);
    apply(name("apply: onto a table of other groups"), b, e.rows, nullptr, ok, gone);
    for (int g = 0; g < G; g++)
      if (b.live(g) != a.live(g) || (a.live(g) && b.canon_rows(g) != a.canon_rows(g))) fail("apply", "the mirror differs", g);
    /* refusals: a wrong format word, a non-canonical word, a main row that lost its continuation, a continuation row
     * alone, a destination out of range - each aimed at a live group - between rows that are taken */
    std::vector<int32_t> rows = e.rows;
    std::vector<uint8_t> want = ok;
    std::vector<int32_t> dest(want.size());
    const int32_t sw = a.stride_w;
    for (auto* tb : {&b, &c}) { /* with and without the election arrays */
      rows = e.rows, want = ok;
      for (size_t j = 0; j < want.size(); j++) dest[j] = (int32_t)((rows[j * sw + 5] + 1) % G); /* every group one row on */
      int32_t mains = 0, refused = 0;
      for (size_t j = 0; j < want.size(); j++) {
        int32_t* r = &rows[j * sw];
        const bool two = r[1] == GPX_IMAGE_MAIN && (r[2] & GPX_IMG_F_CONTINUED);
        if (r[1] == GPX_IMAGE_CONT) {
          if (!tb->elect) want[j] = want[j - 1] = GPX_S_IMAGE; /* no election arrays, no GPX_IMG_VIEWCHANGE */
          continue;
        }
        switch (mains++ % 9) {
          case 1: r[0] = 7, want[j] = GPX_S_IMAGE; break;
          case 3: r[15] = 1, want[j] = GPX_S_IMAGE; break;
          case 5: dest[j] = G + 5, want[j] = GPX_S_NOGROUP; break;
          case 7: r[16 + 2 * K + W + 3] ^= 0x40 << 8, want[j] = GPX_S_IMAGE; break; /* an unknown bit in a ring's flag word */
          default: break;
        }
        if (two && want[j] != GPX_S_OK) want[j + 1] = want[j];
        if (two && want[j] == GPX_S_OK && mains % 4 == 0) rows[(j + 1) * sw + 5] ^= 1, want[j] = want[j + 1] = GPX_S_IMAGE; /* not its row */
        refused += want[j] != GPX_S_OK;
      }
      if (refused < 50) fail("apply", "the test refuses too little", refused);
      apply(name(tb->elect ? "apply: replace and refuse" : "apply: replace and refuse, no election arrays"), *tb, rows, dest.data(), want, {});
    }
  }
}

int main() {
  shape(3, 8);
  shape(8, 4);
  // many tiles: more than one round of k_delta_offsets, caps that cut far in
  {
    const int32_t big = 257 * GPX_IMAGE_TILE + 1;
    Table t(big, 3, 8, true, 258);
    for (int g = 0; g < big; g++)
      if ((g * 2654435761u >> 9) % 5 == 0) t.fill(g);
    run("258 tiles: baseline, cap = half", t, big, nullptr, 0, big / 10, 0);
    for (int g = 0; g < big; g += 17)
      if (t.live(g)) g % 2 ? t.kill(g) : t.fill(g);
    run("258 tiles: the rest and the delta", t, big, nullptr, 0, big, 100);
    if (run("258 tiles: after", t, big, nullptr, 0, big, big).counts.n_changed != 0) fail("258 tiles", "changed");
  }
  return 0;
}
