// Lockstep CPU emulation of the kernels of gigapaxos_amd/csrc/gpx_checkpoint.hip.h (tests/test_checkpoint_abi.py
// compiles and runs this with AddressSanitizer and UBSan): the real header, unmodified, over stand-ins for what it takes
// from gpx_kernels.hip.h - the ring view, the collection and reconstructDecision, written here straight from the Java
// (whole-ring scans, no narrow walks).  One std::thread per lane of a workgroup, barriers for __syncthreads and for the
// wave collectives, one workgroup at a time.  The scratch starts as garbage and lives on from call to call; every
// buffer is a heap block of its exact size, so an index past an end is a sanitizer report.
//
// The cases and the expected answers come from the Java reading, tests/checkpoint_model.py: argv[1] is a file of
// integers the test wrote - tables (group words and both rings), calls (records, peek or not) and, per call, every dense
// output, the runs, the counts and the table afterwards.  Ring entries are compared by what is live: the flag word
// whole, an entry's other words where its presence bit is set.  What this cannot show is what only the GPU has: the
// compiler's code, memory ordering between launches, and the real helpers (tests/test_checkpoint_gpu.py).
#include <algorithm>
#include <barrier>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "lockstep_runtime.h"

// ---- what the kernels take from include/gpx.h and gpx_kernels.hip.h ----
#define GPX_S_OK 0
#define GPX_S_NOGROUP 1
#define GPX_S_STOPPED 2
#define GPX_F_ACCEPTS_FROM_DISK 1u
#define GF_EXISTS 1u
#define GF_STOPPED 2u
#define RF_PRESENT 1
#define RF_STOP 2
#define RF_HASVALUE 4
#define AF_MASK 0xffu
#define CF_SHIFT 8
#define CF_MASK 0xff00u
struct alignas(16) I4 { int32_t x, y, z, w; };
static I4 mk4(int32_t x, int32_t y, int32_t z, int32_t w) { return I4{x, y, z, w}; }
struct DevState {
  int32_t G, W;
  uint32_t flags;
  uint32_t* g_flags;
  int32_t *a_slot, *a_gc;
  I4 *acc_ring, *com_ring;
};
static int32_t jsub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
static int32_t ballot_cmp(int32_t n1, int32_t c1, int32_t n2, int32_t c2) { return n1 != n2 ? jsub(n1, n2) : jsub(c1, c2); }
struct AccState { int32_t slot, bnum, bcoord, gc; bool stopped; };
// the ring of one group; ONE cached entry, the preset one, so that a wrong preset shows
struct AccView {
  I4* ring; int64_t G; int32_t g, pw; I4 pv;
  void init(const DevState& S, int32_t g_) { ring = S.acc_ring, G = S.G, g = g_, pw = -1, pv = I4{0, 0, 0, 0}; }
  void preset(int32_t w, const I4& v) { pw = w, pv = v; }
  I4 rd(int32_t w) { return w == pw ? pv : ring[(int64_t)w * G + g]; }
  void wr_flags(int32_t w, int32_t f) {
    ring[(int64_t)w * G + g].w = f;
    if (w == pw) pv.w = f;
  }
};
// PaxosAcceptor.garbageCollectAccepted and garbageCollectDecisions (PaxosAcceptor.java:476-506) as written
static void acc_gc(const DevState& S, AccView& V, AccState& a, int32_t gcSlot) {
  if (jsub(a.slot, gcSlot) <= 0) gcSlot = jsub(a.slot, 1);
  if (jsub(gcSlot, a.gc) > 0) {
    a.gc = gcSlot;
    for (int32_t w = 0; w < S.W; w++) {
      const I4 e = V.rd(w);
      if ((e.w & RF_PRESENT) && jsub(e.x, gcSlot) <= 0) V.wr_flags(w, e.w & ~(int32_t)AF_MASK);
    }
  }
  if (jsub(gcSlot, a.slot) >= 0) return;
  for (int32_t w = 0; w < S.W; w++) {
    const I4 e = V.rd(w);
    if ((((uint32_t)e.w >> CF_SHIFT) & RF_PRESENT) && jsub(gcSlot, S.com_ring[(int64_t)w * S.G + V.g].x) > 0)
      V.wr_flags(w, e.w & ~(int32_t)CF_MASK);
  }
}
struct Dec { int32_t bnum, bcoord, slot, median; bool has_value, stop; };
// PaxosAcceptor.reconstructDecision (PaxosAcceptor.java:369-385)
static bool acc_reconstruct(const DevState& S, AccView& V, int32_t g, int32_t slot, Dec* out) {
  const int32_t w = slot & (S.W - 1);
  const I4 ar = V.rd(w), cr = S.com_ring[(int64_t)w * S.G + g];
  const uint32_t cf = ((uint32_t)ar.w >> CF_SHIFT) & 0xffu, af = (uint32_t)ar.w & AF_MASK;
  if (!(cf & RF_PRESENT) || cr.x != slot) return false;
  if (cf & RF_HASVALUE) {
    *out = Dec{cr.y, cr.z, slot, cr.w, true, (cf & RF_STOP) != 0};
    return true;
  }
  if ((af & RF_PRESENT) && ar.x == slot && ballot_cmp(ar.y, ar.z, cr.y, cr.z) == 0) {
    *out = Dec{ar.y, ar.z, slot, cr.w, true, (af & RF_STOP) != 0};
    return true;
  }
  return false;
}
static void acc_store(const DevState& S, int32_t g, uint32_t gf, const AccState& a, const AccState& a0) {
  if (a.bnum != a0.bnum || a.bcoord != a0.bcoord) {
    printf("the ballot of group %d changed\n", g);
    exit(1);
  }
  if (a.slot != a0.slot) S.a_slot[g] = a.slot;
  if (a.gc != a0.gc) S.a_gc[g] = a.gc;
  if (a.stopped && !(gf & GF_STOPPED)) S.g_flags[g] = gf | GF_STOPPED;
}

#include "gpx_compact.hip.h"
#include "gpx_checkpoint.hip.h"


static FILE* g_in;
static long rd() {
  long v;
  if (fscanf(g_in, "%ld", &v) != 1) {
    printf("the case file ends early\n");
    exit(1);
  }
  return v;
}

struct Table {
  int32_t G, W;
  uint32_t flags;
  uint32_t* gf;
  int32_t *slot, *gc;
  I4 *acc, *com;
  void read_into(uint32_t* f, int32_t* s, int32_t* c, I4* a, I4* m) const {
    for (int32_t g = 0; g < G; g++) {
      f[g] = (uint32_t)rd(), s[g] = (int32_t)rd(), c[g] = (int32_t)rd();
      const int32_t live = (int32_t)rd(); /* ring indices that follow; the others are empty */
      for (int32_t w = 0; w < W; w++) a[(int64_t)w * G + g] = I4{0, 0, 0, 0}, m[(int64_t)w * G + g] = I4{0, 0, 0, 0};
      for (int32_t q = 0; q < live; q++) {
        const int32_t w = (int32_t)rd();
        I4 e, k;
        e.x = (int32_t)rd(), e.y = (int32_t)rd(), e.z = (int32_t)rd(), e.w = (int32_t)rd();
        k.x = (int32_t)rd(), k.y = (int32_t)rd(), k.z = (int32_t)rd(), k.w = (int32_t)rd();
        a[(int64_t)w * G + g] = e, m[(int64_t)w * G + g] = k;
      }
    }
  }
};

static void fail(const char* what, const char* msg, long a = 0, long b = 0, long c = 0) {
  printf("%s: %s (%ld, %ld, %ld)\n", what, msg, a, b, c);
  exit(1);
}

int main(int argc, char** argv) {
  if (argc < 2 || !(g_in = fopen(argv[1], "r"))) return 2;
  const int nlegs = (int)rd();
  for (int leg = 0; leg < nlegs; leg++) {
    Table T;
    T.G = (int32_t)rd(), T.W = (int32_t)rd(), T.flags = (uint32_t)rd();
    const size_t ring = (size_t)T.G * T.W;
    T.gf = blk<uint32_t>(T.G, 0), T.slot = blk<int32_t>(T.G, 0), T.gc = blk<int32_t>(T.G, 0);
    T.acc = blk<I4>(ring, 0), T.com = blk<I4>(ring, 0);
    T.read_into(T.gf, T.slot, T.gc, T.acc, T.com);
    const int32_t max_n = (int32_t)rd(); /* the largest call of the leg: sizes the scratch, in whole tiles */
    const size_t tiles = std::max<size_t>(((size_t)max_n + GPX_CP_TILE - 1) / GPX_CP_TILE, 1);
    CpMem M;
    M.park_g = blk<int32_t>(tiles * GPX_CP_TILE, 0xEE), M.park_first = blk<int32_t>(tiles * GPX_CP_TILE, 0xEE);
    M.park_count = blk<int32_t>(tiles * GPX_CP_TILE, 0xEE), M.tile = blk<I4>(tiles, 0xEE);
    DevState S{T.G, T.W, T.flags, T.gf, T.slot, T.gc, T.acc, T.com};
    const int ncalls = (int)rd();
    for (int call = 0; call < ncalls; call++) {
      char what[64];
      snprintf(what, sizeof what, "leg %d call %d", leg, call);
      const int32_t n = (int32_t)rd(), peek = (int32_t)rd();
      int32_t *gidx = blk<int32_t>(n, 0), *cp = blk<int32_t>(n, 0);
      for (int32_t i = 0; i < n; i++) gidx[i] = (int32_t)rd(), cp[i] = (int32_t)rd();
      int32_t *o_from = blk<int32_t>(n, 0xA5), *o_to = blk<int32_t>(n, 0xA5);
      uint8_t *o_fl = blk<uint8_t>(n, 0xA5), *o_st = blk<uint8_t>(n, 0xA5);
      int32_t *x_g = blk<int32_t>(n, 0xA5), *x_f = blk<int32_t>(n, 0xA5), *x_c = blk<int32_t>(n, 0xA5);
      CpCounts* counts = blk<CpCounts>(1, 0xA5);
      /* the state before, for a peek */
      std::vector<uint32_t> gf0(T.gf, T.gf + T.G);
      std::vector<int32_t> sl0(T.slot, T.slot + T.G), gc0(T.gc, T.gc + T.G);
      std::vector<I4> acc0(T.acc, T.acc + ring), com0(T.com, T.com + ring);
      const int ntiles = (n + GPX_CP_TILE - 1) / GPX_CP_TILE;
      if ((size_t)ntiles > tiles) fail(what, "more tiles than the leg's scratch holds");
      if (ntiles && peek) launch(ntiles, [&] { k_cp_tile<true>(S, n, gidx, cp, o_from, o_to, o_fl, o_st, M); });
      if (ntiles && !peek) launch(ntiles, [&] { k_cp_tile<false>(S, n, gidx, cp, o_from, o_to, o_fl, o_st, M); });
      launch(1, [&] { k_cp_offsets(ntiles, M, counts); });
      if (ntiles && !peek) launch(ntiles, [&] { k_cp_move(M, x_g, x_f, x_c); });
      /* dense outputs */
      for (int32_t i = 0; i < n; i++) {
        const long st = rd(), from = rd(), to = rd(), fl = rd();
        if (o_st[i] != st || o_from[i] != from || o_to[i] != to || o_fl[i] != fl) {
          printf("%s: record %d (group %d, cp %d): got status %d from %d to %d flags %d, the model gives %ld %ld %ld %ld\n", what,
                 i, gidx[i], cp[i], o_st[i], o_from[i], o_to[i], o_fl[i], st, from, to, fl);
          exit(1);
        }
      }
      const int32_t nruns = (int32_t)rd();
      for (int32_t j = 0; j < n; j++) {
        if (j < nruns) {
          const long g = rd(), f = rd(), c = rd();
          if (x_g[j] != g || x_f[j] != f || x_c[j] != c) fail(what, "run wrong", j, x_g[j], x_f[j]);
        } else if (x_g[j] != (int32_t)0xA5A5A5A5 || x_f[j] != (int32_t)0xA5A5A5A5 || x_c[j] != (int32_t)0xA5A5A5A5) {
          fail(what, "run column written at or beyond n_runs", j);
        }
      }
      const long ca = rd(), cn = rd(), cs = rd(), cr = rd();
      if (counts->n_adopted != ca || counts->n_nogroup != cn || counts->n_stopped != cs || counts->n_runs != cr ||
          cr != nruns) {
        printf("%s: counts %d %d %d %d, the model gives %ld %ld %ld %ld\n", what, counts->n_adopted, counts->n_nogroup,
               counts->n_stopped, counts->n_runs, ca, cn, cs, cr);
        exit(1);
      }
      if (peek) {
        if (memcmp(gf0.data(), T.gf, T.G * 4) || memcmp(sl0.data(), T.slot, T.G * 4) || memcmp(gc0.data(), T.gc, T.G * 4) ||
            memcmp(acc0.data(), T.acc, ring * sizeof(I4)) || memcmp(com0.data(), T.com, ring * sizeof(I4)))
          fail(what, "a peek changed a byte of state");
      } else {
        /* the table afterwards, by what is live */
        uint32_t* wf = blk<uint32_t>(T.G, 0);
        int32_t *ws = blk<int32_t>(T.G, 0), *wc = blk<int32_t>(T.G, 0);
        I4 *wa = blk<I4>(ring, 0), *wm = blk<I4>(ring, 0);
        T.read_into(wf, ws, wc, wa, wm);
        for (int32_t g = 0; g < T.G; g++) {
          if (T.gf[g] != wf[g] || T.slot[g] != ws[g] || T.gc[g] != wc[g]) fail(what, "group words", g, T.slot[g], T.gc[g]);
          for (int32_t w = 0; w < T.W; w++) {
            const I4 e = T.acc[(int64_t)w * T.G + g], k = T.com[(int64_t)w * T.G + g];
            const I4 we = wa[(int64_t)w * T.G + g], wk = wm[(int64_t)w * T.G + g];
            if (e.w != we.w) fail(what, "ring flags", g, w, e.w);
            if ((e.w & RF_PRESENT) && (e.x != we.x || e.y != we.y || e.z != we.z)) fail(what, "accepted entry", g, w);
            if (((e.w >> CF_SHIFT) & RF_PRESENT) && memcmp(&k, &wk, sizeof k)) fail(what, "committed entry", g, w);
          }
        }
        free(wf), free(ws), free(wc), free(wa), free(wm);
      }
      printf("%s: ok, n %d%s, adopted %d, no group %d, stopped %d, runs %d\n", what, n, peek ? " (peek)" : "",
             counts->n_adopted, counts->n_nogroup, counts->n_stopped, counts->n_runs);
      free(gidx), free(cp), free(o_from), free(o_to), free(o_fl), free(o_st), free(x_g), free(x_f), free(x_c), free(counts);
    }
    free(T.gf), free(T.slot), free(T.gc), free(T.acc), free(T.com);
    free(M.park_g), free(M.park_first), free(M.park_count), free(M.tile);
  }
  return 0;
}
