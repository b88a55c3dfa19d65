// The control-plane host-pointer calls on the CPU (tests/test_host_ctl_abi.py compiles this with AddressSanitizer and
// UBSan and runs it): gpx_ctl_args.inc, gpx_host_stage.inc, the four *_host.inc and gpx_group_host.inc as they are, over stand-ins for the
// HIP runtime, the engine, the *_dev twins and the directly launched kernels.  "Device" memory is heap blocks of the
// exact size asked for, so a copy or a stub past an end is a sanitizer report; every runtime call is counted; a stub
// fills its outputs as a hash of everything it was given, so a column that did not arrive whole changes every output.
// Each line of the transcript is one call: its return code, a digest of every output byte, and the runtime calls it
// made.  tests/golden/host_ctl_transcript.txt is the transcript of the text these calls had before CtlStage, made by
// this program with -DGPX_CTL_TEXT='"<file with that text>"'; scripts/host_ctl_previous_text.sh writes that file from the history.
// What this cannot show is what only the GPU has: real kernels, real ordering on a stream (tests/test_host_ctl_gpu.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "gpx.h"
#include "gpx_wire.h"
#include "gpx_scan.h"
#include "gpx_sweep.h"

// ---- the runtime ----------------------------------------------------------------------------------------------------
typedef int hipError_t;
typedef void* hipStream_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2, hipErrorInjected = 3 };
enum hipMemcpyKind { hipMemcpyHostToDevice, hipMemcpyDeviceToHost };
static const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : e ? "error" : "ok"; }

struct Rt {
  std::map<void*, size_t> live;
  long allocs = 0, memsets = 0, copies = 0, launches = 0, syncs = 0; /* of the current call */
  long fail_alloc = 0, fail_copy = 0, fail_sync = 0;                  /* the k-th of the call fails (0: none) */
  long pending = 0;                                                   /* queued behind the last synchronisation */
  void begin() { allocs = memsets = copies = launches = syncs = 0; }
} rt;

static hipError_t hipMalloc(void** p, size_t bytes) {
  if (++rt.allocs == rt.fail_alloc) return hipErrorOutOfMemory;
  *p = malloc(bytes);
  memset(*p, 0xEE, bytes); /* garbage: what a call reads it has zeroed or written */
  rt.live[*p] = bytes;
  return hipSuccess;
}
static hipError_t hipFree(void* p) {
  if (!rt.live.erase(p)) {
    printf("hipFree of an unknown block\n");
    exit(1);
  }
  free(p);
  return hipSuccess;
}
static hipError_t hipMemsetAsync(void* p, int v, size_t bytes, hipStream_t) {
  rt.memsets++, rt.pending++;
  memset(p, v, bytes);
  return hipSuccess;
}
static hipError_t hipStreamSynchronize(hipStream_t) {
  if (++rt.syncs == rt.fail_sync) return hipErrorInjected;
  rt.pending = 0;
  return hipSuccess;
}
struct gpx_engine;
static hipError_t xfer(gpx_engine*, void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
  if (++rt.copies == rt.fail_copy) return hipErrorInjected;
  if (!dst || !src) return hipErrorInvalidValue;
  rt.pending++;
  memcpy(dst, src, bytes);
  return hipSuccess;
}

static thread_local char g_err[256] = "";
#define HIPQ(call) ((void)(call))
#define HIPCHK(expr)                                               \
  do {                                                             \
    hipError_t _e = (expr);                                        \
    if (_e != hipSuccess) {                                        \
      snprintf(g_err, sizeof(g_err), "%s -> %s", #expr, hipGetErrorString(_e)); \
      return GPX_EDEVICE;                                          \
    }                                                              \
  } while (0)
#define LAUNCH(e, name, kernel, grid, ...) \
  do {                                     \
    (void)(grid);                          \
    rt.launches++, rt.pending++;           \
    kernel(__VA_ARGS__);                   \
  } while (0)
#define GPX_BLOCK 256
static inline int grid_for(int64_t n) { return (int)((n + GPX_BLOCK - 1) / GPX_BLOCK); }

// ---- the engine -----------------------------------------------------------------------------------------------------
#define GPX_MAX_NODE_LIST 16
#define NM_WAYS 4
#define NM_BUCKET 128
struct NodeLists {
  int32_t n_down, n_long;
  int32_t down[GPX_MAX_NODE_LIST], longdead[GPX_MAX_NODE_LIST];
};
struct DevState { int32_t G, W; };
struct DevNames {
  uint8_t *rows, *tab;
  int32_t cap;
};
struct NameCopies {
  uint8_t *rows, *tab;
};
struct ScanCounts { int32_t v[4]; };
struct SweepCounts { int32_t v[4]; };
struct gpx_engine {
  hipStream_t sB = nullptr, stream = nullptr;
  char* arena = nullptr;
  size_t arena_cap = 0, arena_used = 0, arena_demand = 0, arena_want = 0;
  bool arena_busy = false;
  struct { int32_t max_batch = 4096, max_groups = 1 << 19, kmax = 3; } cfg;
  DevState S{1 << 19, 8};
  DevNames N{};
  int64_t nm_tomb = 0;
  ScanCounts* scan_counts = nullptr;
  SweepCounts* sweep_counts = nullptr;
  std::vector<int32_t> free_rows;
  bool free_init = false;
  gpx_engine() { /* what the lazy initialisers of the real engine allocate: here before the first call is counted */
    N.cap = 4096;
    hipMalloc((void**)&N.tab, (size_t)N.cap / NM_WAYS * NM_BUCKET);
    hipMalloc((void**)&scan_counts, sizeof(ScanCounts));
    hipMalloc((void**)&sweep_counts, sizeof(SweepCounts));
  }
  ~gpx_engine() {
    if (arena) hipFree(arena);
    hipFree(N.tab), hipFree(scan_counts), hipFree(sweep_counts);
  }
};
static int check_batch(gpx_engine* h, int32_t n) {
  if (!h || n < 0) return GPX_EINVAL;
  return n > h->cfg.max_batch ? GPX_ECAPACITY : GPX_OK;
}
static int wire_names_init(gpx_engine*) { return GPX_OK; }
// scan_open / sweep_open are the engine's side (the size limit, the scratch): stand-ins; the argument checks are the real ones
static int64_t scan_max_n(const gpx_engine* e) { return std::max<int64_t>(e->cfg.max_groups, e->cfg.max_batch); }
static int scan_open(gpx_engine* h, int32_t n) { return (int64_t)n > scan_max_n(h) ? GPX_ECAPACITY : GPX_OK; }
static int sweep_open(gpx_engine* h, int32_t n) { return scan_open(h, n); }

// ---- stubs: every output a hash of every input ------------------------------------------------------------------------
struct Mix {
  uint64_t h = 1469598103934665603ull;
  void raw(const void* p, size_t b) {
    for (size_t i = 0; i < b; i++) h = (h ^ ((const uint8_t*)p)[i]) * 1099511628211ull;
  }
  Mix& sc(int64_t v) { return raw(&v, 8), *this; }
  template <class T>
  Mix& in(const T* p, size_t n) { return p ? raw(p, n * sizeof(T)) : raw("null", 4), *this; }
  uint64_t at(int salt, size_t i) const {
    uint64_t x = h ^ ((uint64_t)(salt + 1) * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)i * 0xC2B2AE3D27D4EB4Full);
    x ^= x >> 29, x *= 0xBF58476D1CE4E5B9ull, x ^= x >> 32;
    return x;
  }
  template <class T>
  const Mix& out(T* p, size_t n, int salt) const { /* a null output is one the caller did not ask for */
    for (size_t i = 0; p && i < n; i++) {
      const uint64_t v = at(salt, i);
      memcpy(&p[i], &v, sizeof(T));
    }
    return *this;
  }
  const Mix& rows(gpx_hri* p, size_t n, int salt) const { return out((uint32_t*)p, n * (sizeof(gpx_hri) / 4), salt); }
};
static_assert(sizeof(gpx_hri) % 4 == 0, "rows are filled word by word");
static void stub_dev() { rt.launches++, rt.pending++; }

static void k_names_bind(DevState, DevNames, int32_t, int32_t n, const uint8_t* names, const int32_t* off,
                         const int32_t* g, uint8_t* st) {
  Mix().sc(n).in(off, n + 1).in(names, off[n]).in(g, n).out(st, n, 0);
}
static void k_names_unbind(DevNames, int32_t, int32_t n, const int32_t* g, uint8_t* st) { Mix().sc(n).in(g, n).out(st, n, 0); }
static void k_names_reinsert(DevNames, int32_t) {}
static void k_names_lookup(DevNames, int32_t n, const uint8_t* names, const int32_t* off, int32_t* out) {
  Mix().sc(n).in(off, n + 1).in(names, off[n]).out(out, n, 0);
}
static void k_names_coordinator(DevState, DevNames, int32_t n, const int32_t* g, int32_t b, int32_t* out) {
  Mix().sc(n).sc(b).in(g, n).out(out, n, 0);
}
static void k_election_scan(DevState, int32_t n, const int32_t* g, NodeLists L, int32_t force, uint8_t* run, int32_t* b,
                            int32_t* f, uint8_t* st) {
  Mix().sc(n).sc(force).in(g, n).in(&L, 1).out(run, n, 0).out(b, n, 1).out(f, n, 2).out(st, n, 3);
}
static void k_gap_scan(DevState, int32_t n, const int32_t* g, int32_t th, int32_t mode, int32_t lim, int32_t* f, int32_t* m,
                       unsigned long long* mi, uint8_t* sy, uint8_t* st) {
  Mix().sc(n).sc(th).sc(mode).sc(lim).in(g, n).out(f, n, 0).out(m, n, 1).out(mi, n, 2).out(sy, n, 3).out(st, n, 4);
}
template <int K>
static void k_poke_scan(DevState, int32_t n, const int32_t* g, uint8_t* pk, int32_t* sl, int32_t* bn, int32_t* bc,
                        int32_t* md, uint8_t* fl, uint32_t* hd, uint8_t* st) {
  Mix().sc(n).sc(K).in(g, n).out(pk, n, 0).out(sl, n, 1).out(bn, n, 2).out(bc, n, 3).out(md, n, 4).out(fl, n, 5).out(hd, n, 6)
      .out(st, n, 7);
}
static void k_group_create(DevState, int32_t n, const int32_t* g, const int32_t* mem, const uint8_t* k, const gpx_hri* rows,
                           uint8_t* st, NameCopies) {
  Mix().sc(n).in(g, n).in(mem, (size_t)n * 3).in(k, n).in(rows, n).out(st, n, 0);
}
static void k_group_retire(DevState, int32_t n, const int32_t* g, int32_t mode, gpx_hri* rows, uint8_t* st, NameCopies) {
  Mix().sc(n).sc(mode).in(g, n).out(st, n, 0).rows(rows, n, 1);
}

extern "C" {
int gpx_prepare_batch_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* bnum, const int32_t* bcoord,
                          const int32_t* first_slot, int32_t* r_bnum, int32_t* r_bcoord, int32_t* r_gc, uint8_t* r_flags,
                          uint64_t* p_mask, int32_t* p_slot, int32_t* p_bnum, int32_t* p_bcoord, uint8_t* status) {
  stub_dev();
  const size_t nw = (size_t)n * h->S.W;
  Mix().sc(n).in(gidx, n).in(bnum, n).in(bcoord, n).in(first_slot, n).out(r_bnum, n, 0).out(r_bcoord, n, 1).out(r_gc, n, 2)
      .out(r_flags, n, 3).out(p_mask, n, 4).out(p_slot, nw, 5).out(p_bnum, nw, 6).out(p_bcoord, nw, 7).out(status, n, 8);
  return GPX_OK;
}
int gpx_request_batch_dev(gpx_engine*, int32_t n, const int32_t* gidx, const int32_t* est, const int32_t* weight,
                          const uint8_t* is_stop, int32_t max_bytes, int32_t max_size, int32_t* leader, uint8_t* status,
                          int32_t* b_gidx, int32_t* b_leader, int32_t* b_count, int32_t* b_bytes, int32_t* b_size,
                          uint8_t* b_stop, int32_t* n_batches) {
  stub_dev();
  Mix m;
  m.sc(n).sc(max_bytes).sc(max_size).in(gidx, n).in(est, n).in(weight, n).in(is_stop, n);
  const size_t nb = max_size == 1 ? 0 : m.at(9, 0) % (n + 1); /* max_size 1: the call that finds no batch */
  *n_batches = (int32_t)nb;
  m.out(leader, n, 0).out(status, n, 1).out(b_gidx, nb, 2).out(b_leader, nb, 3).out(b_count, nb, 4).out(b_bytes, nb, 5)
      .out(b_size, nb, 6).out(b_stop, nb, 7);
  return GPX_OK;
}
int gpx_wire_decode_dev(gpx_engine*, int32_t n, const uint8_t* frames, const int64_t* off, uint8_t* f_status,
                        int32_t* f_gidx, int32_t* f_type, const gpx_wire_votes* V, const gpx_wire_commits* C,
                        const gpx_wire_accepts* A, const gpx_wire_requests* R, gpx_wire_counts* counts) {
  stub_dev();
  Mix m;
  m.sc(n).in(off, n + 1).in(frames, off[n]).sc(!!V).sc(!!C).sc(!!A).sc(!!R);
  m.out(f_status, n, 0).out(f_gidx, n, 1).out(f_type, n, 2);
  /* counts up to n + 2: past a capacity of n, where the record blocks hold only what fits */
  const int32_t nv = m.at(3, 0) % (n + 3), nc = m.at(3, 1) % (n + 3), na = m.at(3, 2) % (n + 3), nr = m.at(3, 3) % (n + 3);
  memset(counts, 0, sizeof(*counts));
  counts->n_votes = nv, counts->n_commits = nc, counts->n_accepts = na, counts->n_requests = nr;
  auto k = [](int32_t got, int32_t cap) { return (size_t)std::max(0, std::min(got, cap)); };
  if (V)
    m.out(V->gidx, k(nv, V->cap), 10).out(V->bnum, k(nv, V->cap), 11).out(V->bcoord, k(nv, V->cap), 12)
        .out(V->slot, k(nv, V->cap), 13).out(V->acceptor, k(nv, V->cap), 14).out(V->max_cp, k(nv, V->cap), 15)
        .out(V->frame, k(nv, V->cap), 16);
  if (C)
    m.out(C->gidx, k(nc, C->cap), 20).out(C->bnum, k(nc, C->cap), 21).out(C->bcoord, k(nc, C->cap), 22)
        .out(C->slot, k(nc, C->cap), 23).out(C->median_cp, k(nc, C->cap), 24).out(C->kind, k(nc, C->cap), 25)
        .out(C->frame, k(nc, C->cap), 26);
  if (A)
    m.out(A->gidx, k(na, A->cap), 30).out(A->bnum, k(na, A->cap), 31).out(A->bcoord, k(na, A->cap), 32)
        .out(A->slot, k(na, A->cap), 33).out(A->median_cp, k(na, A->cap), 34).out(A->flags, k(na, A->cap), 35)
        .out(A->sender, k(na, A->cap), 36).out(A->req_id, k(na, A->cap), 37).out(A->frame, k(na, A->cap), 38);
  if (R)
    m.out(R->gidx, k(nr, R->cap), 40).out(R->is_stop, k(nr, R->cap), 41).out(R->req_id, k(nr, R->cap), 42)
        .out(R->frame, k(nr, R->cap), 43);
  return GPX_OK;
}
int gpx_wire_pack_commits_dev(gpx_engine*, int32_t n, const int32_t* n_dev, const int32_t* g, const int32_t* slot,
                              const int32_t* bnum, const int32_t* bcoord, const int32_t* median, const uint8_t* kind,
                              uint8_t* out, int64_t cap_bytes, int64_t* frame_off, int32_t* frame_len, int32_t* f_gidx,
                              int32_t* n_frames, int64_t* n_bytes) {
  stub_dev();
  if (!g || !slot || !bnum || !bcoord || !median || !kind || !out || n_dev) return GPX_EINVAL;
  Mix m;
  m.sc(n).sc(cap_bytes).in(g, n).in(slot, n).in(bnum, n).in(bcoord, n).in(median, n).in(kind, n);
  const int32_t nf = cap_bytes == 13 ? -1 : (int32_t)(m.at(9, 0) % (n + 1)); /* 13 bytes: the call with a run too long */
  *n_frames = nf;
  *n_bytes = (int64_t)std::max(nf, 0) * 7; /* may exceed cap_bytes: then nothing but the counts is written */
  if (nf > 0 && *n_bytes <= cap_bytes) m.out(out, (size_t)*n_bytes, 0).out(frame_off, nf, 1).out(frame_len, nf, 2).out(f_gidx, nf, 3);
  return GPX_OK;
}
int gpx_wire_pack_accept_replies_dev(gpx_engine*, int32_t n, const int32_t* g, const int32_t* slot, const int32_t* sender,
                                     const int64_t* req_id, const int32_t* r_bnum, const int32_t* r_bcoord,
                                     const int32_t* r_maxcp, const uint8_t* status, uint8_t* unbatched, uint8_t* out,
                                     int64_t cap_bytes, int64_t* frame_off, int32_t* frame_len, int32_t* f_gidx,
                                     int32_t* f_dest, int32_t* n_frames, int64_t* n_bytes) {
  stub_dev();
  if (!g || !slot || !r_bnum || !r_bcoord || !r_maxcp || !status || !out) return GPX_EINVAL;
  Mix m;
  m.sc(n).sc(cap_bytes).in(g, n).in(slot, n).in(sender, n).in(req_id, n).in(r_bnum, n).in(r_bcoord, n).in(r_maxcp, n)
      .in(status, n);
  /* the second half of a pass of more than two records, where the group is a multiple of 3, is left for another pass */
  for (int32_t i = 0; unbatched && i < n; i++) unbatched[i] = n > 2 && 2 * i >= n && g[i] % 3 == 0 ? 2 : (uint8_t)(g[i] & 1);
  const int32_t nf = (int32_t)(m.at(9, 0) % (n + 1));
  *n_frames = nf;
  *n_bytes = (int64_t)nf * 5;
  if (*n_bytes <= cap_bytes)
    m.out(out, (size_t)*n_bytes, 0).out(frame_off, nf, 1).out(frame_len, nf, 2).out(f_gidx, nf, 3).out(f_dest, nf, 4);
  return GPX_OK;
}
int gpx_election_begin_dev(gpx_engine*, int32_t n, const int32_t* g, const int32_t* b, uint8_t* st) {
  stub_dev();
  Mix().sc(n).in(g, n).in(b, n).out(st, n, 0);
  return GPX_OK;
}
int gpx_prepare_reply_batch_dev(gpx_engine* h, int32_t n, const int32_t* g, const int32_t* acc, const int32_t* rb,
                                const int32_t* rc, const int32_t* fs, const int32_t* pv_off, int32_t m, const int32_t* ps,
                                const int32_t* pb, const int32_t* pc, const int64_t* ph, const uint8_t* pf, uint8_t* v_kind,
                                int32_t* e_count, int32_t* e_median, int32_t* e_slot, uint8_t* e_kind, int64_t* e_handle,
                                uint8_t* e_flags, uint8_t* status) {
  stub_dev();
  if (pv_off[n] != m) return GPX_EINVAL;
  const size_t nw = (size_t)n * h->S.W;
  Mix().sc(n).in(g, n).in(acc, n).in(rb, n).in(rc, n).in(fs, n).in(pv_off, n + 1).in(ps, m).in(pb, m).in(pc, m).in(ph, m)
      .in(pf, m).out(v_kind, n, 0).out(e_count, n, 1).out(e_median, n, 2).out(e_slot, nw, 3).out(e_kind, nw, 4)
      .out(e_handle, nw, 5).out(e_flags, nw, 6).out(status, n, 7);
  return GPX_OK;
}
/* a scan: hits up to n, so past a capacity below n; only what fits is written */
static size_t scan_counts_stub(const Mix& m, int32_t n, int32_t cap, void* counts) {
  const int32_t c[4] = {(int32_t)(m.at(9, 0) % (n + 1)), (int32_t)(m.at(9, 1) % 3), 0, 0};
  memcpy(counts, c, 16);
  return (size_t)std::min(c[0], cap);
}
int gpx_election_scan_hits_dev(gpx_engine*, int32_t n, const int32_t* g, const int32_t* down, int32_t n_down,
                               const int32_t* dead, int32_t n_dead, int32_t force, int32_t cap, int32_t* o_g, uint8_t* o_run,
                               int32_t* o_b, int32_t* o_f, gpx_scan_counts* counts) {
  stub_dev();
  Mix m;
  m.sc(n).sc(force).in(g, g ? n : 0).in(down, n_down).in(dead, n_dead);
  const size_t k = scan_counts_stub(m, n, cap, counts);
  m.out(o_g, k, 0).out(o_run, k, 1).out(o_b, k, 2).out(o_f, k, 3);
  return GPX_OK;
}
int gpx_poke_scan_hits_dev(gpx_engine*, int32_t n, const int32_t* g, int32_t cap, int32_t* o_g, uint8_t* o_pk, int32_t* o_sl,
                           int32_t* o_bn, int32_t* o_bc, int32_t* o_md, uint8_t* o_fl, uint32_t* o_hd,
                           gpx_scan_counts* counts) {
  stub_dev();
  Mix m;
  m.sc(n).in(g, g ? n : 0);
  const size_t k = scan_counts_stub(m, n, cap, counts);
  m.out(o_g, k, 0).out(o_pk, k, 1).out(o_sl, k, 2).out(o_bn, k, 3).out(o_bc, k, 4).out(o_md, k, 5).out(o_fl, k, 6).out(o_hd, k, 7);
  return GPX_OK;
}
int gpx_gap_scan_hits_dev(gpx_engine*, int32_t n, const int32_t* g, int32_t th, int32_t mode, int32_t lim, int32_t require,
                          int32_t cap, int32_t* o_g, int32_t* o_f, int32_t* o_m, uint64_t* o_mi, uint8_t* o_sy,
                          gpx_scan_counts* counts) {
  stub_dev();
  Mix m;
  m.sc(n).sc(th).sc(mode).sc(lim).sc(require).in(g, g ? n : 0);
  const size_t k = scan_counts_stub(m, n, cap, counts);
  m.out(o_g, k, 0).out(o_f, k, 1).out(o_m, k, 2).out(o_mi, k, 3).out(o_sy, k, 4);
  return GPX_OK;
}
int gpx_pause_sweep_dev(gpx_engine*, int32_t n, const int32_t* g, int32_t min_age, int32_t flags, int32_t cap, int32_t* o_g,
                        uint8_t* o_age, gpx_hri* o_rows, gpx_sweep_counts* counts) {
  stub_dev();
  Mix m;
  m.sc(n).sc(min_age).sc(flags).in(g, g ? n : 0);
  const size_t k = scan_counts_stub(m, n, cap, counts);
  m.out(o_g, k, 0).out(o_age, k, 1).rows(o_rows, k, 2);
  return GPX_OK;
}
}

// ---- the text under test ----------------------------------------------------------------------------------------------
#ifdef GPX_CTL_TEXT
#include GPX_CTL_TEXT
#else
#include "gpx_ctl_args.inc"
#include "gpx_host_stage.inc"
#include "gpx_wire_host.inc"
#include "gpx_elect_host.inc"
#include "gpx_scan_host.inc"
#include "gpx_sweep_host.inc"
#include "gpx_group_host.inc"
#endif

// ---- the script -------------------------------------------------------------------------------------------------------
// One call: its buffers (exact-size heap blocks: inputs from a generator, outputs pre-filled with 0xA5 so that a byte
// written past the entries a call returns shows in the digest), then its line of the transcript.
static bool g_quiet = false; /* fault injection: no transcript */
struct Call {
  std::vector<void*> blocks;
  std::vector<std::pair<void*, size_t>> outs;
  int bad; /* which argument is faulty (0: none); the arguments of a call are numbered as they are wrapped below */
  explicit Call(int bad_) : bad(bad_) {}
  ~Call() {
    for (void* p : blocks) free(p);
  }
  void* block(size_t bytes) {
    void* p = malloc(std::max<size_t>(bytes, 1));
    blocks.push_back(p);
    return p;
  }
  template <class T>
  T* in(size_t n, uint32_t seed, uint32_t mod) {
    T* p = (T*)block(n * sizeof(T));
    uint32_t x = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < n; i++) x = x * 1664525u + 1013904223u, p[i] = (T)((x >> 8) % mod);
    return p;
  }
  template <class T>
  T* offsets(size_t n, uint32_t seed, uint32_t max_len) { /* n + 1 ascending offsets from 0 */
    T* p = (T*)block((n + 1) * sizeof(T));
    uint32_t x = seed * 2654435761u + 999u;
    p[0] = 0;
    for (size_t i = 0; i < n; i++) x = x * 1664525u + 1013904223u, p[i + 1] = p[i] + (T)((x >> 8) % (max_len + 1));
    return p;
  }
  template <class T>
  T* out(size_t n) {
    T* p = (T*)block(n * sizeof(T));
    memset(p, 0xA5, n * sizeof(T));
    outs.push_back({p, n * sizeof(T)});
    return p;
  }
  /* argument number k of the call: null / negative when it is the faulty one */
  template <class T>
  T* a(int k, T* p) const { return bad == k ? nullptr : p; }
  int32_t a(int k, int32_t n) const { return bad == k ? -1 : n; }
  void line(const char* name, int variant, int64_t n, int rc) {
    if (g_quiet) return;
    Mix d;
    for (auto& o : outs) d.raw(o.first, o.second);
    printf("%s variant %d bad %d n %lld rc %d digest %016llx allocs %ld memsets %ld copies %ld launches %ld syncs %ld\n", name,
           variant, bad, (long long)n, rc, (unsigned long long)d.h, rt.allocs, rt.memsets, rt.copies, rt.launches, rt.syncs);
  }
};

/* Every entry point as one function of (engine, n, variant, faulty argument).  Variant bit 0: optional pointers absent;
 * the further bits are the call's own (a small capacity, a mode).  Returns the return code; *nbad = how many kinds of
 * faulty argument the call has. */
typedef int (*Entry)(gpx_engine* e, int32_t n, int variant, int bad, int* nbad);
#define ENTRY(name) static int name(gpx_engine* e, int32_t n, int variant, int bad, int* nbad)
#define BEGIN(count_bad) \
  Call c(bad);           \
  *nbad = (count_bad);   \
  const bool opt = !(variant & 1); \
  (void)opt;             \
  const size_t nn = (size_t)std::max(n, 0); \
  rt.begin()
/* the call itself: its arguments in a braced list, which evaluates them left to right - the order in which the output
 * blocks enter the digest */
#define CALL(name, fn, ...)                                   \
  const int rc_ = std::apply(fn, std::tuple{__VA_ARGS__});    \
  c.line(name, variant, n, rc_);                              \
  return rc_

ENTRY(e_names_bind) {
  BEGIN(6);
  int32_t* off = c.offsets<int32_t>(nn, 1, 12);
  CALL("names_bind", gpx_names_bind, c.a(1, e), c.a(2, n), c.a(3, c.in<uint8_t>(off[nn], 2, 251)), c.a(4, off),
                                   c.a(5, c.in<int32_t>(nn, 3, 5000)), c.a(6, c.out<uint8_t>(nn)));
}
ENTRY(e_names_unbind) {
  BEGIN(3);
  uint8_t* st = opt ? c.out<uint8_t>(nn) : nullptr;
  CALL("names_unbind", gpx_names_unbind, c.a(1, e), c.a(2, n), c.a(3, c.in<int32_t>(nn, 3, 5000)), st);
}
ENTRY(e_names_lookup) {
  BEGIN(5);
  int32_t* off = c.offsets<int32_t>(nn, 1, 12);
  CALL("names_lookup", gpx_names_lookup, c.a(1, e), c.a(2, n), c.a(3, c.in<uint8_t>(off[nn], 2, 251)), c.a(4, off),
                                       c.a(5, c.out<int32_t>(nn)));
}
ENTRY(e_names_coordinator) {
  BEGIN(4);
  CALL("names_coordinator", gpx_names_coordinator, c.a(1, e), c.a(2, n), c.a(3, c.in<int32_t>(nn, 3, 5000)), 7, c.a(4, c.out<int32_t>(nn)));
}
ENTRY(e_election_scan) {
  BEGIN(11);
  const int32_t* g = opt ? c.in<int32_t>(nn, 3, 5000) : nullptr;
  const int32_t nd = bad == 8 ? 17 : bad == 9 ? -1 : 3, nl = bad == 10 ? 17 : 2;
  CALL("election_scan", gpx_election_scan, c.a(1, e), c.a(2, n), g, c.a(3, c.in<int32_t>(17, 4, 9)), nd,
                                         c.a(11, c.in<int32_t>(17, 5, 9)), nl, variant >> 1, c.a(4, c.out<uint8_t>(nn)),
                                         c.a(5, c.out<int32_t>(nn)), c.a(6, c.out<int32_t>(nn)), c.a(7, c.out<uint8_t>(nn)));
}
ENTRY(e_gap_scan) {
  BEGIN(8);
  CALL("gap_scan", gpx_gap_scan, c.a(1, e), c.a(2, n), c.a(3, c.in<int32_t>(nn, 3, 5000)), 4, 1, 64, c.a(4, c.out<int32_t>(nn)),
                               c.a(5, c.out<int32_t>(nn)), c.a(6, c.out<uint64_t>(nn)), c.a(7, c.out<uint8_t>(nn)),
                               c.a(8, c.out<uint8_t>(nn)));
}
ENTRY(e_poke_scan) {
  BEGIN(10);
  const int32_t* g = opt ? c.in<int32_t>(nn, 3, 5000) : nullptr;
  e->cfg.kmax = variant & 2 ? 9 : 3; /* another instantiation; every engine of the script lives for one entry point */
  CALL("poke_scan", gpx_poke_scan, c.a(1, e), c.a(2, n), g, c.a(3, c.out<uint8_t>(nn)), c.a(4, c.out<int32_t>(nn)),
                               c.a(5, c.out<int32_t>(nn)), c.a(6, c.out<int32_t>(nn)), c.a(7, c.out<int32_t>(nn)),
                               c.a(8, c.out<uint8_t>(nn)), c.a(9, c.out<uint32_t>(nn)), c.a(10, c.out<uint8_t>(nn)));
}
ENTRY(e_prepare_batch) {
  BEGIN(15);
  const size_t nw = nn * 8;
  CALL("prepare_batch", gpx_prepare_batch, c.a(1, e), c.a(2, n), c.a(3, c.in<int32_t>(nn, 1, 5000)), c.a(4, c.in<int32_t>(nn, 2, 9)),
                        c.a(5, c.in<int32_t>(nn, 3, 9)), c.a(6, c.in<int32_t>(nn, 4, 99)), c.a(7, c.out<int32_t>(nn)),
                        c.a(8, c.out<int32_t>(nn)), c.a(9, c.out<int32_t>(nn)), c.a(10, c.out<uint8_t>(nn)),
                        c.a(11, c.out<uint64_t>(nn)), c.a(12, c.out<int32_t>(nw)), c.a(13, c.out<int32_t>(nw)),
                        c.a(14, c.out<int32_t>(nw)), c.a(15, c.out<uint8_t>(nn)));
}
ENTRY(e_request_batch) {
  BEGIN(13);
  const int32_t* w = opt ? c.in<int32_t>(nn, 3, 9) : nullptr;
  const uint8_t* st = opt ? c.in<uint8_t>(nn, 4, 2) : nullptr;
  CALL("request_batch", gpx_request_batch, c.a(1, e), c.a(2, n), c.a(3, c.in<int32_t>(nn, 1, 5000)), c.a(4, c.in<int32_t>(nn, 2, 900)), w, st, 4096,
                        variant & 2 ? 1 : 16, c.a(5, c.out<int32_t>(nn)), c.a(6, c.out<uint8_t>(nn)), c.a(7, c.out<int32_t>(nn)),
                        c.a(8, c.out<int32_t>(nn)), c.a(9, c.out<int32_t>(nn)), c.a(10, c.out<int32_t>(nn)),
                        c.a(11, c.out<int32_t>(nn)), c.a(12, c.out<uint8_t>(nn)), c.a(13, c.out<int32_t>(1)));
}
ENTRY(e_wire_decode) {
  BEGIN(5);
  int64_t* off = c.offsets<int64_t>(nn, 1, 40);
  /* variant bit 1: capacities of a third of the frames; bit 0: no frame columns, no per-frame outputs, no request block */
  const int32_t cap = variant & 2 ? n / 3 : n;
  const size_t cc = (size_t)std::max(cap, 0);
  auto i32 = [&] { return c.out<int32_t>(cc); };
  gpx_wire_votes V{cap, i32(), i32(), i32(), i32(), i32(), i32(), opt ? i32() : nullptr};
  gpx_wire_commits Cm{cap, i32(), i32(), i32(), i32(), i32(), c.out<uint8_t>(cc), opt ? i32() : nullptr};
  gpx_wire_accepts A{cap, i32(), i32(), i32(), i32(), i32(), c.out<uint8_t>(cc), i32(), c.out<int64_t>(cc), opt ? i32() : nullptr};
  gpx_wire_requests R{cap, i32(), c.out<uint8_t>(cc), c.out<int64_t>(cc), opt ? i32() : nullptr};
  CALL("wire_decode", gpx_wire_decode, c.a(1, e), c.a(2, n), c.a(3, c.in<uint8_t>((size_t)off[nn], 2, 256)), c.a(4, off),
                      opt ? c.out<uint8_t>(nn) : nullptr, opt ? c.out<int32_t>(nn) : nullptr, opt ? c.out<int32_t>(nn) : nullptr,
                      &V, &Cm, &A, opt ? &R : nullptr, c.a(5, c.out<gpx_wire_counts>(1)));
}
ENTRY(e_pack_accept_replies) {
  BEGIN(11);
  /* variant bit 1: a capacity that the frames outgrow */
  const int64_t cap = bad == 11 ? -1 : variant & 2 ? 9 : (int64_t)nn * 12 + 8;
  const size_t cb = (size_t)std::max<int64_t>(cap, 0);
  CALL("pack_accept_replies", gpx_wire_pack_accept_replies, c.a(1, e), c.a(2, n), c.a(3, c.in<int32_t>(nn, 1, 5000)), c.a(4, c.in<int32_t>(nn, 2, 99)),
                                   opt ? c.in<int32_t>(nn, 3, 9) : nullptr, opt ? c.in<int64_t>(nn, 4, 100000) : nullptr,
                                   c.a(5, c.in<int32_t>(nn, 5, 9)), c.a(6, c.in<int32_t>(nn, 6, 9)),
                                   c.a(7, c.in<int32_t>(nn, 7, 99)), c.a(8, c.in<uint8_t>(nn, 8, 4)),
                                   opt ? c.out<uint8_t>(nn) : nullptr, c.out<uint8_t>(cb), cap, c.out<int64_t>(nn),
                                   c.out<int32_t>(nn), c.out<int32_t>(nn), c.out<int32_t>(nn), c.a(9, c.out<int32_t>(1)),
                                   c.a(10, c.out<int64_t>(1)));
}
ENTRY(e_pack_commits) {
  BEGIN(15);
  /* variant bit 1: a capacity that the frames outgrow; bit 2: the call whose twin reports a run too long */
  const int64_t cap = bad == 15 ? -1 : variant & 4 ? 13 : variant & 2 ? 9 : (int64_t)nn * 7 + 3;
  const size_t cb = (size_t)std::max<int64_t>(cap, 0);
  CALL("pack_commits", gpx_wire_pack_commits, c.a(1, e), c.a(2, n), c.a(3, c.in<int32_t>(nn, 1, 5000)), c.a(4, c.in<int32_t>(nn, 2, 99)),
                            c.a(5, c.in<int32_t>(nn, 3, 9)), c.a(6, c.in<int32_t>(nn, 4, 9)), c.a(7, c.in<int32_t>(nn, 5, 99)),
                            c.a(8, c.in<uint8_t>(nn, 6, 3)), c.a(9, c.out<uint8_t>(cb)), cap, c.a(10, c.out<int64_t>(nn)),
                            c.a(11, c.out<int32_t>(nn)), c.a(12, c.out<int32_t>(nn)), c.a(13, c.out<int32_t>(1)),
                            c.a(14, c.out<int64_t>(1)));
}
ENTRY(e_election_begin) {
  BEGIN(6);
  int32_t* g = c.in<int32_t>(nn, 1, 1 << 30);
  std::sort(g, g + nn);
  for (size_t i = 1; i < nn; i++) g[i] = std::max(g[i], g[i - 1] + 1); /* one record per group */
  if (bad == 6 && nn > 1) g[nn - 1] = g[0];
  CALL("election_begin", gpx_election_begin, c.a(1, e), c.a(2, n), c.a(3, g), c.a(4, c.in<int32_t>(nn, 2, 99)), c.a(5, c.out<uint8_t>(nn)));
}
ENTRY(e_prepare_reply_batch) {
  BEGIN(20);
  /* variant bit 1: no pvalues at all, and then no pvalue columns */
  int32_t* off = c.offsets<int32_t>(nn, 1, variant & 2 ? 0 : 3);
  const size_t m = (size_t)off[nn], nw = nn * 8;
  if (bad == 19 && nn) off[0] = 1;
  if (bad == 20 && nn) off[nn] = -1;
  const bool pv = !(variant & 2);
  CALL("prepare_reply_batch", gpx_prepare_reply_batch, c.a(1, e), c.a(2, n), c.a(3, c.in<int32_t>(nn, 2, 5000)), c.a(4, c.in<int32_t>(nn, 3, 9)),
                              c.a(5, c.in<int32_t>(nn, 4, 9)), c.a(6, c.in<int32_t>(nn, 5, 9)), c.a(7, c.in<int32_t>(nn, 6, 99)),
                              c.a(8, off), pv ? c.a(9, c.in<int32_t>(m, 7, 99)) : nullptr,
                              pv ? c.a(10, c.in<int32_t>(m, 8, 9)) : nullptr, pv ? c.in<int32_t>(m, 9, 9) : nullptr,
                              pv && opt ? c.in<int64_t>(m, 10, 100000) : nullptr, pv && opt ? c.in<uint8_t>(m, 11, 4) : nullptr,
                              c.a(11, c.out<uint8_t>(nn)), c.a(12, c.out<int32_t>(nn)), c.a(13, c.out<int32_t>(nn)),
                              c.a(14, c.out<int32_t>(nw)), c.a(15, c.out<uint8_t>(nw)), c.a(16, c.out<int64_t>(nw)),
                              c.a(17, c.out<uint8_t>(nw)), c.a(18, c.out<uint8_t>(nn)));
}
/* the _hits twins and the sweep: variant bits 1-2 choose the capacity: n, n / 4, 0, n + 5 */
static int32_t cap_of(int32_t n, int variant, int bad, int k) {
  const int32_t caps[4] = {n, n / 4, 0, n + 5};
  return bad == k ? -1 : caps[(variant >> 1) & 3];
}
ENTRY(e_election_scan_hits) {
  BEGIN(10);
  const int32_t cap = cap_of(n, variant, bad, 3);
  const size_t cc = (size_t)std::max(cap, 0);
  const int32_t nd = bad == 9 ? 17 : bad == 10 ? -1 : 3;
  CALL("election_scan_hits", gpx_election_scan_hits, c.a(1, e), c.a(2, n), opt ? c.in<int32_t>(nn, 3, 5000) : nullptr, c.in<int32_t>(17, 4, 9), nd,
                             c.in<int32_t>(17, 5, 9), 2, 0, cap, c.a(4, c.out<int32_t>(cc)), c.a(5, c.out<uint8_t>(cc)),
                             c.a(6, c.out<int32_t>(cc)), c.a(7, c.out<int32_t>(cc)), c.a(8, c.out<gpx_scan_counts>(1)));
}
ENTRY(e_poke_scan_hits) {
  BEGIN(12);
  const int32_t cap = cap_of(n, variant, bad, 3);
  const size_t cc = (size_t)std::max(cap, 0);
  CALL("poke_scan_hits", gpx_poke_scan_hits, c.a(1, e), c.a(2, n), opt ? c.in<int32_t>(nn, 3, 5000) : nullptr, cap, c.a(4, c.out<int32_t>(cc)),
                         c.a(5, c.out<uint8_t>(cc)), c.a(6, c.out<int32_t>(cc)), c.a(7, c.out<int32_t>(cc)),
                         c.a(8, c.out<int32_t>(cc)), c.a(9, c.out<int32_t>(cc)), c.a(10, c.out<uint8_t>(cc)),
                         c.a(11, c.out<uint32_t>(cc)), c.a(12, c.out<gpx_scan_counts>(1)));
}
ENTRY(e_gap_scan_hits) {
  BEGIN(9);
  const int32_t cap = cap_of(n, variant, bad, 3);
  const size_t cc = (size_t)std::max(cap, 0);
  CALL("gap_scan_hits", gpx_gap_scan_hits, c.a(1, e), c.a(2, n), opt ? c.in<int32_t>(nn, 3, 5000) : nullptr, 4, 1, 64, 3, cap,
                        c.a(4, c.out<int32_t>(cc)), c.a(5, c.out<int32_t>(cc)), c.a(6, c.out<int32_t>(cc)),
                        c.a(7, c.out<uint64_t>(cc)), c.a(8, c.out<uint8_t>(cc)), c.a(9, c.out<gpx_scan_counts>(1)));
}
ENTRY(e_pause_sweep) {
  BEGIN(9);
  const int32_t cap = cap_of(n, variant, bad, 3);
  const size_t cc = (size_t)std::max(cap, 0);
  CALL("pause_sweep", gpx_pause_sweep, c.a(1, e), c.a(2, n), opt ? c.in<int32_t>(nn, 3, 5000) : nullptr, bad == 8 ? 256 : 2, bad == 9 ? 4 : 0, cap,
                      c.a(4, c.out<int32_t>(cc)), c.a(5, c.out<uint8_t>(cc)), c.a(6, c.out<gpx_hri>(cc)),
                      c.a(7, c.out<gpx_sweep_counts>(1)));
}
ENTRY(e_group_create) {
  BEGIN(6);
  CALL("group_create", gpx_group_create, c.a(1, e), c.a(2, n), c.a(3, c.in<int32_t>(nn, 1, 1 << 19)), c.a(4, c.in<int32_t>(nn * 3, 2, 9)),
                       c.a(5, c.in<uint8_t>(nn, 3, 4)), c.a(6, (gpx_hri*)c.in<uint32_t>(nn * (sizeof(gpx_hri) / 4), 4, 99)),
                       opt ? c.out<uint8_t>(nn) : nullptr);
}
ENTRY(e_group_retire) { /* variant bit 1: kill instead of pause */
  BEGIN(4);
  CALL("group_retire", gpx_group_retire, c.a(1, e), c.a(2, n), c.a(3, c.in<int32_t>(nn, 1, 1 << 19)), bad == 4 ? 2 : (variant >> 1) & 1,
                                       opt ? c.out<gpx_hri>(nn) : nullptr, opt ? c.out<uint8_t>(nn) : nullptr);
}
ENTRY(e_group_snapshot) {
  BEGIN(4);
  CALL("group_snapshot", gpx_group_snapshot, c.a(1, e), c.a(2, n), c.a(3, c.in<int32_t>(nn, 1, 1 << 19)), c.a(4, c.out<gpx_hri>(nn)),
                                           opt ? c.out<uint8_t>(nn) : nullptr);
}

struct Row {
  Entry fn;
  std::vector<int> variants; /* beyond 0 (everything there) and 1 (optional pointers absent) */
  bool lifecycle;
};
static const Row ROWS[] = {
    {e_names_bind, {}, false},          {e_names_unbind, {}, false},        {e_names_lookup, {}, false},
    {e_names_coordinator, {}, false},   {e_election_scan, {2}, false},      {e_gap_scan, {}, false},
    {e_poke_scan, {2}, false},          {e_prepare_batch, {}, false},       {e_request_batch, {2}, false},
    {e_wire_decode, {2, 3}, false},     {e_pack_accept_replies, {2}, false}, {e_pack_commits, {2, 4}, false},
    {e_election_begin, {}, false},      {e_prepare_reply_batch, {2, 3}, false},
    {e_election_scan_hits, {2, 4, 6, 3}, false}, {e_poke_scan_hits, {2, 4, 6}, false}, {e_gap_scan_hits, {2, 4, 6}, false},
    {e_pause_sweep, {2, 4, 6, 3}, false}, {e_group_create, {}, true},       {e_group_retire, {2}, true},
    {e_group_snapshot, {}, true},
};

int main(int argc, char** argv) {
  setvbuf(stdout, nullptr, _IOLBF, 0); /* a sanitizer report ends the process: the transcript up to it stays */
  const bool faults = !(argc > 1 && !strcmp(argv[1], "--transcript-only"));
  int nbad = 0;
  for (const Row& r : ROWS) {
    /* one engine per entry point: the first call finds no arena (every buffer its own allocation), the second an arena
     * sized by the first, the larger third one takes part of its buffers from the arena and part per call, and the small
     * ones after it rewind a regrown arena */
    {
      gpx_engine e;
      for (int32_t n : {1001, 1001, 3001, 1, 0, 1001}) r.fn(&e, n, 0, 0, &nbad);
      for (int32_t n : {1001, 1, 0}) r.fn(&e, n, 1, 0, &nbad);
      for (int v : r.variants)
        for (int32_t n : {1001, 1}) r.fn(&e, n, v, 0, &nbad);
      if (r.lifecycle)
        for (int v : {0, 1}) r.fn(&e, (1 << 18) + 1, v, 0, &nbad); /* one chunk plus one record */
      else
        r.fn(&e, 5000, 0, 0, &nbad); /* above max_batch where the call has such a limit */
      for (int bad = 1; bad <= nbad; bad++) r.fn(&e, 1001, 0, bad, &nbad);
    }
    if (faults && (rt.live.size() || rt.pending)) { /* (the earlier text left copies queued when it refused a call) */
      printf("left behind: %zu blocks, %ld queued\n", rt.live.size(), rt.pending);
      return 1;
    }
    rt.pending = 0;
  }
  if (!faults) return 0;
  /* Fault injection, each on a fresh engine (every buffer a per-call allocation): the k-th allocation, copy and
   * synchronisation of the call fails, for every k the call has.  The call says so, frees what it took and leaves
   * nothing queued. */
  g_quiet = true;
  long injected = 0;
  for (const Row& r : ROWS)
    for (int32_t n : {1001, r.lifecycle ? (1 << 18) + 1 : 3})
      for (int kind = 0; kind < 3; kind++) {
        long total;
        {
          gpx_engine e;
          r.fn(&e, n, 0, 0, &nbad);
          total = kind == 0 ? rt.allocs : kind == 1 ? rt.copies : rt.syncs;
        }
        for (long k = 1; k <= total; k++) {
          gpx_engine e;
          const size_t live = rt.live.size();
          (kind == 0 ? rt.fail_alloc : kind == 1 ? rt.fail_copy : rt.fail_sync) = k;
          const int rc = r.fn(&e, n, 0, 0, &nbad);
          rt.fail_alloc = rt.fail_copy = rt.fail_sync = 0;
          if (rc >= 0 || rt.live.size() != live || rt.pending || e.arena_busy) {
            printf("entry %d n %d: %s %ld of %ld failed: rc %d, %zu blocks (were %zu), %ld queued\n", (int)(&r - ROWS), n,
                    kind == 0 ? "allocation" : kind == 1 ? "copy" : "synchronisation", k, total, rc, rt.live.size(), live,
                    rt.pending);
            return 1;
          }
          injected++;
        }
      }
  printf("faults: ok, %ld injected\n", injected);
  return 0;
}
