/*
 * gpx_host_calls.inc — the host-pointer data-path calls of include/gpx.h (included by gpx_engine.hip: one
 * translation unit, one libgpx_hip.so).  Host code only: copy in, the _dev twin, copy out.
 *
 * Each of the four call kinds is described ONCE - its shape (how many columns of which sort), its twin (run_twin)
 * and, per entry point, the caller's pointers (HostCall) - and each transport is written ONCE over that description:
 *   staged_call   synchronous, at most GPX_STAGE_N records: one staged block each way (Stage)
 *   column_call   synchronous, above that: a copy per column, compaction only for a batch that needs it
 *   async_call    gpx_*_async + gpx_engine_wait: a set of device columns per call in flight, three streams
 * A new form of a call (other inputs, other outputs) is a HostCall plus a CallForm, not another copy of a driver.
 */

namespace {

/* ---- one description per call kind ------------------------------------------------------------------------ */

/* The device columns of one call.  Every kind lays its columns out in the order of its twin's parameters: the int32
 * inputs from i32[0], then the dense per-record int32 outputs, then the compacted ones; u8[0] is the byte input or -
 * no kind has both - the compacted byte column, the dense byte outputs follow from u8[1]. */
struct DevCols {
  int32_t* i32[11];
  uint8_t* u8[3];
  int32_t* cnt;    /* the call's output count */
  int64_t* handle; /* gpx_propose_batch_h's 64-bit handles, or null */
};

enum CallKind { K_PROPOSE, K_ACCEPT, K_REPLY, K_COMMIT };
struct CallShape {
  int n_in, n_dense, n_dense_u8, n_comp;
  bool in_u8, comp_u8;
  bool has_count;
};
constexpr CallShape SHAPES[4] = {
    /* K_PROPOSE: gidx [is_stop] -> slot bnum bcoord median_cp, status */
    {1, 4, 1, 0, true, false, false},
    /* K_ACCEPT: gidx bnum bcoord slot median_cp [a_flags] -> r_bnum r_bcoord r_maxcp, r_flags status; x_gidx x_first x_count */
    {5, 3, 2, 3, true, false, true},
    /* K_REPLY: gidx bnum bcoord slot acceptor max_cp -> [status]; d_gidx d_slot d_bnum d_bcoord d_median_cp, d_kind */
    {6, 0, 1, 5, false, true, true},
    /* K_COMMIT: gidx bnum bcoord slot median_cp [c_kind] -> status; x_gidx x_first x_count */
    {5, 0, 1, 3, true, false, true},
};

/* The caller's pointers of one call, in the shape's order.  Optional (may be null): in_u8, handle, and the status of
 * accept replies.  A form that brings its inputs or takes its outputs another way (CallForm) leaves those null. */
struct HostCall {
  CallKind kind;
  int32_t n;
  const int32_t* in[6];
  const uint8_t* in_u8;
  const int64_t* handle;
  int32_t* dense[4];
  uint8_t* dense_u8[2];
  int32_t* comp[5];
  uint8_t* comp_u8;
  int32_t* count;
  const CallShape& shape() const { return SHAPES[kind]; }
  int dense_col(int k) const { return shape().n_in + k; }
  int comp_col(int k) const { return shape().n_in + shape().n_dense + k; }
};

/* How a form of an asynchronous call differs from the plain one.  Input stage: the caller's columns; those plus two
 * constant ballot columns made on the device; or packed votes (include/gpx_packed.h).  Output stage: the compacted
 * columns remembered for async_submit / gpx_engine_wait; or one packed buffer (include/gpx_packed_out.h). */
struct CallForm {
  const gpx_packed_votes* votes = nullptr; /* K_REPLY: the six input columns come packed */
  bool common_ballot = false;              /* K_REPLY: in[1] and in[2] are null, every vote carries this ballot */
  int32_t common_bnum = 0, common_bcoord = 0;
  void* packed_out = nullptr; /* K_PROPOSE / K_REPLY: the outputs (but the status of votes) leave as one packed buffer */
  size_t packed_out_bytes = 0;
};

/* the only place that knows which column is which parameter of a twin */
int run_twin(gpx_engine* h, const HostCall& c, const DevCols& d) {
  int32_t* const* i = d.i32;
  const uint8_t* in_u8 = c.in_u8 ? d.u8[0] : nullptr;
  switch (c.kind) {
    case K_PROPOSE:
      return propose_dev_impl(h, c.n, i[0], in_u8, d.handle, i[1], i[2], i[3], i[4], d.u8[1]);
    case K_ACCEPT:
      return gpx_accept_batch_dev(h, c.n, i[0], i[1], i[2], i[3], i[4], in_u8, i[5], i[6], i[7], d.u8[1], d.u8[2], i[8],
                                  i[9], i[10], d.cnt);
    case K_REPLY:
      return gpx_accept_reply_batch_dev(h, c.n, i[0], i[1], i[2], i[3], i[4], i[5], i[6], i[7], i[8], i[9], i[10], d.u8[0],
                                        d.cnt, d.u8[1]);
    case K_COMMIT:
      return gpx_commit_batch_dev(h, c.n, i[0], i[1], i[2], i[3], i[4], in_u8, d.u8[1], i[5], i[6], i[7], d.cnt);
  }
  return GPX_EINVAL;
}

/* every pointer this form of the call needs is there (asked for n > 0 only: an empty call touches none of them) */
bool complete(const HostCall& c, const CallForm& f) {
  const CallShape& s = c.shape();
  for (int k = 0; !f.votes && k < s.n_in; k++)
    if (!c.in[k] && !(f.common_ballot && (k == 1 || k == 2))) return false;
  if (f.packed_out) return true;
  for (int k = 0; k < s.n_dense; k++)
    if (!c.dense[k]) return false;
  for (int k = 0; k < s.n_dense_u8; k++)
    if (!c.dense_u8[k] && c.kind != K_REPLY) return false;
  for (int k = 0; k < s.n_comp; k++)
    if (!c.comp[k]) return false;
  return !s.comp_u8 || c.comp_u8;
}

HostCall propose_call(int32_t n, const int32_t* gidx, const uint8_t* is_stop, const int64_t* handle, int32_t* slot,
                      int32_t* bnum, int32_t* bcoord, int32_t* median_cp, uint8_t* status) {
  return HostCall{K_PROPOSE, n, {gidx}, is_stop, handle, {slot, bnum, bcoord, median_cp}, {status}, {}, nullptr, nullptr};
}
HostCall accept_call(int32_t n, const int32_t* gidx, const int32_t* bnum, const int32_t* bcoord, const int32_t* slot,
                     const int32_t* median_cp, const uint8_t* a_flags, int32_t* r_bnum, int32_t* r_bcoord,
                     int32_t* r_maxcp, uint8_t* r_flags, uint8_t* status, int32_t* x_gidx, int32_t* x_first,
                     int32_t* x_count, int32_t* n_runs) {
  return HostCall{K_ACCEPT, n, {gidx, bnum, bcoord, slot, median_cp}, a_flags, nullptr, {r_bnum, r_bcoord, r_maxcp},
                  {r_flags, status}, {x_gidx, x_first, x_count}, nullptr, n_runs};
}
HostCall reply_call(int32_t n, const int32_t* gidx, const int32_t* bnum, const int32_t* bcoord, const int32_t* slot,
                    const int32_t* acceptor, const int32_t* max_cp, int32_t* d_gidx, int32_t* d_slot, int32_t* d_bnum,
                    int32_t* d_bcoord, int32_t* d_median_cp, uint8_t* d_kind, int32_t* n_out, uint8_t* status) {
  return HostCall{K_REPLY, n, {gidx, bnum, bcoord, slot, acceptor, max_cp}, nullptr, nullptr, {}, {status},
                  {d_gidx, d_slot, d_bnum, d_bcoord, d_median_cp}, d_kind, n_out};
}
HostCall commit_call(int32_t n, const int32_t* gidx, const int32_t* bnum, const int32_t* bcoord, const int32_t* slot,
                     const int32_t* median_cp, const uint8_t* c_kind, uint8_t* status, int32_t* x_gidx, int32_t* x_first,
                     int32_t* x_count, int32_t* n_runs) {
  return HostCall{K_COMMIT, n, {gidx, bnum, bcoord, slot, median_cp}, c_kind, nullptr, {}, {status},
                  {x_gidx, x_first, x_count}, nullptr, n_runs};
}

/* What the twins do with the compacted outputs of an unusual batch, for the length of one twin call (lazy_outputs()):
 * 0 = dense columns whatever the batch - one block comes back, or a kernel reads the count on the device -, 1 = left
 * parked (negative count) for the caller to compact on demand.  GPX_LAZY_OUTPUTS itself is for the _dev calls alone. */
struct LazyScope {
  gpx_engine* e;
  LazyScope(gpx_engine* e_, int lazy) : e(e_) { e->lazy_override = lazy; }
  ~LazyScope() { e->lazy_override = -1; }
};

/* ---- synchronous, one staged block each way ------------------------------------------------------------------ */

int staged_call(gpx_engine* h, const HostCall& c) {
  const CallShape& s = c.shape();
  const size_t n = (size_t)c.n;
  Stage st(h);
  DevCols d{}, v{}; /* v: where d's output columns will be in the pinned block after finish() (read only) */
  for (int k = 0; k < s.n_in; k++) d.i32[k] = const_cast<int32_t*>(st.in(c.in[k], n));
  d.u8[0] = const_cast<uint8_t*>(st.in(c.in_u8, n));
  d.handle = const_cast<int64_t*>(st.in(c.handle, n));
  auto out32 = [&](int col, size_t count) { return st.out<int32_t>(count, const_cast<const int32_t**>(&v.i32[col])); };
  auto out8 = [&](int col) { return st.out<uint8_t>(n, const_cast<const uint8_t**>(&v.u8[col])); };
  for (int k = 0; k < s.n_dense; k++) d.i32[c.dense_col(k)] = out32(c.dense_col(k), n);
  for (int k = 0; k < s.n_dense_u8; k++) d.u8[1 + k] = out8(1 + k);
  for (int k = 0; k < s.n_comp; k++) d.i32[c.comp_col(k)] = out32(c.comp_col(k), n);
  if (s.comp_u8) d.u8[0] = out8(0);
  if (s.has_count) d.cnt = st.out<int32_t>(4, const_cast<const int32_t**>(&v.cnt));
  int rc = st.upload();
  if (rc != GPX_OK) return rc;
  {
    LazyScope dense(h, 0);
    rc = run_twin(h, c, d);
  }
  if (s.has_count) h->last.kind = 0;
  if (rc != GPX_OK) return rc;
  if ((rc = st.finish()) != GPX_OK) return rc;
  size_t m = 0;
  if (s.has_count) m = (size_t)(*c.count = v.cnt[0]);
  for (int k = 0; k < s.n_dense; k++) memcpy(c.dense[k], v.i32[c.dense_col(k)], n * 4);
  for (int k = 0; k < s.n_dense_u8; k++)
    if (c.dense_u8[k]) memcpy(c.dense_u8[k], v.u8[1 + k], n);
  for (int k = 0; k < s.n_comp; k++) memcpy(c.comp[k], v.i32[c.comp_col(k)], m * 4);
  if (s.comp_u8) memcpy(c.comp_u8, v.u8[0], m);
  return GPX_OK;
}

/* ---- synchronous, a copy per column ---------------------------------------------------------------------------- */

int column_call(gpx_engine* h, const HostCall& c) {
  const CallShape& s = c.shape();
  const size_t n = (size_t)c.n;
  DevCols d{};
  for (int k = 0; k < 11; k++) d.i32[k] = h->st_i32[k];
  for (int k = 0; k < 3; k++) d.u8[k] = h->st_u8[k];
  d.cnt = h->st_count;
  int rc = GPX_OK;
  for (int k = 0; k < s.n_in; k++) H2D(d.i32[k], c.in[k], n * 4);
  if (c.in_u8) H2D(d.u8[0], c.in_u8, n);
  if (c.handle) { /* staging column of the 64-bit handles: allocated on first use */
    if (!h->st_handle && (rc = dev_alloc(h, &h->st_handle, (size_t)h->cfg.max_batch, false)) != GPX_OK) return rc;
    d.handle = h->st_handle;
    H2D(d.handle, c.handle, n * 8);
  }
  {
    LazyScope on_demand(h, 1); /* the count comes to the host anyway: compaction only for a batch that needs it */
    rc = run_twin(h, c, d);
  }
  if (rc != GPX_OK) return rc;
  if (s.has_count) D2H(c.count, d.cnt, 4);
  for (int k = 0; k < s.n_dense; k++) D2H(c.dense[k], d.i32[c.dense_col(k)], n * 4);
  for (int k = 0; k < s.n_dense_u8; k++)
    if (c.dense_u8[k]) D2H(c.dense_u8[k], d.u8[1 + k], n);
  SYNC_CHECKED(h, h->sB);
  if (!s.has_count) return GPX_OK;
  if (h->last.kind) {
    if (*c.count < 0) {
      if ((rc = gpx_compact_last_dev(h)) != GPX_OK) return rc;
      D2H(c.count, d.cnt, 4);
      SYNC_CHECKED(h, h->sB);
    }
    h->last.kind = 0;
  }
  const size_t m = (size_t)(*c.count);
  if (m) { /* exactly m compacted entries, not the capacity */
    for (int k = 0; k < s.n_comp; k++) D2H(c.comp[k], d.i32[c.comp_col(k)], m * 4);
    if (s.comp_u8) D2H(c.comp_u8, d.u8[0], m);
    SYNC_CHECKED(h, h->sB);
  }
  return GPX_OK;
}

int host_call(gpx_engine* h, const HostCall& c) {
  int rc = check_batch(h, c.n);
  if (rc != GPX_OK) return rc;
  if (c.shape().has_count) {
    if (!c.count) return GPX_EINVAL;
    *c.count = 0;
  }
  if (c.n == 0) return GPX_OK;
  if (!complete(c, CallForm{})) return GPX_EINVAL;
  return c.n <= GPX_STAGE_N ? staged_call(h, c) : column_call(h, c);
}

/* ---- asynchronous ------------------------------------------------------------------------------------------------ */
/* (include/gpx.h: inputs on a copy-in stream, kernels on the engine's stream behind them, dense outputs and
 * the count on the set's copy-out stream; gpx_engine_wait fetches exactly `count` compacted entries) */

/* the device address of a host buffer of `bytes` bytes INSIDE a block this engine knows to be pinned - given to
 * gpx_host_register or got from gpx_host_alloc - or null (the caller then takes the copy path, which works for any host
 * memory).  The buffer must fit in its block: a kernel running over the end of a mapping faults on the GPU.
 * Memory the engine was never told about is NOT written through a mapping, whatever the runtime says about it (until
 * round 6 hipPointerGetAttributes' "host memory" was taken on its word; scripts/probe_runtime_pins.py shows that the
 * runtime does not report its own transient pinnings that way, so this was not the fault of profiles/
 * r06_abort_backtrace.txt - but one rule is easier to keep than two).  Pinned memory from elsewhere is registered like
 * any other (gpx_host_register notes that it is pinned already). */
void* mapped_host(gpx_engine* e, void* p, size_t bytes) {
  if (!p) return nullptr;
  bool known = false;
  for (auto& r : e->registered)
    if ((char*)p >= r.first && (char*)p < r.first + r.second) {
      if ((char*)p + bytes > r.first + r.second) return nullptr;
      known = true;
      break;
    }
  if (!known) return nullptr;
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return d;
}

/* an asynchronous call failed after some of its copies or kernels were queued: no ticket will be issued, so the
 * caller has nothing to wait on - wait here, so that it may reuse its buffers and the set's columns are quiet */
int async_fail(gpx_engine* e, gpx_engine::AsyncSet& a, int rc) {
  if (e->s_in) HIPQ(hipStreamSynchronize(e->s_in));
  HIPQ(hipStreamSynchronize(e->sB));
  if (a.s_out) HIPQ(hipStreamSynchronize(a.s_out));
  (void)hipGetLastError();
  return rc;
}

int async_begin(gpx_engine* e, int32_t n, gpx_engine::AsyncSet** out) {
  int rc = check_batch(e, n);
  if (rc != GPX_OK) return rc;
  gpx_engine::AsyncSet& a = e->as[e->async_seq % (uint64_t)e->async_depth];
  if (a.busy) return GPX_EBUSY;
  if (!e->s_in) {
    const char* dd = getenv("GPX_ASYNC_DIRECT");
    e->async_no_direct = dd && !strcmp(dd, "0");
    HIPCHK(hipStreamCreateWithFlags(&e->s_in, hipStreamNonBlocking));
  }
  if (!a.ready) {
    const size_t N = (size_t)e->cfg.max_batch;
    for (auto& p : a.i32)
      if ((rc = dev_alloc(e, &p, N, false)) != GPX_OK) return rc;
    for (auto& p : a.u8)
      if ((rc = dev_alloc(e, &p, N, false)) != GPX_OK) return rc;
    if ((rc = dev_alloc(e, &a.cnt, 4, true)) != GPX_OK) return rc;
    HIPCHK(hipHostMalloc((void**)&a.h_cnt, 64, hipHostMallocDefault));
    HIPCHK(hipStreamCreateWithFlags(&a.s_out, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&a.ev_in, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&a.ev_k, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&a.ev_cnt, hipEventDisableTiming));
    a.ready = true;
  }
  a.ncols = 0;
  a.n = n;
  a.host_kind = nullptr;
  a.dev_kind = nullptr;
  a.host_count = nullptr;
  a.po_host = nullptr;
  a.h_cnt[0] = 0;
  *out = &a;
  return GPX_OK;
}
/* queues the input columns the caller brought: a DMA copy per column (from pageable memory the runtime stages it) */
int async_inputs(gpx_engine* e, const HostCall& c, const DevCols& d) {
  for (int k = 0; k < c.shape().n_in; k++)
    if (c.in[k]) HIPCHK(xfer(e, d.i32[k], c.in[k], (size_t)c.n * 4, hipMemcpyHostToDevice, e->s_in));
  if (c.in_u8) HIPCHK(xfer(e, d.u8[0], c.in_u8, (size_t)c.n, hipMemcpyHostToDevice, e->s_in));
  return GPX_OK;
}
/* queues a packed call's inputs: 8 bytes per vote and 32 per exception row cross the link, then k_votes_unpack makes
 * the six input columns of them on the same stream (where the common-ballot form runs k_fill_i32) */
int packed_inputs(gpx_engine* h, gpx_engine::AsyncSet& a, const gpx_packed_votes* pv, const DevCols& d) {
  HIPCHK(xfer(h, a.pk_rec, pv->rec, (size_t)pv->n * 8, hipMemcpyHostToDevice, h->s_in));
  if (pv->n_exc > 0) HIPCHK(xfer(h, a.pk_exc, pv->exc, (size_t)pv->n_exc * 32, hipMemcpyHostToDevice, h->s_in));
  hipLaunchKernelGGL(k_votes_unpack, dim3(grid_for(votes_unpack_lanes(pv->n))), dim3(GPX_BLOCK), 0, h->s_in, packed_hdr(*pv),
                     (const uint4*)a.pk_rec, (const int32_t*)a.pk_exc, (int4*)d.i32[0], (int4*)d.i32[1], (int4*)d.i32[2],
                     (int4*)d.i32[3], (int4*)d.i32[4], (int4*)d.i32[5]);
  return GPX_OK;
}
/* inputs are on their way: the kernels (engine stream) wait for them */
int async_inputs_done(gpx_engine* e, gpx_engine::AsyncSet& a) {
  HIPCHK(hipEventRecord(a.ev_in, e->s_in));
  HIPCHK(hipStreamWaitEvent(e->sB, a.ev_in, 0));
  return GPX_OK;
}
/* kernels are queued: the copy-out stream waits for them */
int async_kernels_done(gpx_engine* e, gpx_engine::AsyncSet& a) {
  HIPCHK(hipEventRecord(a.ev_k, e->sB));
  HIPCHK(hipStreamWaitEvent(a.s_out, a.ev_k, 0));
  return GPX_OK;
}
/* dense per-record outputs (n entries each) the caller asked for: one k_copy_out into registered memory, else a copy per column */
int async_dense_out(gpx_engine* e, gpx_engine::AsyncSet& a, const HostCall& c, const DevCols& d) {
  const size_t n = (size_t)c.n;
  CopyOut C{};
  C.fixed_n = c.n;
  for (int k = 0; k < c.shape().n_dense; k++)
    if (c.dense[k]) C.dst[C.ncols] = c.dense[k], C.src[C.ncols++] = d.i32[c.dense_col(k)];
  for (int k = 0; k < c.shape().n_dense_u8; k++)
    if (c.dense_u8[k]) C.bdst[C.nb] = c.dense_u8[k], C.bsrc[C.nb++] = d.u8[1 + k];
  if (!C.ncols && !C.nb) return GPX_OK;
  CopyOut M = C; /* ... through the host mapping */
  bool ok = !e->async_no_direct;
  for (int k = 0; k < C.ncols && ok; k++) ok = (M.dst[k] = (int32_t*)mapped_host(e, C.dst[k], n * 4)) != nullptr;
  for (int k = 0; k < C.nb && ok; k++) ok = (M.bdst[k] = (uint8_t*)mapped_host(e, C.bdst[k], n)) != nullptr;
  /* (a kernel writing through the host mapping moves about 31 GB/s where a lone DMA copy moves 48 with the other direction
   * busy - but DMA copies for the big dense columns, tried in round 5, queue behind the copy-in stream's DMA: 2.35 ms per
   * step against 1.33, profiles/r05_bench_e2e_dense_dma.json) */
  if (ok) {
    hipLaunchKernelGGL(k_copy_out, dim3(512), dim3(256), 0, a.s_out, (const int32_t*)nullptr, M);
    return GPX_OK;
  }
  for (int k = 0; k < C.ncols; k++) HIPCHK(xfer(e, C.dst[k], C.src[k], n * 4, hipMemcpyDeviceToHost, a.s_out));
  for (int k = 0; k < C.nb; k++) HIPCHK(xfer(e, C.bdst[k], C.bsrc[k], n, hipMemcpyDeviceToHost, a.s_out));
  return GPX_OK;
}

int async_submit(gpx_engine* e, gpx_engine::AsyncSet& a, bool with_count, gpx_ticket* ticket) {
  a.direct = false;
  if (with_count && a.ncols > 0 && !e->async_no_direct) {
    /* every compacted output column in registered memory: a kernel writes exactly `count` entries there */
    CopyOut C{};
    C.ncols = a.ncols;
    bool ok = true;
    for (int k = 0; k < a.ncols && ok; k++) {
      C.src[k] = a.dev_col[k];
      C.dst[k] = (int32_t*)mapped_host(e, a.host_col[k], (size_t)a.n * 4);
      ok = C.dst[k] != nullptr;
    }
    if (ok && a.host_kind) {
      C.nb = 1;
      C.bsrc[0] = a.dev_kind;
      C.bdst[0] = (uint8_t*)mapped_host(e, a.host_kind, (size_t)a.n);
      ok = C.bdst[0] != nullptr;
    }
    C.count_dst = ok ? (int32_t*)mapped_host(e, a.host_count, 4) : nullptr;
    if (ok && C.count_dst) {
      hipLaunchKernelGGL(k_copy_out, dim3(512), dim3(256), 0, a.s_out, (const int32_t*)a.cnt, C);
      a.direct = true;
    }
  }
  if (with_count && !a.direct) HIPCHK(hipMemcpyAsync(a.h_cnt, a.cnt, sizeof(int32_t), hipMemcpyDeviceToHost, a.s_out));
  HIPCHK(hipEventRecord(a.ev_cnt, a.s_out));
  a.busy = true;
  a.ticket = ++e->async_seq; /* > 0; the next call takes the next set */
  *ticket = a.ticket;
  return GPX_OK;
}
#define A_OUT(dst, src, bytes) HIPCHK(xfer(h, (dst), (src), (bytes), hipMemcpyDeviceToHost, a.s_out))

/* the staged buffer of a packed-output call over n entries to the caller: through the mapping of a block the engine knows
 * to be pinned (the length is read on the device), else left to gpx_engine_wait, which needs the header first */
int po_out(gpx_engine* e, gpx_engine::AsyncSet& a, void* out, size_t out_bytes, int32_t n) {
  void* d = (e->async_no_direct || ((uintptr_t)out & 15)) ? nullptr : mapped_host(e, out, GPX_PACKED_OUT_BYTES(n));
  if (d && !((uintptr_t)d & 15)) {
    hipLaunchKernelGGL(k_po_copy_out, dim3(512), dim3(256), 0, a.s_out, (const uint4*)a.po_stage, (uint4*)d,
                       (int64_t)GPX_PACKED_OUT_BYTES(n));
    return GPX_OK;
  }
  HIPCHK(hipMemcpyAsync(a.h_cnt, a.po_stage, sizeof(gpx_packed_out_hdr), hipMemcpyDeviceToHost, a.s_out));
  a.po_host = out;
  a.po_bytes = out_bytes;
  return GPX_OK;
}

bool async_args(const gpx_engine* h, const HostCall& c, const CallForm& f, const gpx_ticket* ticket) {
  return h && ticket && (c.count || !c.shape().has_count || f.packed_out) && (c.n <= 0 || complete(c, f));
}

int async_call(gpx_engine* h, const HostCall& c, const CallForm& f, gpx_ticket* ticket) {
  if (!async_args(h, c, f, ticket)) return GPX_EINVAL;
  const CallShape& s = c.shape();
  gpx_engine::AsyncSet* ap = nullptr;
  int rc = async_begin(h, c.n, &ap);
  if (rc != GPX_OK) return rc;
  gpx_engine::AsyncSet& a = *ap;
  /* first-use allocations, before anything is queued */
  const size_t N = (size_t)h->cfg.max_batch;
  if (f.votes && !a.pk_rec && (rc = dev_alloc(h, &a.pk_rec, 2 * N, false)) != GPX_OK) return rc;
  if (f.votes && !a.pk_exc && (rc = dev_alloc(h, &a.pk_exc, 8 * (N / GPX_PACKED_EXC_DIV), false)) != GPX_OK) return rc;
  if (f.packed_out && !a.po_stage && (rc = dev_alloc(h, &a.po_stage, GPX_PACKED_OUT_BYTES(N), false)) != GPX_OK) return rc;
  if (c.count) {
    a.host_count = c.count;
    *c.count = 0;
  }
  if (c.n > 0) {
    DevCols d{};
    for (int k = 0; k < 11; k++) d.i32[k] = a.i32[k];
    for (int k = 0; k < 3; k++) d.u8[k] = a.u8[k];
    d.cnt = a.cnt;
    /* input stage, on the copy-in stream */
    rc = f.votes ? packed_inputs(h, a, f.votes, d) : async_inputs(h, c, d);
    if (rc == GPX_OK && f.common_ballot) { /* one ballot for the whole batch: the two columns are made on the device */
      hipLaunchKernelGGL(k_fill_i32, dim3(grid_for(c.n)), dim3(GPX_BLOCK), 0, h->s_in, c.n, f.common_bnum, d.i32[1]);
      hipLaunchKernelGGL(k_fill_i32, dim3(grid_for(c.n)), dim3(GPX_BLOCK), 0, h->s_in, c.n, f.common_bcoord, d.i32[2]);
    }
    if (rc == GPX_OK) rc = async_inputs_done(h, a);
    if (rc == GPX_OK) {
      LazyScope dense(h, 0); /* k_copy_out and the pack kernels read the count on the device: dense columns, always */
      rc = run_twin(h, c, d);
    }
    if (rc == GPX_OK && f.packed_out)
      rc = c.kind == K_PROPOSE
               ? gpx_proposals_pack_dev(h, c.n, d.i32[1], d.i32[2], d.i32[3], d.i32[4], d.u8[1], a.po_stage)
               : gpx_decisions_pack_dev(h, d.cnt, c.n, d.i32[6], d.i32[7], d.i32[8], d.i32[9], d.i32[10], d.u8[0], a.po_stage);
    if (rc == GPX_OK) rc = async_kernels_done(h, a);
    if (rc == GPX_OK) rc = async_dense_out(h, a, c, d);
    /* output stage */
    if (rc == GPX_OK && f.packed_out) {
      rc = po_out(h, a, f.packed_out, f.packed_out_bytes, c.n);
    } else if (rc == GPX_OK && c.count) { /* the compacted columns: async_submit's direct copy, or gpx_engine_wait */
      a.ncols = s.n_comp;
      for (int k = 0; k < s.n_comp; k++) a.host_col[k] = c.comp[k], a.dev_col[k] = d.i32[c.comp_col(k)];
      if (s.comp_u8) a.host_kind = c.comp_u8, a.dev_kind = d.u8[0];
    }
  } else if (f.packed_out) { /* an empty call's buffer: the header alone, written at once */
    const gpx_packed_out_hdr H{GPX_PO_RECORDS, c.kind == K_PROPOSE ? GPX_PO_PROPOSALS : GPX_PO_DECISIONS, 0, 0, 0, 0, 0, 0};
    memcpy(f.packed_out, &H, sizeof(H));
  }
  if (rc == GPX_OK) rc = async_submit(h, a, c.count && c.n > 0, ticket);
  return rc == GPX_OK ? rc : async_fail(h, a, rc);
}

}  // namespace

extern "C" {

int gpx_propose_batch(gpx_engine* h, int32_t n, const int32_t* gidx, const uint8_t* is_stop,
                      int32_t* slot, int32_t* bnum, int32_t* bcoord, int32_t* median_cp,
                      uint8_t* status) {
  return host_call(h, propose_call(n, gidx, is_stop, nullptr, slot, bnum, bcoord, median_cp, status));
}

int gpx_propose_batch_h(gpx_engine* h, int32_t n, const int32_t* gidx, const uint8_t* is_stop,
                        const int64_t* handle, int32_t* slot, int32_t* bnum, int32_t* bcoord,
                        int32_t* median_cp, uint8_t* status) {
  return host_call(h, propose_call(n, gidx, is_stop, handle, slot, bnum, bcoord, median_cp, status));
}

int gpx_accept_batch(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* bnum,
                     const int32_t* bcoord, const int32_t* slot, const int32_t* median_cp,
                     const uint8_t* a_flags, int32_t* r_bnum, int32_t* r_bcoord,
                     int32_t* r_maxcp, uint8_t* r_flags, uint8_t* status, int32_t* x_gidx,
                     int32_t* x_first, int32_t* x_count, int32_t* n_runs) {
  return host_call(h, accept_call(n, gidx, bnum, bcoord, slot, median_cp, a_flags, r_bnum, r_bcoord, r_maxcp, r_flags,
                                  status, x_gidx, x_first, x_count, n_runs));
}

int gpx_accept_reply_batch(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* bnum,
                           const int32_t* bcoord, const int32_t* slot, const int32_t* acceptor,
                           const int32_t* max_cp, int32_t* d_gidx, int32_t* d_slot,
                           int32_t* d_bnum, int32_t* d_bcoord, int32_t* d_median_cp,
                           uint8_t* d_kind, int32_t* n_out, uint8_t* status) {
  return host_call(h, reply_call(n, gidx, bnum, bcoord, slot, acceptor, max_cp, d_gidx, d_slot, d_bnum, d_bcoord,
                                 d_median_cp, d_kind, n_out, status));
}

int gpx_commit_batch(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* bnum,
                     const int32_t* bcoord, const int32_t* slot, const int32_t* median_cp,
                     const uint8_t* c_kind, uint8_t* status, int32_t* x_gidx, int32_t* x_first,
                     int32_t* x_count, int32_t* n_runs) {
  return host_call(h, commit_call(n, gidx, bnum, bcoord, slot, median_cp, c_kind, status, x_gidx, x_first, x_count, n_runs));
}

int gpx_propose_batch_async(gpx_engine* h, int32_t n, const int32_t* gidx, const uint8_t* is_stop, int32_t* slot,
                            int32_t* bnum, int32_t* bcoord, int32_t* median_cp, uint8_t* status,
                            gpx_ticket* ticket) {
  return async_call(h, propose_call(n, gidx, is_stop, nullptr, slot, bnum, bcoord, median_cp, status), CallForm{}, ticket);
}

int gpx_accept_batch_async(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* bnum,
                           const int32_t* bcoord, const int32_t* slot, const int32_t* median_cp,
                           const uint8_t* a_flags, int32_t* r_bnum, int32_t* r_bcoord, int32_t* r_maxcp,
                           uint8_t* r_flags, uint8_t* status, int32_t* x_gidx, int32_t* x_first,
                           int32_t* x_count, int32_t* n_runs, gpx_ticket* ticket) {
  return async_call(h, accept_call(n, gidx, bnum, bcoord, slot, median_cp, a_flags, r_bnum, r_bcoord, r_maxcp, r_flags, status,
                                   x_gidx, x_first, x_count, n_runs), CallForm{}, ticket);
}

int gpx_accept_reply_batch_async(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* bnum,
                                 const int32_t* bcoord, int32_t common_bnum, int32_t common_bcoord,
                                 const int32_t* slot, const int32_t* acceptor, const int32_t* max_cp,
                                 int32_t* d_gidx, int32_t* d_slot, int32_t* d_bnum, int32_t* d_bcoord,
                                 int32_t* d_median_cp, uint8_t* d_kind, int32_t* n_out, uint8_t* status,
                                 gpx_ticket* ticket) {
  if ((bnum == nullptr) != (bcoord == nullptr)) return GPX_EINVAL;
  CallForm f;
  f.common_ballot = !bnum, f.common_bnum = common_bnum, f.common_bcoord = common_bcoord;
  return async_call(h, reply_call(n, gidx, bnum, bcoord, slot, acceptor, max_cp, d_gidx, d_slot, d_bnum, d_bcoord, d_median_cp,
                                  d_kind, n_out, status), f, ticket);
}

int gpx_accept_reply_packed_async(gpx_engine* h, const gpx_packed_votes* pv, int32_t* d_gidx, int32_t* d_slot,
                                  int32_t* d_bnum, int32_t* d_bcoord, int32_t* d_median_cp, uint8_t* d_kind,
                                  int32_t* n_out, uint8_t* status, gpx_ticket* ticket) {
  if (!ticket || !n_out) return GPX_EINVAL;
  int rc = packed_check(h, pv);
  if (rc != GPX_OK) return rc;
  CallForm f;
  f.votes = pv;
  return async_call(h, reply_call(pv->n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, d_gidx, d_slot, d_bnum, d_bcoord,
                                  d_median_cp, d_kind, n_out, status), f, ticket);
}

int gpx_propose_packed_out_async(gpx_engine* h, int32_t n, const int32_t* gidx, const uint8_t* is_stop, void* out,
                                 size_t out_bytes, gpx_ticket* ticket) {
  const HostCall c = propose_call(n, gidx, is_stop, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  CallForm f;
  f.packed_out = out, f.packed_out_bytes = out_bytes;
  if (!out || !async_args(h, c, f, ticket)) return GPX_EINVAL;
  int rc = check_batch(h, n);
  if (rc != GPX_OK) return rc;
  if (out_bytes < GPX_PACKED_OUT_BYTES(n)) return GPX_ECAPACITY;
  return async_call(h, c, f, ticket);
}

int gpx_accept_reply_packed_io_async(gpx_engine* h, const gpx_packed_votes* pv, void* out, size_t out_bytes,
                                     uint8_t* status, gpx_ticket* ticket) {
  if (!ticket || !out) return GPX_EINVAL;
  int rc = packed_check(h, pv);
  if (rc != GPX_OK) return rc;
  if (out_bytes < GPX_PACKED_OUT_BYTES(pv->n)) return GPX_ECAPACITY;
  const HostCall c = reply_call(pv->n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr, nullptr, status);
  CallForm f;
  f.votes = pv;
  f.packed_out = out, f.packed_out_bytes = out_bytes;
  return async_call(h, c, f, ticket);
}

int gpx_commit_batch_async(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* bnum,
                           const int32_t* bcoord, const int32_t* slot, const int32_t* median_cp,
                           const uint8_t* c_kind, uint8_t* status, int32_t* x_gidx, int32_t* x_first,
                           int32_t* x_count, int32_t* n_runs, gpx_ticket* ticket) {
  return async_call(h, commit_call(n, gidx, bnum, bcoord, slot, median_cp, c_kind, status, x_gidx, x_first, x_count, n_runs),
                    CallForm{}, ticket);
}

int gpx_engine_wait(gpx_engine* h, gpx_ticket ticket) {
  if (!h) return GPX_EINVAL;
  for (auto& a : h->as) {
    if (!a.busy || a.ticket != ticket) continue;
    HIPCHK(hipEventSynchronize(a.ev_cnt)); /* dense outputs and the count are on the host */
    if (int rc_abort = check_batch(h, 0)) { /* an exchange kernel of this call (or one before it) gave up: nothing to hand over */
      a.busy = false;
      return rc_abort;
    }
    if (a.po_host) { /* a packed buffer outside mapped memory: the header is here, it says how much there is to fetch */
      void* dst = a.po_host;
      a.po_host = nullptr;
      const int64_t used = po_size(a.h_cnt[0], a.h_cnt[1], a.h_cnt[2], a.h_cnt[3]);
      if (used < 32 || (uint64_t)used > a.po_bytes) {
        a.busy = false;
        snprintf(g_err, sizeof(g_err), "packed output header names %lld bytes for a buffer of %zu", (long long)used, a.po_bytes);
        return GPX_EDEVICE;
      }
      A_OUT(dst, a.po_stage, (size_t)used);
      SYNC_CHECKED(h, a.s_out);
    }
    if (a.host_count && !a.direct) {
      const int32_t m = a.ncols ? a.h_cnt[0] : 0;
      *a.host_count = m;
      if (m > 0) { /* exactly m compacted entries, not the capacity */
        for (int k = 0; k < a.ncols; k++) A_OUT(a.host_col[k], a.dev_col[k], (size_t)m * 4);
        if (a.host_kind) A_OUT(a.host_kind, a.dev_kind, (size_t)m);
        SYNC_CHECKED(h, a.s_out);
      }
    }
    a.busy = false;
    return GPX_OK;
  }
  return GPX_EBUSY; /* unknown, or already waited for */
}

} /* extern "C" */
#undef A_OUT
