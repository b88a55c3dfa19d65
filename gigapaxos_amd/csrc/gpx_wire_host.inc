/*
 * gpx_wire_host.inc — host side of include/gpx_wire.h (included at the end of gpx_engine.hip: one
 * translation unit, one libgpx_hip.so).  Lazily allocated device tables / scratch, launches, and
 * the host-pointer twins (H2D -> *_dev -> D2H).
 */

namespace {

/* Temporary device buffers of a host-pointer call.  They come out of one engine-owned arena that is
 * rewound at the start of every call (the host-pointer calls are synchronous, nothing of the previous
 * call is in flight) - a hipMalloc / hipFree pair per buffer cost more than the kernels of a small
 * call.  The arena grows between calls to the largest demand seen; a call that outgrows it takes
 * its extra buffers from hipMalloc for that call only. */
struct TmpDev {
  gpx_engine* e;
  hipStream_t stream;
  std::vector<void*> extra;
  bool owner;
  explicit TmpDev(gpx_engine* e_) : e(e_), stream(e_->sB), owner(!e_->arena_busy) {
    if (!owner) return; /* nested use: plain allocations */
    e->arena_busy = true;
    if (e->arena_want > e->arena_cap) {
      /* nothing is in flight on the old block: every host-pointer call ends with a stream sync */
      if (e->arena) HIPQ(hipFree(e->arena));
      e->arena = nullptr;
      e->arena_cap = 0;
      const size_t want = e->arena_want + e->arena_want / 4;
      void* q = nullptr;
      if (hipMalloc(&q, want) == hipSuccess) {
        e->arena = (char*)q;
        e->arena_cap = want;
      }
    }
    e->arena_used = 0;
    e->arena_demand = 0;
  }
  ~TmpDev() {
    for (void* q : extra) HIPQ(hipFree(q));
    if (owner) {
      e->arena_want = std::max(e->arena_want, e->arena_demand);
      e->arena_busy = false;
    }
  }
  template <typename T>
  T* get(size_t count) {
    const size_t bytes = (std::max<size_t>(count, 1) * sizeof(T) + 255) & ~(size_t)255;
    void* q = nullptr;
    if (owner) e->arena_demand += bytes;
    if (owner && e->arena && e->arena_used + bytes <= e->arena_cap) {
      q = e->arena + e->arena_used;
      e->arena_used += bytes;
    } else {
      if (hipMalloc(&q, bytes) != hipSuccess) return nullptr;
      extra.push_back(q);
    }
    /* deterministic contents where a kernel leaves a slot unwritten (records of frames refused
     * with GPX_W_CAPACITY).  On the engine's stream: the engine streams are non-blocking, a
     * null-stream memset would not be ordered before the copies / kernels that follow. */
    if (hipMemsetAsync(q, 0, bytes, stream) != hipSuccess) return nullptr;
    return (T*)q;
  }
};

int wire_names_init(gpx_engine* e) {
  if (e->N.tab) return GPX_OK;
  const size_t G = (size_t)e->cfg.max_groups;
  size_t cap = 1024; /* entries = 4 * buckets, buckets >= G: at most one name per 128-byte bucket on average */
  while (cap < 4 * G) cap <<= 1;
  DevNames& N = e->N;
  int rc;
  if ((rc = dev_alloc(e, &N.rows, G * NM_STRIDE, true)) != GPX_OK) return rc;
  uint8_t* tab = nullptr;
  if ((rc = dev_alloc(e, &tab, cap / NM_WAYS * NM_BUCKET, true)) != GPX_OK) return rc;
  N.cap = (int32_t)cap;
  N.tab = tab; /* last: names_find treats a null table as "no names" */
  return GPX_OK;
}

int wire_scratch_init(gpx_engine* e) {
  if (e->w_cnt) return GPX_OK;
  const size_t N = (size_t)e->cfg.max_batch;
  const size_t nt = (N + GPX_BLOCK - 1) / GPX_BLOCK + 1;
  int rc;
  if ((rc = dev_alloc(e, &e->w_cnt, N, false)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &e->w_tile, 4 * nt, false)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &e->w_tile_b, nt, false)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &e->w_err, 1, true)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &e->w_look, 4 * nt, true)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &e->w_ticket, 1, true)) != GPX_OK) return rc;
  if (const char* wt = getenv("GPX_WD_TILE")) {
    const int v = atoi(wt);
    if (v == 256 || v == 512) e->wire_tile = v;
  }
  return GPX_OK;
}

/* scratch of gpx_wire_pack_accepts_dev, sized from max_batch on its first call (about 100 bytes per record) */
int wire_accept_init(gpx_engine* e) {
  if (e->wa.rec) return GPX_OK;
  const size_t N = (size_t)e->cfg.max_batch, nt = (N + GPX_BLOCK - 1) / GPX_BLOCK + 1;
  AccScratch& X = e->wa;
  int rc;
  if ((rc = dev_alloc(e, &X.lead, N, false)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &X.psize, N, false)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &X.pfol, N, false)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &X.tile_b, nt, false)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &X.tile_f, nt, false)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &X.tile_k, nt, false)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &X.fd, N, false)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &X.flist, N, false)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &X.fsorted, N, false)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &X.fpos, N, false)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &X.n_members, 1, true)) != GPX_OK) return rc;
  AccRec* rec = nullptr;
  if ((rc = dev_alloc(e, &rec, N, false)) != GPX_OK) return rc;
  X.rec = rec; /* last: marks the scratch complete */
  return GPX_OK;
}

AccIn acc_in(gpx_engine* h, int32_t n_frames, const uint8_t* frames, const int64_t* frame_off, int32_t n_req,
             const int32_t* r_frame) {
  AccIn I;
  memset(&I, 0, sizeof(I));
  I.frames = frames;
  I.foff = (const long long*)frame_off;
  I.n_frames = n_frames;
  I.n_req = n_req;
  I.r_frame = r_frame;
  I.my_id = h->cfg.my_id;
  return I;
}

}  // namespace

extern "C" {

int gpx_names_bind(gpx_engine* h, int32_t n, const uint8_t* names, const int32_t* name_off,
                   const int32_t* gidx, uint8_t* status) {
  if (!h || n < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (!names || !name_off || !gidx || !status) return GPX_EINVAL;
  int rc = wire_names_init(h);
  if (rc != GPX_OK) return rc;
  const size_t nbytes = (size_t)name_off[n];
  TmpDev t(h);
  uint8_t* d_names = t.get<uint8_t>(nbytes);
  int32_t* d_off = t.get<int32_t>((size_t)n + 1);
  int32_t* d_g = t.get<int32_t>(n);
  uint8_t* d_s = t.get<uint8_t>(n);
  if (!d_names || !d_off || !d_g || !d_s) return GPX_ENOMEM;
  H2D_B(d_names, names, nbytes);
  H2D_B(d_off, name_off, ((size_t)n + 1) * 4);
  H2D_B(d_g, gidx, (size_t)n * 4);
  LAUNCH(h, "k_names_bind", k_names_bind, grid_for(n), h->S, h->N, h->S.G, n, (const uint8_t*)d_names,
         (const int32_t*)d_off, (const int32_t*)d_g, d_s);
  D2H(status, d_s, (size_t)n);
  HIPCHK(hipStreamSynchronize(h->sB));
  return GPX_OK;
}

int gpx_names_unbind(gpx_engine* h, int32_t n, const int32_t* gidx, uint8_t* status) {
  if (!h || n < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (!gidx) return GPX_EINVAL;
  int rc = wire_names_init(h);
  if (rc != GPX_OK) return rc;
  TmpDev t(h);
  int32_t* d_g = t.get<int32_t>(n);
  uint8_t* d_s = t.get<uint8_t>(n);
  if (!d_g || !d_s) return GPX_ENOMEM;
  H2D_B(d_g, gidx, (size_t)n * 4);
  LAUNCH(h, "k_names_unbind", k_names_unbind, grid_for(n), h->N, h->S.G, n, (const int32_t*)d_g, d_s);
  if (status) D2H(status, d_s, (size_t)n);
  /* tombstones fill ways that an insert never takes again and a lookup has to walk past: rebuild the table
   * once they are a sixteenth of its entries (a quarter of its buckets) */
  h->nm_tomb += n;
  if (h->nm_tomb > h->N.cap / 16) {
    HIPCHK(hipMemsetAsync(h->N.tab, 0, (size_t)h->N.cap / NM_WAYS * NM_BUCKET, h->sB));
    LAUNCH(h, "k_names_reinsert", k_names_reinsert, grid_for(h->S.G), h->N, h->S.G);
    h->nm_tomb = 0;
  }
  HIPCHK(hipStreamSynchronize(h->sB));
  return GPX_OK;
}

int gpx_names_lookup(gpx_engine* h, int32_t n, const uint8_t* names, const int32_t* name_off,
                     int32_t* gidx_out) {
  if (!h || n < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (!names || !name_off || !gidx_out) return GPX_EINVAL;
  const size_t nbytes = (size_t)name_off[n];
  TmpDev t(h);
  uint8_t* d_names = t.get<uint8_t>(nbytes);
  int32_t* d_off = t.get<int32_t>((size_t)n + 1);
  int32_t* d_o = t.get<int32_t>(n);
  if (!d_names || !d_off || !d_o) return GPX_ENOMEM;
  H2D_B(d_names, names, nbytes);
  H2D_B(d_off, name_off, ((size_t)n + 1) * 4);
  LAUNCH(h, "k_names_lookup", k_names_lookup, grid_for(n), h->N, n, (const uint8_t*)d_names,
         (const int32_t*)d_off, d_o);
  D2H(gidx_out, d_o, (size_t)n * 4);
  HIPCHK(hipStreamSynchronize(h->sB));
  return GPX_OK;
}

int gpx_names_coordinator(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t ballotnum,
                          int32_t* out) {
  if (!h || n < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (!gidx || !out) return GPX_EINVAL;
  TmpDev t(h);
  int32_t* d_g = t.get<int32_t>(n);
  int32_t* d_o = t.get<int32_t>(n);
  if (!d_g || !d_o) return GPX_ENOMEM;
  H2D_B(d_g, gidx, (size_t)n * 4);
  LAUNCH(h, "k_names_coordinator", k_names_coordinator, grid_for(n), h->S, h->N, n,
         (const int32_t*)d_g, ballotnum, d_o);
  D2H(out, d_o, (size_t)n * 4);
  HIPCHK(hipStreamSynchronize(h->sB));
  return GPX_OK;
}

int gpx_election_scan(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* down_nodes,
                      int32_t n_down, const int32_t* long_dead_nodes, int32_t n_long_dead,
                      int32_t force, uint8_t* run, int32_t* p_bnum, int32_t* p_first,
                      uint8_t* status) {
  if (!h || n < 0 || n_down < 0 || n_long_dead < 0) return GPX_EINVAL;
  if (n_down > GPX_MAX_NODE_LIST || n_long_dead > GPX_MAX_NODE_LIST) return GPX_ECAPACITY;
  if (n == 0) return GPX_OK;
  if (!run || !p_bnum || !p_first || !status || (n_down && !down_nodes) || (n_long_dead && !long_dead_nodes))
    return GPX_EINVAL;
  NodeLists L;
  memset(&L, 0, sizeof(L));
  L.n_down = n_down;
  L.n_long = n_long_dead;
  for (int32_t q = 0; q < n_down; q++) L.down[q] = down_nodes[q];
  for (int32_t q = 0; q < n_long_dead; q++) L.longdead[q] = long_dead_nodes[q];
  TmpDev t(h);
  const size_t nn = (size_t)n;
  int32_t* d_g = gidx ? t.get<int32_t>(nn) : nullptr;
  uint8_t *d_r = t.get<uint8_t>(nn), *d_s = t.get<uint8_t>(nn);
  int32_t *d_b = t.get<int32_t>(nn), *d_f = t.get<int32_t>(nn);
  if ((gidx && !d_g) || !d_r || !d_s || !d_b || !d_f) return GPX_ENOMEM;
  if (gidx) H2D_B(d_g, gidx, nn * 4);
  LAUNCH(h, "k_election_scan", k_election_scan, grid_for(n), h->S, n, (const int32_t*)d_g, L, force,
         d_r, d_b, d_f, d_s);
  D2H(run, d_r, nn);
  D2H(p_bnum, d_b, nn * 4);
  D2H(p_first, d_f, nn * 4);
  D2H(status, d_s, nn);
  HIPCHK(hipStreamSynchronize(h->sB));
  return GPX_OK;
}

int gpx_gap_scan(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t threshold,
                 int32_t sync_mode, int32_t size_limit, int32_t* first_slot,
                 int32_t* max_committed, uint64_t* missing, uint8_t* should_sync, uint8_t* status) {
  if (!h || n < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (!gidx || !first_slot || !max_committed || !missing || !should_sync || !status) return GPX_EINVAL;
  TmpDev t(h);
  const size_t nn = (size_t)n;
  int32_t *d_g = t.get<int32_t>(nn), *d_f = t.get<int32_t>(nn), *d_m = t.get<int32_t>(nn);
  unsigned long long* d_mi = t.get<unsigned long long>(nn);
  uint8_t *d_sy = t.get<uint8_t>(nn), *d_st = t.get<uint8_t>(nn);
  if (!d_g || !d_f || !d_m || !d_mi || !d_sy || !d_st) return GPX_ENOMEM;
  H2D_B(d_g, gidx, nn * 4);
  LAUNCH(h, "k_gap_scan", k_gap_scan, grid_for(n), h->S, n, (const int32_t*)d_g, threshold, sync_mode,
         size_limit, d_f, d_m, d_mi, d_sy, d_st);
  D2H(first_slot, d_f, nn * 4);
  D2H(max_committed, d_m, nn * 4);
  D2H(missing, d_mi, nn * 8);
  D2H(should_sync, d_sy, nn);
  D2H(status, d_st, nn);
  HIPCHK(hipStreamSynchronize(h->sB));
  return GPX_OK;
}

int gpx_prepare_batch_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* bnum,
                          const int32_t* bcoord, const int32_t* first_slot, int32_t* r_bnum,
                          int32_t* r_bcoord, int32_t* r_gc, uint8_t* r_flags, uint64_t* p_mask,
                          int32_t* p_slot, int32_t* p_bnum, int32_t* p_bcoord, uint8_t* status) {
  int rc = check_batch(h, n);
  if (rc != GPX_OK) return rc;
  if (n == 0) return GPX_OK;
  if (!gidx || !bnum || !bcoord || !first_slot || !r_bnum || !r_bcoord || !r_gc || !r_flags ||
      !p_mask || !p_slot || !p_bnum || !p_bcoord || !status)
    return GPX_EINVAL;
  gpx_engine* e = h;
  const int fs = begin_front(e);
  front_hist(e, n, gidx, status, 0);
  /* payload a = firstUndecidedSlot; the dense reply columns of dropped records are zeroed here */
  launch_scatter_ac(e, n, gidx, bnum, bcoord, first_slot, first_slot, nullptr, r_bnum, r_bcoord, r_gc, r_flags);
  HIPCHK(hipMemsetAsync(p_mask, 0, (size_t)n * 8, e->stream));
  begin_back(e, fs, n);
  PrepOut O{n, r_bnum, r_bcoord, r_gc, r_flags, (unsigned long long*)p_mask, p_slot, p_bnum, p_bcoord, status};
  LAUNCH_B(e, "k_bucket_prepare", k_bucket_prepare, e->S, e->X, O);
  end_call(e, fs);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

int gpx_prepare_batch(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* bnum,
                      const int32_t* bcoord, const int32_t* first_slot, int32_t* r_bnum,
                      int32_t* r_bcoord, int32_t* r_gc, uint8_t* r_flags, uint64_t* p_mask,
                      int32_t* p_slot, int32_t* p_bnum, int32_t* p_bcoord, uint8_t* status) {
  if (!h || n < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (n > h->cfg.max_batch) return GPX_ECAPACITY;
  if (!gidx || !bnum || !bcoord || !first_slot) return GPX_EINVAL;
  TmpDev t(h);
  const size_t nn = (size_t)n, W = (size_t)h->S.W;
  const int32_t* src[4] = {gidx, bnum, bcoord, first_slot};
  int32_t* in[4];
  for (int q = 0; q < 4; q++) {
    if (!(in[q] = t.get<int32_t>(nn))) return GPX_ENOMEM;
    H2D_B(in[q], src[q], nn * 4);
  }
  int32_t *o[3], *pl[3];
  for (auto& p : o) p = t.get<int32_t>(nn);
  for (auto& p : pl) p = t.get<int32_t>(nn * W);
  uint8_t *dfl = t.get<uint8_t>(nn), *dst = t.get<uint8_t>(nn);
  uint64_t* dm = t.get<uint64_t>(nn);
  if (!o[0] || !o[1] || !o[2] || !pl[0] || !pl[1] || !pl[2] || !dfl || !dst || !dm) return GPX_ENOMEM;
  int rc = gpx_prepare_batch_dev(h, n, in[0], in[1], in[2], in[3], o[0], o[1], o[2], dfl, dm, pl[0],
                                 pl[1], pl[2], dst);
  if (rc != GPX_OK) return rc;
  D2H(r_bnum, o[0], nn * 4);
  D2H(r_bcoord, o[1], nn * 4);
  D2H(r_gc, o[2], nn * 4);
  D2H(r_flags, dfl, nn);
  D2H(p_mask, dm, nn * 8);
  D2H(p_slot, pl[0], nn * W * 4);
  D2H(p_bnum, pl[1], nn * W * 4);
  D2H(p_bcoord, pl[2], nn * W * 4);
  D2H(status, dst, nn);
  HIPCHK(hipStreamSynchronize(h->sB));
  return GPX_OK;
}

int gpx_request_batch_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* est_bytes,
                          const int32_t* weight, const uint8_t* is_stop, int32_t max_bytes,
                          int32_t max_size, int32_t* leader, uint8_t* status, int32_t* b_gidx,
                          int32_t* b_leader, int32_t* b_count, int32_t* b_bytes, int32_t* b_size,
                          uint8_t* b_stop, int32_t* n_batches) {
  int rc = check_batch(h, n);
  if (rc != GPX_OK) return rc;
  if (!n_batches) return GPX_EINVAL;
  if (n == 0) {
    HIPCHK(hipMemsetAsync(n_batches, 0, sizeof(int32_t), h->sB));
    return GPX_OK;
  }
  if (!gidx || !est_bytes || !leader || !status || !b_gidx || !b_leader || !b_count || !b_bytes ||
      !b_size || !b_stop)
    return GPX_EINVAL;
  gpx_engine* e = h;
  if (!e->w_ones) { /* weight == NULL: a column of ones */
    if ((rc = dev_alloc(e, &e->w_ones, (size_t)e->cfg.max_batch, false)) != GPX_OK) return rc;
    hipLaunchKernelGGL(k_fill_i32, dim3(grid_for(e->cfg.max_batch)), dim3(GPX_BLOCK), 0, e->sB,
                       e->cfg.max_batch, 1, e->w_ones);
    HIPCHK(hipStreamSynchronize(e->sB));
  }
  const int fs = begin_front(e);
  LAUNCH(e, "k_fill_i32", k_fill_i32, grid_for(n), n, -1, leader);
  front_hist(e, n, gidx, status, -1);
  /* payload: a = est_bytes, b = weight, c = stop flag */
  launch_scatter_ac(e, n, gidx, gidx, gidx, est_bytes, weight ? weight : (const int32_t*)e->w_ones, is_stop,
                    nullptr, nullptr, nullptr, nullptr);
  begin_back(e, fs, n);
  LAUNCH_B(e, "k_bucket_reqbatch", k_bucket_reqbatch, e->S, e->X, max_bytes, max_size, leader);
  LAUNCH(e, "k_emit_dec", k_emit_dec, e->X.nbk, e->X, b_gidx, b_leader, b_count, b_bytes, b_size,
         b_stop, n_batches, (unsigned long long*)nullptr);
  end_call(e, fs);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

int gpx_request_batch(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* est_bytes,
                      const int32_t* weight, const uint8_t* is_stop, int32_t max_bytes,
                      int32_t max_size, int32_t* leader, uint8_t* status, int32_t* b_gidx,
                      int32_t* b_leader, int32_t* b_count, int32_t* b_bytes, int32_t* b_size,
                      uint8_t* b_stop, int32_t* n_batches) {
  if (!h || n < 0 || !n_batches) return GPX_EINVAL;
  *n_batches = 0;
  if (n == 0) return GPX_OK;
  if (n > h->cfg.max_batch) return GPX_ECAPACITY;
  if (!gidx || !est_bytes || !leader || !status) return GPX_EINVAL;
  TmpDev t(h);
  const size_t nn = (size_t)n;
  int32_t *dg = t.get<int32_t>(nn), *de = t.get<int32_t>(nn), *dw = weight ? t.get<int32_t>(nn) : nullptr;
  uint8_t* ds = is_stop ? t.get<uint8_t>(nn) : nullptr;
  int32_t *dl = t.get<int32_t>(nn), *o[5];
  for (auto& p : o) p = t.get<int32_t>(nn);
  uint8_t *dst = t.get<uint8_t>(nn), *dbs = t.get<uint8_t>(nn);
  int32_t* dn = t.get<int32_t>(1);
  if (!dg || !de || (weight && !dw) || (is_stop && !ds) || !dl || !o[0] || !o[1] || !o[2] || !o[3] ||
      !o[4] || !dst || !dbs || !dn)
    return GPX_ENOMEM;
  H2D_B(dg, gidx, nn * 4);
  H2D_B(de, est_bytes, nn * 4);
  if (weight) H2D_B(dw, weight, nn * 4);
  if (is_stop) H2D_B(ds, is_stop, nn);
  int rc = gpx_request_batch_dev(h, n, dg, de, dw, ds, max_bytes, max_size, dl, dst, o[0], o[1], o[2],
                                 o[3], o[4], dbs, dn);
  if (rc != GPX_OK) return rc;
  D2H(n_batches, dn, 4);
  D2H(leader, dl, nn * 4);
  D2H(status, dst, nn);
  HIPCHK(hipStreamSynchronize(h->sB));
  const size_t m = (size_t)*n_batches;
  if (m) {
    int32_t* dsts[5] = {b_gidx, b_leader, b_count, b_bytes, b_size};
    for (int q = 0; q < 5; q++) D2H(dsts[q], o[q], m * 4);
    D2H(b_stop, dbs, m);
    HIPCHK(hipStreamSynchronize(h->sB));
  }
  return GPX_OK;
}

/* host-side LIFO free list over the row space (control plane, like the Java map it serves) */
static void rows_init(gpx_engine* h) {
  if (h->free_init) return;
  for (int32_t g = h->cfg.max_groups - 1; g >= 0; g--) h->free_rows.push_back(g);
  h->free_init = true;
}
int gpx_rows_alloc(gpx_engine* h, int32_t n, int32_t* gidx_out) {
  if (!h || n < 0 || (n && !gidx_out)) return GPX_EINVAL;
  rows_init(h);
  if ((size_t)n > h->free_rows.size()) return GPX_ECAPACITY;
  for (int32_t i = 0; i < n; i++) {
    gidx_out[i] = h->free_rows.back();
    h->free_rows.pop_back();
  }
  return GPX_OK;
}
int gpx_rows_free(gpx_engine* h, int32_t n, const int32_t* gidx) {
  if (!h || n < 0 || (n && !gidx)) return GPX_EINVAL;
  rows_init(h);
  for (int32_t i = 0; i < n; i++)
    if (gidx[i] < 0 || gidx[i] >= h->cfg.max_groups) return GPX_EINVAL;
  for (int32_t i = 0; i < n; i++) h->free_rows.push_back(gidx[i]);
  return GPX_OK;
}

int gpx_wire_decode_dev(gpx_engine* h, int32_t n_frames, const uint8_t* frames,
                        const int64_t* frame_off, uint8_t* f_status, int32_t* f_gidx,
                        int32_t* f_type, const gpx_wire_votes* votes,
                        const gpx_wire_commits* commits, const gpx_wire_accepts* accepts,
                        const gpx_wire_requests* requests, gpx_wire_counts* counts) {
  if (!h || n_frames < 0 || !counts) return GPX_EINVAL;
  if (n_frames > h->cfg.max_batch) return GPX_ECAPACITY;
  HIPCHK(hipMemsetAsync(counts, 0, sizeof(gpx_wire_counts), h->sB));
  if (n_frames == 0) return GPX_OK;
  if (!frames || !frame_off || !f_status) return GPX_EINVAL;
  int rc = wire_scratch_init(h);
  if (rc != GPX_OK) return rc;
  WireOut O;
  memset(&O, 0, sizeof(O));
  if (votes) O.V = *votes;
  if (commits) O.C = *commits;
  if (accepts) O.A = *accepts;
  if (requests) O.R = *requests;
  h->stream = h->sB;
  {
    /* one launch: parse, place (look-back over the tiles), emit */
    const size_t nt = (size_t)(h->cfg.max_batch + GPX_BLOCK - 1) / GPX_BLOCK + 1;
    if (++h->w_epoch >= (1u << 24) || epoch_wraps(h, h->w_epoch)) {
      HIPCHK(hipMemsetAsync(h->w_look, 0, 4 * nt * sizeof(unsigned long long), h->stream));
      h->w_epoch = 1;
    }
    WireLook K;
    K.state = h->w_look;
    K.ticket = h->w_ticket;
    K.epoch = h->w_epoch;
#ifdef GPX_WD_TRACE
    static unsigned long long* trace_dev = nullptr;
    if (!trace_dev) HIPCHK(hipMalloc(&trace_dev, nt * 16 * sizeof(unsigned long long)));
    HIPCHK(hipMemsetAsync(trace_dev, 0, nt * 16 * sizeof(unsigned long long), h->stream));
    K.trace = trace_dev;
#endif
    {
      LaunchScope ls(h, "k_wire_decode1");
      const int wb = h->wire_tile;
      const int32_t nt1 = (n_frames + wb - 1) / wb;
      if (wb == 512)
        hipLaunchKernelGGL(k_wire_decode1<512>, dim3(nt1), dim3(512), 0, h->stream, h->S, h->N, K, O, n_frames, nt1,
                           frames, (const int64_t*)frame_off, f_status, f_gidx, f_type, counts);
      else
        hipLaunchKernelGGL(k_wire_decode1<256>, dim3(nt1), dim3(256), 0, h->stream, h->S, h->N, K, O, n_frames, nt1,
                           frames, (const int64_t*)frame_off, f_status, f_gidx, f_type, counts);
    }
#ifdef GPX_WD_TRACE
    static int trace_call = 0;
    const char* tc = getenv("GPX_WD_TRACE_CALL"); /* which decode call of the process to keep (default: every, last wins) */
    const char* tf = getenv("GPX_WD_TRACE_FILE");
    if (tf && (!tc || atoi(tc) == trace_call++)) {
      HIPCHK(hipStreamSynchronize(h->stream));
      const int32_t nt1 = (n_frames + h->wire_tile - 1) / h->wire_tile;
      std::vector<unsigned long long> tr((size_t)nt1 * 16);
      HIPCHK(hipMemcpy(tr.data(), trace_dev, tr.size() * 8, hipMemcpyDeviceToHost));
      if (FILE* fp = fopen(tf, "wb")) {
        fwrite(tr.data(), 8, tr.size(), fp);
        fclose(fp);
      }
    }
#endif
    HIPCHK(hipGetLastError());
    return GPX_OK;
  }
}

int gpx_wire_decode(gpx_engine* h, int32_t n_frames, const uint8_t* frames,
                    const int64_t* frame_off, uint8_t* f_status, int32_t* f_gidx, int32_t* f_type,
                    const gpx_wire_votes* V, const gpx_wire_commits* Cm, const gpx_wire_accepts* A,
                    const gpx_wire_requests* R, gpx_wire_counts* counts) {
  if (!h || n_frames < 0 || !counts) return GPX_EINVAL;
  memset(counts, 0, sizeof(*counts));
  if (n_frames == 0) return GPX_OK;
  if (!frames || !frame_off) return GPX_EINVAL;
  if (n_frames > h->cfg.max_batch) return GPX_ECAPACITY;
  const size_t nbytes = (size_t)frame_off[n_frames];
  const size_t nf = (size_t)n_frames;
  TmpDev t(h);
  uint8_t* d_fr = t.get<uint8_t>(nbytes);
  int64_t* d_off = t.get<int64_t>(nf + 1);
  uint8_t* d_st = t.get<uint8_t>(nf);
  int32_t* d_fg = t.get<int32_t>(nf);
  int32_t* d_ft = t.get<int32_t>(nf);
  gpx_wire_counts* d_cn = t.get<gpx_wire_counts>(1);
  if (!d_fr || !d_off || !d_st || !d_fg || !d_ft || !d_cn) return GPX_ENOMEM;
  gpx_wire_votes dV;
  gpx_wire_commits dC;
  gpx_wire_accepts dA;
  gpx_wire_requests dR;
  memset(&dV, 0, sizeof(dV));
  memset(&dC, 0, sizeof(dC));
  memset(&dA, 0, sizeof(dA));
  memset(&dR, 0, sizeof(dR));
  bool ok = true;
  auto i32 = [&](int32_t cap) { int32_t* p = t.get<int32_t>((size_t)std::max(cap, 0)); ok = ok && p; return p; };
  auto u8 = [&](int32_t cap) { uint8_t* p = t.get<uint8_t>((size_t)std::max(cap, 0)); ok = ok && p; return p; };
  auto i64 = [&](int32_t cap) { int64_t* p = t.get<int64_t>((size_t)std::max(cap, 0)); ok = ok && p; return p; };
  if (V) {
    dV.cap = V->cap;
    dV.gidx = i32(V->cap); dV.bnum = i32(V->cap); dV.bcoord = i32(V->cap); dV.slot = i32(V->cap);
    dV.acceptor = i32(V->cap); dV.max_cp = i32(V->cap);
    dV.frame = V->frame ? i32(V->cap) : nullptr;
  }
  if (Cm) {
    dC.cap = Cm->cap;
    dC.gidx = i32(Cm->cap); dC.bnum = i32(Cm->cap); dC.bcoord = i32(Cm->cap); dC.slot = i32(Cm->cap);
    dC.median_cp = i32(Cm->cap); dC.kind = u8(Cm->cap);
    dC.frame = Cm->frame ? i32(Cm->cap) : nullptr;
  }
  if (A) {
    dA.cap = A->cap;
    dA.gidx = i32(A->cap); dA.bnum = i32(A->cap); dA.bcoord = i32(A->cap); dA.slot = i32(A->cap);
    dA.median_cp = i32(A->cap); dA.flags = u8(A->cap); dA.sender = i32(A->cap); dA.req_id = i64(A->cap);
    dA.frame = A->frame ? i32(A->cap) : nullptr;
  }
  if (R) {
    dR.cap = R->cap;
    dR.gidx = i32(R->cap); dR.is_stop = u8(R->cap); dR.req_id = i64(R->cap);
    dR.frame = R->frame ? i32(R->cap) : nullptr;
  }
  if (!ok) return GPX_ENOMEM;
  H2D_B(d_fr, frames, nbytes);
  H2D_B(d_off, frame_off, (nf + 1) * 8);
  int rc = gpx_wire_decode_dev(h, n_frames, d_fr, d_off, d_st, d_fg, d_ft, V ? &dV : nullptr,
                               Cm ? &dC : nullptr, A ? &dA : nullptr, R ? &dR : nullptr, d_cn);
  if (rc != GPX_OK) return rc;
  D2H(counts, d_cn, sizeof(gpx_wire_counts));
  if (f_status) D2H(f_status, d_st, nf);
  if (f_gidx) D2H(f_gidx, d_fg, nf * 4);
  if (f_type) D2H(f_type, d_ft, nf * 4);
  HIPCHK(hipStreamSynchronize(h->sB));
  auto cut = [](int32_t n, int32_t cap) { return (size_t)std::max(0, std::min(n, cap)); };
  if (V) {
    const size_t m = cut(counts->n_votes, V->cap);
    D2H(V->gidx, dV.gidx, m * 4); D2H(V->bnum, dV.bnum, m * 4); D2H(V->bcoord, dV.bcoord, m * 4);
    D2H(V->slot, dV.slot, m * 4); D2H(V->acceptor, dV.acceptor, m * 4); D2H(V->max_cp, dV.max_cp, m * 4);
    if (V->frame) D2H(V->frame, dV.frame, m * 4);
  }
  if (Cm) {
    const size_t m = cut(counts->n_commits, Cm->cap);
    D2H(Cm->gidx, dC.gidx, m * 4); D2H(Cm->bnum, dC.bnum, m * 4); D2H(Cm->bcoord, dC.bcoord, m * 4);
    D2H(Cm->slot, dC.slot, m * 4); D2H(Cm->median_cp, dC.median_cp, m * 4); D2H(Cm->kind, dC.kind, m);
    if (Cm->frame) D2H(Cm->frame, dC.frame, m * 4);
  }
  if (A) {
    const size_t m = cut(counts->n_accepts, A->cap);
    D2H(A->gidx, dA.gidx, m * 4); D2H(A->bnum, dA.bnum, m * 4); D2H(A->bcoord, dA.bcoord, m * 4);
    D2H(A->slot, dA.slot, m * 4); D2H(A->median_cp, dA.median_cp, m * 4); D2H(A->flags, dA.flags, m);
    D2H(A->sender, dA.sender, m * 4); D2H(A->req_id, dA.req_id, m * 8);
    if (A->frame) D2H(A->frame, dA.frame, m * 4);
  }
  if (R) {
    const size_t m = cut(counts->n_requests, R->cap);
    D2H(R->gidx, dR.gidx, m * 4); D2H(R->is_stop, dR.is_stop, m); D2H(R->req_id, dR.req_id, m * 8);
    if (R->frame) D2H(R->frame, dR.frame, m * 4);
  }
  HIPCHK(hipStreamSynchronize(h->sB));
  return GPX_OK;
}

int gpx_wire_pack_commits_dev(gpx_engine* h, int32_t n, const int32_t* n_dev,
                              const int32_t* d_gidx, const int32_t* d_slot, const int32_t* d_bnum,
                              const int32_t* d_bcoord, const int32_t* d_median_cp,
                              const uint8_t* d_kind, uint8_t* out, int64_t cap_bytes,
                              int64_t* frame_off, int32_t* frame_len, int32_t* f_gidx,
                              int32_t* n_frames, int64_t* n_bytes) {
  if (!h || n < 0 || !n_frames || !n_bytes) return GPX_EINVAL;
  if (n > h->cfg.max_batch) return GPX_ECAPACITY;
  if (n == 0) {
    HIPCHK(hipMemsetAsync(n_frames, 0, sizeof(int32_t), h->sB));
    HIPCHK(hipMemsetAsync(n_bytes, 0, sizeof(int64_t), h->sB));
    return GPX_OK;
  }
  if (!d_gidx || !d_slot || !d_bnum || !d_bcoord || !d_median_cp || !d_kind || !out || !frame_off ||
      !frame_len || !f_gidx || ((uintptr_t)out & 3))
    return GPX_EINVAL;
  int rc = wire_scratch_init(h);
  if (rc != GPX_OK) return rc;
  PackIn P{n, n_dev, d_gidx, d_slot, d_bnum, d_bcoord, d_median_cp, d_kind};
  PackScratch X;
  X.err = h->w_err;
  X.size = h->w_cnt;
  X.tile_b = h->w_tile_b;
  X.tile_f = h->w_tile;
  X.ntiles = grid_for(n);
  h->stream = h->sB;
  HIPCHK(hipMemsetAsync(h->w_err, 0, sizeof(int32_t), h->sB));
  LAUNCH(h, "k_pack_scan", k_pack_scan, X.ntiles, h->S, h->N, P, X);
  LAUNCH(h, "k_pack_write", k_pack_write, X.ntiles, h->S, h->N, P, X, out, (long long)cap_bytes,
         (long long*)frame_off, frame_len, f_gidx, n_frames, (long long*)n_bytes);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

int gpx_wire_pack_accept_replies_dev(gpx_engine* h, int32_t n, const int32_t* gidx,
                                     const int32_t* slot, const int32_t* sender,
                                     const int64_t* req_id, const int32_t* r_bnum,
                                     const int32_t* r_bcoord, const int32_t* r_maxcp,
                                     const uint8_t* status, uint8_t* unbatched, uint8_t* out,
                                     int64_t cap_bytes, int64_t* frame_off, int32_t* frame_len,
                                     int32_t* f_gidx, int32_t* f_dest, int32_t* n_frames,
                                     int64_t* n_bytes) {
  int rc = check_batch(h, n);
  if (rc != GPX_OK) return rc;
  if (!n_frames || !n_bytes) return GPX_EINVAL;
  if (n == 0) {
    HIPCHK(hipMemsetAsync(n_frames, 0, sizeof(int32_t), h->sB));
    HIPCHK(hipMemsetAsync(n_bytes, 0, sizeof(int64_t), h->sB));
    return GPX_OK;
  }
  if (!gidx || !slot || !r_bnum || !r_bcoord || !r_maxcp || !status || !out || !frame_off ||
      !frame_len || !f_gidx || !f_dest || ((uintptr_t)out & 3))
    return GPX_EINVAL;
  gpx_engine* e = h;
  if (!e->w_stage) {
    if ((rc = dev_alloc(e, &e->w_stage, (size_t)e->cfg.max_batch * GPX_W_BAR_REC_BYTES, false)) != GPX_OK)
      return rc;
    if ((rc = dev_alloc(e, &e->w_bucket_bytes, (size_t)e->X.nbk, true)) != GPX_OK) return rc;
  }
  const int fs = begin_front(e);
  if (unbatched) HIPCHK(hipMemsetAsync(unbatched, 0, (size_t)n, e->stream));
  front_hist(e, n, gidx, nullptr, -1);
  launch_scatter_ac(e, n, gidx, r_bnum, r_bcoord, slot, r_maxcp, nullptr, nullptr, nullptr, nullptr, nullptr);
  begin_back(e, fs, n);
  PackArIn P{sender, (const long long*)req_id, status, unbatched, e->w_stage, e->w_bucket_bytes};
  LAUNCH_B(e, "k_bucket_pack_ar", k_bucket_pack_ar, e->S, e->X, e->N, P);
  LAUNCH(e, "k_emit_frames", k_emit_frames, e->X.nbk, e->X, P, out, (long long)cap_bytes,
         (long long*)frame_off, frame_len, f_gidx, f_dest, n_frames, (long long*)n_bytes);
  end_call(e, fs);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

int gpx_wire_pack_accept_replies(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* slot,
                                 const int32_t* sender, const int64_t* req_id,
                                 const int32_t* r_bnum, const int32_t* r_bcoord,
                                 const int32_t* r_maxcp, const uint8_t* status, uint8_t* unbatched,
                                 uint8_t* out, int64_t cap_bytes, int64_t* frame_off,
                                 int32_t* frame_len, int32_t* f_gidx, int32_t* f_dest,
                                 int32_t* n_frames, int64_t* n_bytes) {
  if (!h || n < 0 || !n_frames || !n_bytes || cap_bytes < 0) return GPX_EINVAL;
  *n_frames = 0;
  *n_bytes = 0;
  if (n == 0) return GPX_OK;
  if (n > h->cfg.max_batch) return GPX_ECAPACITY;
  TmpDev t(h);
  const size_t nn = (size_t)n;
  const int32_t* src[6] = {gidx, slot, sender, r_bnum, r_bcoord, r_maxcp};
  int32_t* c[6] = {};
  for (int q = 0; q < 6; q++) {
    if (!src[q]) continue;
    if (!(c[q] = t.get<int32_t>(nn))) return GPX_ENOMEM;
    H2D_B(c[q], src[q], nn * 4);
  }
  int64_t* drq = nullptr;
  if (req_id) {
    if (!(drq = t.get<int64_t>(nn))) return GPX_ENOMEM;
    H2D_B(drq, req_id, nn * 8);
  }
  uint8_t* dst = t.get<uint8_t>(nn);
  uint8_t* dub = t.get<uint8_t>(nn);
  uint8_t* dout = t.get<uint8_t>((size_t)cap_bytes + 4);
  int64_t* doff = t.get<int64_t>(nn);
  int32_t* dlen = t.get<int32_t>(nn);
  int32_t* dfg = t.get<int32_t>(nn);
  int32_t* dfd = t.get<int32_t>(nn);
  int32_t* dnf = t.get<int32_t>(1);
  int64_t* dnb = t.get<int64_t>(1);
  if (!dst || !dub || !dout || !doff || !dlen || !dfg || !dfd || !dnf || !dnb) return GPX_ENOMEM;
  if (!status) return GPX_EINVAL;
  H2D_B(dst, status, nn);
  int rc = gpx_wire_pack_accept_replies_dev(h, n, c[0], c[1], c[2], drq, c[3], c[4], c[5], dst, dub,
                                            dout, cap_bytes, doff, dlen, dfg, dfd, dnf, dnb);
  if (rc != GPX_OK) return rc;
  std::vector<uint8_t> ub(nn);
  D2H(n_frames, dnf, 4);
  D2H(n_bytes, dnb, 8);
  D2H(ub.data(), dub, nn);
  HIPCHK(hipStreamSynchronize(h->sB));
  if (*n_bytes > cap_bytes) return GPX_ECAPACITY;
  auto fetch = [&](int32_t f0, int64_t b0, int32_t nf, int64_t nb) -> int {
    if (!nf) return GPX_OK;
    D2H(out + b0, dout, (size_t)nb);
    D2H(frame_off + f0, doff, (size_t)nf * 8);
    D2H(frame_len + f0, dlen, (size_t)nf * 4);
    D2H(f_gidx + f0, dfg, (size_t)nf * 4);
    D2H(f_dest + f0, dfd, (size_t)nf * 4);
    HIPCHK(hipStreamSynchronize(h->sB));
    for (int32_t f = 0; f < nf; f++) frame_off[f0 + f] += b0; /* the pass wrote offsets from its own base */
    return GPX_OK;
  };
  if ((rc = fetch(0, 0, *n_frames, *n_bytes)) != GPX_OK) return rc;
  /* Replies over a per-pass limit (more than 256 replies or 4 reply ballots of one group) are packed
   * by further passes over just those records, in array order; their frames follow.  The reference's
   * maps are unbounded, so nothing is left unbatched for that reason. */
  std::vector<int32_t> idx; /* records of the current pass -> records of the call */
  for (int32_t i = 0; i < n; i++) idx.push_back(i);
  for (;;) {
    std::vector<int32_t> over;
    for (size_t q = 0; q < idx.size(); q++)
      if (ub[q] == 2) over.push_back(idx[q]);
      else if (unbatched) unbatched[idx[q]] = ub[q];
    if (over.empty()) break;
    const size_t m = over.size();
    std::vector<int32_t> col(m);
    for (int q = 0; q < 6; q++) {
      if (!src[q]) continue;
      for (size_t r = 0; r < m; r++) col[r] = src[q][over[r]];
      H2D_B(c[q], col.data(), m * 4);
      HIPCHK(hipStreamSynchronize(h->sB)); /* col is reused */
    }
    if (req_id) {
      std::vector<int64_t> rq(m);
      for (size_t r = 0; r < m; r++) rq[r] = req_id[over[r]];
      H2D_B(drq, rq.data(), m * 8);
      HIPCHK(hipStreamSynchronize(h->sB));
    }
    std::vector<uint8_t> st8(m);
    for (size_t r = 0; r < m; r++) st8[r] = status[over[r]];
    H2D_B(dst, st8.data(), m);
    HIPCHK(hipStreamSynchronize(h->sB));
    const int64_t b0 = *n_bytes;
    const int32_t f0 = *n_frames;
    rc = gpx_wire_pack_accept_replies_dev(h, (int32_t)m, c[0], c[1], c[2], drq, c[3], c[4], c[5], dst, dub, dout,
                                          cap_bytes - b0, doff, dlen, dfg, dfd, dnf, dnb);
    if (rc != GPX_OK) return rc;
    int32_t nf2 = 0;
    int64_t nb2 = 0;
    ub.assign(m, 0);
    D2H(&nf2, dnf, 4);
    D2H(&nb2, dnb, 8);
    D2H(ub.data(), dub, m);
    HIPCHK(hipStreamSynchronize(h->sB));
    if (b0 + nb2 > cap_bytes) return GPX_ECAPACITY;
    if ((rc = fetch(f0, b0, nf2, nb2)) != GPX_OK) return rc;
    *n_frames = f0 + nf2;
    *n_bytes = b0 + nb2;
    idx.swap(over);
  }
  return GPX_OK;
}

int gpx_wire_pack_commits(gpx_engine* h, int32_t n, const int32_t* d_gidx, const int32_t* d_slot,
                          const int32_t* d_bnum, const int32_t* d_bcoord,
                          const int32_t* d_median_cp, const uint8_t* d_kind, uint8_t* out,
                          int64_t cap_bytes, int64_t* frame_off, int32_t* frame_len,
                          int32_t* f_gidx, int32_t* n_frames, int64_t* n_bytes) {
  if (!h || n < 0 || !n_frames || !n_bytes || cap_bytes < 0) return GPX_EINVAL;
  *n_frames = 0;
  *n_bytes = 0;
  if (n == 0) return GPX_OK;
  if (n > h->cfg.max_batch) return GPX_ECAPACITY;
  TmpDev t(h);
  const size_t nn = (size_t)n;
  int32_t* c[5];
  for (auto& p : c) p = t.get<int32_t>(nn);
  uint8_t* dk = t.get<uint8_t>(nn);
  uint8_t* dout = t.get<uint8_t>((size_t)cap_bytes + 4);
  int64_t* doff = t.get<int64_t>(nn);
  int32_t* dlen = t.get<int32_t>(nn);
  int32_t* dfg = t.get<int32_t>(nn);
  int32_t* dnf = t.get<int32_t>(1);
  int64_t* dnb = t.get<int64_t>(1);
  if (!c[0] || !c[1] || !c[2] || !c[3] || !c[4] || !dk || !dout || !doff || !dlen || !dfg || !dnf || !dnb)
    return GPX_ENOMEM;
  const int32_t* src[5] = {d_gidx, d_slot, d_bnum, d_bcoord, d_median_cp};
  for (int q = 0; q < 5; q++) H2D_B(c[q], src[q], nn * 4);
  H2D_B(dk, d_kind, nn);
  int rc = gpx_wire_pack_commits_dev(h, n, nullptr, c[0], c[1], c[2], c[3], c[4], dk, dout, cap_bytes,
                                     doff, dlen, dfg, dnf, dnb);
  if (rc != GPX_OK) return rc;
  D2H(n_frames, dnf, 4);
  D2H(n_bytes, dnb, 8);
  HIPCHK(hipStreamSynchronize(h->sB));
  if (*n_frames < 0) {
    *n_frames = 0;
    return GPX_EINVAL; /* more than GPX_W_MAX_SEG consecutive rows of one group */
  }
  if (*n_bytes > cap_bytes) return GPX_ECAPACITY;
  const size_t m = (size_t)*n_frames;
  if (m) {
    D2H(out, dout, (size_t)*n_bytes);
    D2H(frame_off, doff, m * 8);
    D2H(frame_len, dlen, m * 4);
    D2H(f_gidx, dfg, m * 4);
    HIPCHK(hipStreamSynchronize(h->sB));
  }
  return GPX_OK;
}

int gpx_wire_request_sizes_dev(gpx_engine* h, int32_t n_frames, const uint8_t* frames, const int64_t* frame_off,
                               int32_t n, const int32_t* r_frame, int32_t* est_bytes, int32_t* weight) {
  int rc = check_batch(h, n);
  if (rc != GPX_OK) return rc;
  if (n_frames < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (!frames || !frame_off || !r_frame || !est_bytes || !weight) return GPX_EINVAL;
  h->stream = h->sB;
  const AccIn I = acc_in(h, n_frames, frames, frame_off, n, r_frame);
  LAUNCH(h, "k_acc_req_sizes", k_acc_req_sizes, grid_for(n), I, est_bytes, weight);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

int gpx_wire_pack_accepts_dev(gpx_engine* h, int32_t n_frames, const uint8_t* frames, const int64_t* frame_off_in,
                              int32_t n_req, const int32_t* r_frame, const int32_t* leader, int32_t n,
                              const int32_t* n_dev, const int32_t* b_gidx, const int32_t* b_leader,
                              const int32_t* b_count, const int32_t* slot, const int32_t* bnum, const int32_t* bcoord,
                              const int32_t* median_cp, const uint8_t* status, uint8_t* out, int64_t cap_bytes,
                              int64_t* frame_off, int32_t* frame_len, int32_t* f_gidx, int32_t* f_batch,
                              int32_t* frame_of, int32_t* n_frames_out, int64_t* n_bytes) {
  int rc = check_batch(h, n);
  if (rc != GPX_OK) return rc;
  if ((rc = check_batch(h, n_req)) != GPX_OK) return rc;
  if (n_frames < 0 || cap_bytes < 0 || !n_frames_out || !n_bytes) return GPX_EINVAL;
  if (n == 0) {
    HIPCHK(hipMemsetAsync(n_frames_out, 0, sizeof(int32_t), h->sB));
    HIPCHK(hipMemsetAsync(n_bytes, 0, sizeof(int64_t), h->sB));
    return GPX_OK;
  }
  if (!b_gidx || !slot || !bnum || !bcoord || !median_cp || !status || !out || !frame_off || !frame_len || !f_gidx ||
      !f_batch || ((uintptr_t)out & 3) || (n_req > 0 && (!frames || !frame_off_in || !r_frame)))
    return GPX_EINVAL;
  if ((rc = wire_accept_init(h)) != GPX_OK) return rc;
  AccIn I = acc_in(h, n_frames, frames, frame_off_in, n_req, r_frame);
  I.leader = leader;
  I.n = n;
  I.n_dev = n_dev;
  I.b_gidx = b_gidx;
  I.b_leader = b_leader;
  I.b_count = b_count;
  I.slot = slot;
  I.bnum = bnum;
  I.bcoord = bcoord;
  I.median = median_cp;
  I.status = status;
  AccOut O{out, (long long)cap_bytes, (long long*)frame_off, frame_len, f_gidx, f_batch, frame_of, n_frames_out,
           (long long*)n_bytes};
  const AccScratch& X = h->wa;
  h->stream = h->sB;
  if (n_req > 0) HIPCHK(hipMemsetAsync(X.lead, 0, (size_t)n_req * sizeof(AccLead), h->sB));
  const int gr = grid_for(std::max(n, n_req)), gp = grid_for(n), gq = grid_for(std::max(n_req, 1));
  LAUNCH(h, "k_acc_parse", k_acc_parse, gr, I, X);
  LAUNCH(h, "k_acc_size", k_acc_size, gp, I, X);
  LAUNCH(h, "k_acc_place", k_acc_place, gp, I, X, O);
  LAUNCH(h, "k_acc_members", k_acc_members, gq, I, X);
  LAUNCH(h, "k_acc_rank", k_acc_rank, gq, I, X, O);
  /* copy: persistent workgroups over the 16 KB tiles of what fits cap_bytes (the byte count is still on the
   * device): eight per CU of the chip's 256 */
  const long long tiles = (cap_bytes + GPX_WA_TILE - 1) / GPX_WA_TILE;
  if (tiles > 0) LAUNCH(h, "k_acc_copy", k_acc_copy, (int)std::min<long long>(tiles, 2048), I, X, O);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

} /* extern "C" */

/* PaxosPacketBatcher.dequeueImpl's payload bound + process() -> batch() (PaxosPacketBatcher.java:
 * 182-209, 268-303): which frames leave together, and which of them share a BatchedPaxosPacket */
extern "C" int gpx_wire_plan_send(int32_t n_frames, const int64_t* est, const int64_t* dest_key,
                                  int64_t max_payload, int32_t min_batch, int32_t batch_across_groups,
                                  int32_t* burst, int32_t* envelope, int32_t* position, int32_t* n_bursts) {
  if (n_frames < 0 || !n_bursts || (n_frames && (!est || !dest_key || !burst || !envelope || !position)))
    return GPX_EINVAL;
  int32_t nb = 0;
  for (int32_t f0 = 0; f0 < n_frames;) {
    /* one dequeue: take frames while the estimate so far is below the bound */
    int64_t total = 0;
    int32_t f1 = f0;
    while (f1 < n_frames && total < max_payload) total += est[f1++];
    const int32_t tasks = f1 - f0;
    if (batch_across_groups && tasks > min_batch) {
      /* first-appearance order of the recipient sets; a burst holds few distinct sets, but a dense
       * index keeps this linear anyway */
      std::vector<int64_t> keys;
      std::vector<int32_t> fill;
      std::map<int64_t, int32_t> idx;
      for (int32_t f = f0; f < f1; f++) {
        auto it = idx.find(dest_key[f]);
        int32_t e;
        if (it == idx.end()) {
          e = (int32_t)keys.size();
          idx[dest_key[f]] = e;
          keys.push_back(dest_key[f]);
          fill.push_back(0);
        } else {
          e = it->second;
        }
        envelope[f] = e;
        position[f] = fill[(size_t)e]++;
      }
    } else {
      for (int32_t f = f0; f < f1; f++) {
        envelope[f] = -1;
        position[f] = 0;
      }
    }
    for (int32_t f = f0; f < f1; f++) burst[f] = nb;
    nb++;
    f0 = f1;
  }
  *n_bursts = nb;
  return GPX_OK;
}
