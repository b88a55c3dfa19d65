// Device-pointer side of include/gpx_wire.h: the lazily allocated device tables and scratch, and the launches of the
// *_dev calls (the host-pointer twins: gpx_wire_host.inc).  Needs: the engine and the kernels of gpx_engine.hip.

namespace {

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
  LAUNCH_B(e, "k_bucket_prepare", k_bucket_prepare<true>, e->S, e->X, O);
  end_call(e, fs);
  HIPCHK(hipGetLastError());
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
