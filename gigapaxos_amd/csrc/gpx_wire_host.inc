// Host-pointer side of include/gpx_wire.h and of the batch calls of include/gpx.h: names, prepare / request batches,
// frame decode and packing, each staged through CtlStage around its *_dev twin; the row free list and the send plan.
// Needs: gpx_host_stage.inc (CtlStage), wire_names_init (gpx_wire_dev.inc), LAUNCH, grid_for.

extern "C" {

int gpx_names_bind(gpx_engine* h, int32_t n, const uint8_t* names, const int32_t* name_off,
                   const int32_t* gidx, uint8_t* status) {
  if (!h || n < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (!names || !name_off || !gidx || !status) return GPX_EINVAL;
  int rc = wire_names_init(h);
  if (rc != GPX_OK) return rc;
  const size_t nn = (size_t)n;
  CtlStage t(h);
  const uint8_t* d_names = t.in(names, (size_t)name_off[n]);
  const int32_t *d_off = t.in(name_off, nn + 1), *d_g = t.in(gidx, nn);
  uint8_t* d_s = t.out(status, nn);
  if (t.ready()) return t.rc;
  LAUNCH(h, "k_names_bind", k_names_bind, grid_for(n), h->S, h->N, h->S.G, n, d_names, d_off, d_g, d_s);
  return t.fetch({d_s});
}

int gpx_names_unbind(gpx_engine* h, int32_t n, const int32_t* gidx, uint8_t* status) {
  if (!h || n < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (!gidx) return GPX_EINVAL;
  int rc = wire_names_init(h);
  if (rc != GPX_OK) return rc;
  CtlStage t(h);
  const int32_t* d_g = t.in(gidx, (size_t)n);
  uint8_t* d_s = t.out_opt(status, (size_t)n);
  if (t.ready()) return t.rc;
  LAUNCH(h, "k_names_unbind", k_names_unbind, grid_for(n), h->N, h->S.G, n, d_g, d_s);
  t.queue(d_s);
  if (t.rc != GPX_OK) return t.rc;
  /* tombstones fill ways that an insert never takes again and a lookup has to walk past: rebuild the table
   * once they are a sixteenth of its entries (a quarter of its buckets) */
  h->nm_tomb += n;
  if (h->nm_tomb > h->N.cap / 16) {
    t.zero(h->N.tab, (size_t)h->N.cap / NM_WAYS * NM_BUCKET);
    if (t.rc != GPX_OK) return t.rc;
    LAUNCH(h, "k_names_reinsert", k_names_reinsert, grid_for(h->S.G), h->N, h->S.G);
    h->nm_tomb = 0;
  }
  return t.sync();
}

int gpx_names_lookup(gpx_engine* h, int32_t n, const uint8_t* names, const int32_t* name_off,
                     int32_t* gidx_out) {
  if (!h || n < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (!names || !name_off || !gidx_out) return GPX_EINVAL;
  CtlStage t(h);
  const uint8_t* d_names = t.in(names, (size_t)name_off[n]);
  const int32_t* d_off = t.in(name_off, (size_t)n + 1);
  int32_t* d_o = t.out(gidx_out, (size_t)n);
  if (t.ready()) return t.rc;
  LAUNCH(h, "k_names_lookup", k_names_lookup, grid_for(n), h->N, n, d_names, d_off, d_o);
  return t.fetch({d_o});
}

int gpx_names_coordinator(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t ballotnum,
                          int32_t* out) {
  if (!h || n < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (!gidx || !out) return GPX_EINVAL;
  CtlStage t(h);
  const int32_t* d_g = t.in(gidx, (size_t)n);
  int32_t* d_o = t.out(out, (size_t)n);
  if (t.ready()) return t.rc;
  LAUNCH(h, "k_names_coordinator", k_names_coordinator, grid_for(n), h->S, h->N, n, d_g, ballotnum, d_o);
  return t.fetch({d_o});
}

int gpx_prepare_batch(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* bnum,
                      const int32_t* bcoord, const int32_t* first_slot, int32_t* r_bnum,
                      int32_t* r_bcoord, int32_t* r_gc, uint8_t* r_flags, uint64_t* p_mask,
                      int32_t* p_slot, int32_t* p_bnum, int32_t* p_bcoord, uint8_t* status) {
  if (!h || n < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (n > h->cfg.max_batch) return GPX_ECAPACITY;
  if (!gidx || !bnum || !bcoord || !first_slot) return GPX_EINVAL;
  const size_t nn = (size_t)n, nw = nn * (size_t)h->S.W;
  CtlStage t(h);
  const int32_t *d_g = t.in(gidx, nn), *d_b = t.in(bnum, nn), *d_c = t.in(bcoord, nn), *d_f = t.in(first_slot, nn);
  int32_t *o_b = t.out(r_bnum, nn), *o_c = t.out(r_bcoord, nn), *o_gc = t.out(r_gc, nn);
  int32_t *o_ps = t.out(p_slot, nw), *o_pb = t.out(p_bnum, nw), *o_pc = t.out(p_bcoord, nw);
  uint8_t *o_fl = t.out(r_flags, nn), *o_st = t.out(status, nn);
  uint64_t* o_m = t.out(p_mask, nn);
  if (t.ready()) return t.rc;
  if (t.ran(gpx_prepare_batch_dev(h, n, d_g, d_b, d_c, d_f, o_b, o_c, o_gc, o_fl, o_m, o_ps, o_pb, o_pc, o_st)))
    return t.rc;
  return t.fetch({o_b, o_c, o_gc, o_fl, o_m, o_ps, o_pb, o_pc, o_st});
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
  const size_t nn = (size_t)n;
  CtlStage t(h);
  const int32_t *d_g = t.in(gidx, nn), *d_e = t.in(est_bytes, nn), *d_w = t.in_opt(weight, nn);
  const uint8_t* d_s = t.in_opt(is_stop, nn);
  int32_t* o_l = t.out(leader, nn);
  int32_t *o_bg = t.out(b_gidx, nn), *o_bl = t.out(b_leader, nn), *o_bc = t.out(b_count, nn);
  int32_t *o_bb = t.out(b_bytes, nn), *o_bz = t.out(b_size, nn);
  uint8_t *o_st = t.out(status, nn), *o_bs = t.out(b_stop, nn);
  int32_t* o_n = t.out(n_batches, 1);
  if (t.ready()) return t.rc;
  if (t.ran(gpx_request_batch_dev(h, n, d_g, d_e, d_w, d_s, max_bytes, max_size, o_l, o_st, o_bg, o_bl, o_bc, o_bb,
                                  o_bz, o_bs, o_n)))
    return t.rc;
  if (t.fetch({o_n, o_l, o_st})) return t.rc;
  if (*n_batches == 0) return GPX_OK;
  return t.fetch({o_bg, o_bl, o_bc, o_bb, o_bz, o_bs}, (size_t)*n_batches);
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

int gpx_wire_decode(gpx_engine* h, int32_t n_frames, const uint8_t* frames,
                    const int64_t* frame_off, uint8_t* f_status, int32_t* f_gidx, int32_t* f_type,
                    const gpx_wire_votes* V, const gpx_wire_commits* Cm, const gpx_wire_accepts* A,
                    const gpx_wire_requests* R, gpx_wire_counts* counts) {
  if (!h || n_frames < 0 || !counts) return GPX_EINVAL;
  memset(counts, 0, sizeof(*counts));
  if (n_frames == 0) return GPX_OK;
  if (!frames || !frame_off) return GPX_EINVAL;
  if (n_frames > h->cfg.max_batch) return GPX_ECAPACITY;
  const size_t nf = (size_t)n_frames;
  CtlStage t(h);
  const uint8_t* d_fr = t.in(frames, (size_t)frame_off[n_frames]);
  const int64_t* d_off = t.in(frame_off, nf + 1);
  uint8_t* d_st = t.out_opt(f_status, nf);
  int32_t *d_fg = t.out_opt(f_gidx, nf), *d_ft = t.out_opt(f_type, nf);
  gpx_wire_counts* d_cn = t.out(counts, 1);
  /* the device's copy of each record block: the same capacity, every column the caller gave */
  gpx_wire_votes dV;
  gpx_wire_commits dC;
  gpx_wire_accepts dA;
  gpx_wire_requests dR;
  memset(&dV, 0, sizeof(dV));
  memset(&dC, 0, sizeof(dC));
  memset(&dA, 0, sizeof(dA));
  memset(&dR, 0, sizeof(dR));
  std::vector<const void*> cols[4]; /* of V, Cm, A, R */
  int blk = 0;
  int32_t cap = 0;
  auto col = [&](auto* host) {
    auto* d = t.out(host, (size_t)std::max(cap, 0));
    cols[blk].push_back(d);
    return d;
  };
  if (V) {
    blk = 0, cap = dV.cap = V->cap;
    dV.gidx = col(V->gidx), dV.bnum = col(V->bnum), dV.bcoord = col(V->bcoord), dV.slot = col(V->slot);
    dV.acceptor = col(V->acceptor), dV.max_cp = col(V->max_cp);
    if (V->frame) dV.frame = col(V->frame);
  }
  if (Cm) {
    blk = 1, cap = dC.cap = Cm->cap;
    dC.gidx = col(Cm->gidx), dC.bnum = col(Cm->bnum), dC.bcoord = col(Cm->bcoord), dC.slot = col(Cm->slot);
    dC.median_cp = col(Cm->median_cp), dC.kind = col(Cm->kind);
    if (Cm->frame) dC.frame = col(Cm->frame);
  }
  if (A) {
    blk = 2, cap = dA.cap = A->cap;
    dA.gidx = col(A->gidx), dA.bnum = col(A->bnum), dA.bcoord = col(A->bcoord), dA.slot = col(A->slot);
    dA.median_cp = col(A->median_cp), dA.flags = col(A->flags), dA.sender = col(A->sender), dA.req_id = col(A->req_id);
    if (A->frame) dA.frame = col(A->frame);
  }
  if (R) {
    blk = 3, cap = dR.cap = R->cap;
    dR.gidx = col(R->gidx), dR.is_stop = col(R->is_stop), dR.req_id = col(R->req_id);
    if (R->frame) dR.frame = col(R->frame);
  }
  if (t.ready()) return t.rc;
  if (t.ran(gpx_wire_decode_dev(h, n_frames, d_fr, d_off, d_st, d_fg, d_ft, V ? &dV : nullptr, Cm ? &dC : nullptr,
                                A ? &dA : nullptr, R ? &dR : nullptr, d_cn)))
    return t.rc;
  if (t.fetch({d_cn, d_st, d_fg, d_ft})) return t.rc;
  /* a count may exceed its capacity (records refused with GPX_W_CAPACITY): queue() stops at the column's end */
  const int32_t got[4] = {counts->n_votes, counts->n_commits, counts->n_accepts, counts->n_requests};
  for (int b = 0; b < 4; b++)
    for (const void* d : cols[b]) t.queue(d, (size_t)std::max(got[b], 0));
  return t.sync();
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
  if (!gidx || !slot || !r_bnum || !r_bcoord || !r_maxcp || !status) return GPX_EINVAL;
  const size_t nn = (size_t)n;
  /* host columns of a later pass.  For the error path only: every gather waits before the next column is built, but a
   * wait that fails leaves its copy queued, and t's destructor waits once more - so this is declared before t */
  std::vector<std::vector<uint8_t>> held;
  CtlStage t(h);
  const int32_t* src[6] = {gidx, slot, sender, r_bnum, r_bcoord, r_maxcp};
  int32_t* c[6];
  for (int q = 0; q < 6; q++) c[q] = t.in_opt(src[q], nn);
  int64_t* drq = t.in_opt(req_id, nn);
  uint8_t *dst = t.in(status, nn), *dub = t.tmp<uint8_t>(nn), *dout = t.tmp<uint8_t>((size_t)cap_bytes + 4);
  int64_t *doff = t.tmp<int64_t>(nn), *dnb = t.tmp<int64_t>(1);
  int32_t *dlen = t.tmp<int32_t>(nn), *dfg = t.tmp<int32_t>(nn), *dfd = t.tmp<int32_t>(nn), *dnf = t.tmp<int32_t>(1);
  if (t.ready()) return t.rc;
  std::vector<uint8_t> ub;
  /* one pass over the first m records of the device columns: its frames follow the f0 frames / b0 bytes already out */
  auto pass = [&](size_t m, int32_t f0, int64_t b0, int32_t* nf, int64_t* nb) -> int {
    if (t.ran(gpx_wire_pack_accept_replies_dev(h, (int32_t)m, c[0], c[1], c[2], drq, c[3], c[4], c[5], dst, dub, dout,
                                               cap_bytes - b0, doff, dlen, dfg, dfd, dnf, dnb)))
      return t.rc;
    ub.assign(m, 0);
    t.d2h(nf, dnf, 4);
    t.d2h(nb, dnb, 8);
    t.d2h(ub.data(), dub, m);
    if (t.sync()) return t.rc;
    if (b0 + *nb > cap_bytes) return GPX_ECAPACITY;
    if (!*nf) return GPX_OK;
    t.d2h(out + b0, dout, (size_t)*nb);
    t.d2h(frame_off + f0, doff, (size_t)*nf * 8);
    t.d2h(frame_len + f0, dlen, (size_t)*nf * 4);
    t.d2h(f_gidx + f0, dfg, (size_t)*nf * 4);
    t.d2h(f_dest + f0, dfd, (size_t)*nf * 4);
    if (t.sync()) return t.rc;
    for (int32_t f = 0; f < *nf; f++) frame_off[f0 + f] += b0; /* the pass wrote offsets from its own base */
    return GPX_OK;
  };
  int rc = pass(nn, 0, 0, n_frames, n_bytes);
  if (rc != GPX_OK) return rc;
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
    /* the columns of just those records: gathered on the host, each waited for before the next is built */
    auto gather = [&](auto* dev, const auto* host) {
      using T = std::decay_t<decltype(*dev)>;
      held.emplace_back(m * sizeof(T));
      T* g = (T*)held.back().data();
      for (size_t r = 0; r < m; r++) g[r] = host[over[r]];
      t.h2d(dev, g, m * sizeof(T));
      t.sync();
    };
    for (int q = 0; q < 6; q++)
      if (src[q]) gather(c[q], src[q]);
    if (req_id) gather(drq, req_id);
    gather(dst, status);
    if (t.rc != GPX_OK) return t.rc;
    held.clear();
    int32_t nf2 = 0;
    int64_t nb2 = 0;
    const int32_t f0 = *n_frames;
    const int64_t b0 = *n_bytes;
    if ((rc = pass(m, f0, b0, &nf2, &nb2)) != GPX_OK) return rc;
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
  const size_t nn = (size_t)n;
  CtlStage t(h);
  const int32_t *c_g = t.in(d_gidx, nn), *c_s = t.in(d_slot, nn), *c_b = t.in(d_bnum, nn), *c_c = t.in(d_bcoord, nn);
  const int32_t* c_m = t.in(d_median_cp, nn);
  const uint8_t* c_k = t.in(d_kind, nn);
  uint8_t* o_out = t.out(out, (size_t)cap_bytes + 4);
  int64_t *o_off = t.out(frame_off, nn), *o_nb = t.out(n_bytes, 1);
  int32_t *o_len = t.out(frame_len, nn), *o_fg = t.out(f_gidx, nn), *o_nf = t.out(n_frames, 1);
  if (t.ready()) return t.rc;
  if (t.ran(gpx_wire_pack_commits_dev(h, n, nullptr, c_g, c_s, c_b, c_c, c_m, c_k, o_out, cap_bytes, o_off, o_len,
                                      o_fg, o_nf, o_nb)))
    return t.rc;
  if (t.fetch({o_nf, o_nb})) return t.rc;
  if (*n_frames < 0) {
    *n_frames = 0;
    return GPX_EINVAL; /* more than GPX_W_MAX_SEG consecutive rows of one group */
  }
  if (*n_bytes > cap_bytes) return GPX_ECAPACITY;
  if (*n_frames == 0) return GPX_OK;
  t.queue(o_out, (size_t)*n_bytes);
  return t.fetch({o_off, o_len, o_fg}, (size_t)*n_frames);
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
