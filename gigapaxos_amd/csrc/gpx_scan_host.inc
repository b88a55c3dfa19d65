// Host-pointer side of the table scans: the dense election, gap and poke scans of include/gpx.h and their hit-compacting
// forms of include/gpx_scan.h, each staged through CtlStage.
// Needs: gpx_host_stage.inc (CtlStage), scan_args / scan_lists (gpx_ctl_args.inc), scan_open (gpx_scan_dev.inc), LAUNCH, grid_for.

namespace {

/* A hit-compacting twin: the scanned list in, the _dev form into temporaries of min(cap, n) entries, the counts out, then
 * min(n_hits, cap) entries per column.  `dev(d_gidx, m, cols, d_counts)` queues the _dev form; cols[q] has
 * size[q] bytes per entry and goes to host[q]. */
template <class F>
int scan_host(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t cap, int ncols, void* const* host,
              const int* size, gpx_scan_counts* counts, F dev) {
  int rc = scan_open(h, n);
  if (rc != GPX_OK) return rc;
  CtlStage t(h);
  const int32_t m = std::min(cap, n);
  const int32_t* d_g = n ? t.in_opt(gidx, (size_t)n) : nullptr;
  void* cols[8] = {};
  for (int q = 0; q < ncols && m > 0; q++) cols[q] = t.out_bytes(host[q], (size_t)m, (size_t)size[q]);
  if (t.ready()) return t.rc;
  if (t.ran(dev(d_g, m, cols, (gpx_scan_counts*)h->scan_counts))) return t.rc;
  t.d2h(counts, h->scan_counts, sizeof(*counts));
  if (t.sync()) return t.rc;
  const size_t k = (size_t)std::max(0, std::min(counts->n_hits, m));
  if (!k) return GPX_OK;
  for (int q = 0; q < ncols; q++) t.queue(cols[q], k);
  return t.sync();
}

}  // namespace

extern "C" {

int gpx_election_scan(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* down_nodes,
                      int32_t n_down, const int32_t* long_dead_nodes, int32_t n_long_dead,
                      int32_t force, uint8_t* run, int32_t* p_bnum, int32_t* p_first,
                      uint8_t* status) {
  if (!h || n < 0 || n_down < 0 || n_long_dead < 0) return GPX_EINVAL;
  if (n_down > GPX_MAX_NODE_LIST || n_long_dead > GPX_MAX_NODE_LIST) return GPX_ECAPACITY;
  if (n == 0) return GPX_OK;
  if (!run || !p_bnum || !p_first || !status) return GPX_EINVAL;
  NodeLists L;
  int rc = scan_lists(down_nodes, n_down, long_dead_nodes, n_long_dead, &L);
  if (rc != GPX_OK) return rc;
  const size_t nn = (size_t)n;
  CtlStage t(h);
  const int32_t* d_g = t.in_opt(gidx, nn);
  uint8_t *d_r = t.out(run, nn), *d_s = t.out(status, nn);
  int32_t *d_b = t.out(p_bnum, nn), *d_f = t.out(p_first, nn);
  if (t.ready()) return t.rc;
  LAUNCH(h, "k_election_scan", k_election_scan, grid_for(n), h->S, n, d_g, L, force, d_r, d_b, d_f, d_s);
  return t.fetch({d_r, d_b, d_f, d_s});
}

int gpx_gap_scan(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t threshold,
                 int32_t sync_mode, int32_t size_limit, int32_t* first_slot,
                 int32_t* max_committed, uint64_t* missing, uint8_t* should_sync, uint8_t* status) {
  if (!h || n < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (!gidx || !first_slot || !max_committed || !missing || !should_sync || !status) return GPX_EINVAL;
  const size_t nn = (size_t)n;
  CtlStage t(h);
  const int32_t* d_g = t.in(gidx, nn);
  int32_t *d_f = t.out(first_slot, nn), *d_m = t.out(max_committed, nn);
  unsigned long long* d_mi = t.out((unsigned long long*)missing, nn);
  uint8_t *d_sy = t.out(should_sync, nn), *d_st = t.out(status, nn);
  if (t.ready()) return t.rc;
  LAUNCH(h, "k_gap_scan", k_gap_scan, grid_for(n), h->S, n, d_g, threshold, sync_mode, size_limit, d_f, d_m, d_mi, d_sy,
         d_st);
  return t.fetch({d_f, d_m, d_mi, d_sy, d_st});
}

int gpx_poke_scan(gpx_engine* h, int32_t n, const int32_t* gidx, uint8_t* poke, int32_t* slot,
                  int32_t* bnum, int32_t* bcoord, int32_t* median_cp, uint8_t* p_flags,
                  uint32_t* heard, uint8_t* status) {
  if (!h || n < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (!poke || !slot || !bnum || !bcoord || !median_cp || !p_flags || !heard || !status) return GPX_EINVAL;
  const size_t nn = (size_t)n;
  CtlStage t(h);
  const int32_t* d_g = t.in_opt(gidx, nn);
  uint8_t *d_pk = t.out(poke, nn), *d_fl = t.out(p_flags, nn), *d_st = t.out(status, nn);
  int32_t *d_sl = t.out(slot, nn), *d_bn = t.out(bnum, nn), *d_bc = t.out(bcoord, nn), *d_md = t.out(median_cp, nn);
  uint32_t* d_hd = t.out(heard, nn);
  if (t.ready()) return t.rc;
  if (h->cfg.kmax <= 4)
    LAUNCH(h, "k_poke_scan", k_poke_scan<4>, grid_for(n), h->S, n, d_g, d_pk, d_sl, d_bn, d_bc, d_md, d_fl, d_hd, d_st);
  else if (h->cfg.kmax <= 8)
    LAUNCH(h, "k_poke_scan", k_poke_scan<8>, grid_for(n), h->S, n, d_g, d_pk, d_sl, d_bn, d_bc, d_md, d_fl, d_hd, d_st);
  else
    LAUNCH(h, "k_poke_scan", k_poke_scan<16>, grid_for(n), h->S, n, d_g, d_pk, d_sl, d_bn, d_bc, d_md, d_fl, d_hd, d_st);
  return t.fetch({d_pk, d_sl, d_bn, d_bc, d_md, d_fl, d_hd, d_st});
}

int gpx_election_scan_hits(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* down_nodes, int32_t n_down,
                           const int32_t* long_dead_nodes, int32_t n_long_dead, int32_t force, int32_t cap,
                           int32_t* o_gidx, uint8_t* o_run, int32_t* o_bnum, int32_t* o_first,
                           gpx_scan_counts* counts) {
  int rc = scan_args(h, n, cap, counts, {o_gidx, o_run, o_bnum, o_first});
  if (rc != GPX_OK) return rc;
  NodeLists L;
  if ((rc = scan_lists(down_nodes, n_down, long_dead_nodes, n_long_dead, &L)) != GPX_OK) return rc;
  void* const host[4] = {o_gidx, o_run, o_bnum, o_first};
  const int size[4] = {4, 1, 4, 4};
  return scan_host(h, n, gidx, cap, 4, host, size, counts,
                   [&](const int32_t* d_g, int32_t m, void* const* c, gpx_scan_counts* d_counts) {
                     return gpx_election_scan_hits_dev(h, n, d_g, down_nodes, n_down, long_dead_nodes, n_long_dead, force,
                                                       m, (int32_t*)c[0], (uint8_t*)c[1], (int32_t*)c[2], (int32_t*)c[3],
                                                       d_counts);
                   });
}

int gpx_poke_scan_hits(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t cap, int32_t* o_gidx, uint8_t* o_poke,
                       int32_t* o_slot, int32_t* o_bnum, int32_t* o_bcoord, int32_t* o_median_cp, uint8_t* o_flags,
                       uint32_t* o_heard, gpx_scan_counts* counts) {
  int rc = scan_args(h, n, cap, counts, {o_gidx, o_poke, o_slot, o_bnum, o_bcoord, o_median_cp, o_flags, o_heard});
  if (rc != GPX_OK) return rc;
  void* const host[8] = {o_gidx, o_poke, o_slot, o_bnum, o_bcoord, o_median_cp, o_flags, o_heard};
  const int size[8] = {4, 1, 4, 4, 4, 4, 1, 4};
  return scan_host(h, n, gidx, cap, 8, host, size, counts,
                   [&](const int32_t* d_g, int32_t m, void* const* c, gpx_scan_counts* d_counts) {
                     return gpx_poke_scan_hits_dev(h, n, d_g, m, (int32_t*)c[0], (uint8_t*)c[1], (int32_t*)c[2],
                                                   (int32_t*)c[3], (int32_t*)c[4], (int32_t*)c[5], (uint8_t*)c[6],
                                                   (uint32_t*)c[7], d_counts);
                   });
}

int gpx_gap_scan_hits(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t threshold, int32_t sync_mode,
                      int32_t size_limit, int32_t require, int32_t cap, int32_t* o_gidx, int32_t* o_first,
                      int32_t* o_max_committed, uint64_t* o_missing, uint8_t* o_sync, gpx_scan_counts* counts) {
  int rc = scan_args(h, n, cap, counts, {o_gidx, o_first, o_max_committed, o_missing, o_sync});
  if (rc != GPX_OK) return rc;
  void* const host[5] = {o_gidx, o_first, o_max_committed, o_missing, o_sync};
  const int size[5] = {4, 4, 4, 8, 1};
  return scan_host(h, n, gidx, cap, 5, host, size, counts,
                   [&](const int32_t* d_g, int32_t m, void* const* c, gpx_scan_counts* d_counts) {
                     return gpx_gap_scan_hits_dev(h, n, d_g, threshold, sync_mode, size_limit, require, m,
                                                  (int32_t*)c[0], (int32_t*)c[1], (int32_t*)c[2], (uint64_t*)c[3],
                                                  (uint8_t*)c[4], d_counts);
                   });
}

} /* extern "C" */
