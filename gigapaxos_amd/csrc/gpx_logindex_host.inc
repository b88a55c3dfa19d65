// Host-pointer side of the log index (include/gpx_logindex.h), staged through CtlStage around the _dev calls: the
// columns go in, the counts and only what was written come back.  Every twin waits for its call, so the counts it
// fetched are the index's state and the host's bound of the tail becomes exact.
// Needs: gpx_host_stage.inc (CtlStage), the li_*_args checks and the _dev calls (gpx_logindex_dev.inc).

namespace {

/* the counts of the call just queued, then the wait; the tail is known exactly afterwards */
int li_fetch_counts(gpx_engine* h, CtlStage& t, gpx_logindex_counts* counts) {
  t.d2h(counts, h->li_counts, sizeof(*counts));
  if (t.sync()) return t.rc;
  h->li_ub = std::max(0, std::min(counts->n_rows, h->li.cap_rows));
  return GPX_OK;
}

/* the records a call with n_dev takes, on the host */
int32_t li_taken_host(int32_t n, const int32_t* n_dev) { return n_dev ? std::min(n, std::max(*n_dev, 0)) : n; }

}  // namespace

extern "C" {

int gpx_logindex_add(gpx_engine* h, int32_t n, const int32_t* n_dev, const int32_t* e_gidx, const int32_t* e_slot,
                     const int32_t* e_bnum, const int32_t* e_bcoord, const int64_t* e_off, const int32_t* e_len,
                     int32_t file, uint8_t* status, gpx_logindex_counts* counts) {
  int rc = li_add_args(h, n, e_gidx, e_slot, e_bnum, e_bcoord, e_off, e_len, file, counts);
  if (rc != GPX_OK) return rc;
  const int32_t m = li_taken_host(n, n_dev); /* only the records taken cross the link */
  const size_t mm = (size_t)m;
  CtlStage t(h);
  const int32_t *d_g = nullptr, *d_s = nullptr, *d_bn = nullptr, *d_bc = nullptr, *d_l = nullptr;
  const int64_t* d_o = nullptr;
  uint8_t* d_st = nullptr;
  if (m) {
    d_g = t.in(e_gidx, mm), d_s = t.in(e_slot, mm), d_bn = t.in(e_bnum, mm), d_bc = t.in(e_bcoord, mm);
    d_o = t.in(e_off, mm), d_l = t.in(e_len, mm);
    if (status) d_st = t.out(status, mm);
  }
  if (t.ready()) return t.rc;
  if (t.ran(gpx_logindex_add_dev(h, m, nullptr, d_g, d_s, d_bn, d_bc, d_o, d_l, file, d_st,
                                 (gpx_logindex_counts*)h->li_counts)))
    return t.rc;
  if ((rc = li_fetch_counts(h, t, counts)) != GPX_OK) return rc;
  return d_st ? t.fetch({d_st}) : GPX_OK;
}

int gpx_logindex_set_gc(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* gc_slot, int32_t flags,
                        uint8_t* status, gpx_logindex_counts* counts) {
  int rc = li_set_gc_args(h, n, gidx, gc_slot, flags, counts);
  if (rc != GPX_OK) return rc;
  const size_t nn = (size_t)n;
  CtlStage t(h);
  const int32_t* d_g = n ? t.in(gidx, nn) : nullptr;
  const int32_t* d_c = n ? t.in_opt(gc_slot, nn) : nullptr;
  uint8_t* d_st = n && status ? t.out(status, nn) : nullptr;
  if (t.ready()) return t.rc;
  if (t.ran(gpx_logindex_set_gc_dev(h, n, d_g, d_c, flags, d_st, (gpx_logindex_counts*)h->li_counts))) return t.rc;
  if ((rc = li_fetch_counts(h, t, counts)) != GPX_OK) return rc;
  return d_st ? t.fetch({d_st}) : GPX_OK;
}

int gpx_logindex_lookup(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* min_slot, const int32_t* max_slot,
                        const uint8_t* has_max, int32_t cap, int32_t* o_rec, int32_t* o_row, int32_t* o_slot,
                        int32_t* o_bnum, int32_t* o_bcoord, int32_t* o_file, int64_t* o_off, int32_t* o_len,
                        uint8_t* status, gpx_logindex_counts* counts) {
  int rc = li_lookup_args(h, n, gidx, min_slot, max_slot, has_max, cap,
                          {o_rec, o_row, o_slot, o_bnum, o_bcoord, o_file, o_off, o_len}, counts);
  if (rc != GPX_OK) return rc;
  const size_t nn = (size_t)n;
  /* no more hits than rows: the device sees min(cap, the bound of the tail) as its capacity */
  const int32_t m = (int32_t)std::min<int64_t>(cap, h->li_ub);
  const size_t mm = (size_t)m;
  CtlStage t(h);
  const int32_t* d_g = n ? t.in(gidx, nn) : nullptr;
  const int32_t* d_lo = n ? t.in(min_slot, nn) : nullptr;
  const int32_t* d_hi = n ? t.in_opt(max_slot, nn) : nullptr;
  const uint8_t* d_hm = n ? t.in_opt(has_max, nn) : nullptr;
  uint8_t* d_st = n && status ? t.out(status, nn) : nullptr;
  int32_t *d_rec = nullptr, *d_row = nullptr, *d_sl = nullptr, *d_bn = nullptr, *d_bc = nullptr, *d_f = nullptr,
          *d_l = nullptr;
  int64_t* d_o = nullptr;
  if (m > 0) {
    d_rec = t.out(o_rec, mm), d_row = t.out(o_row, mm), d_sl = t.out(o_slot, mm), d_bn = t.out(o_bnum, mm);
    d_bc = t.out(o_bcoord, mm), d_f = t.out(o_file, mm), d_o = t.out(o_off, mm), d_l = t.out(o_len, mm);
  }
  if (t.ready()) return t.rc;
  if (t.ran(gpx_logindex_lookup_dev(h, n, d_g, d_lo, d_hi, d_hm, m, d_rec, d_row, d_sl, d_bn, d_bc, d_f, d_o, d_l, d_st,
                                    (gpx_logindex_counts*)h->li_counts)))
    return t.rc;
  if ((rc = li_fetch_counts(h, t, counts)) != GPX_OK) return rc;
  if (d_st) t.queue(d_st);
  const size_t k = (size_t)std::max(0, std::min(counts->n_done, m));
  if (k)
    for (const void* d : {(const void*)d_rec, (const void*)d_row, (const void*)d_sl, (const void*)d_bn, (const void*)d_bc,
                          (const void*)d_f, (const void*)d_o, (const void*)d_l})
      t.queue(d, k);
  return t.sync();
}

int gpx_logindex_file_rows(gpx_engine* h, int32_t file, int32_t cap, int32_t* o_row, int32_t* e_gidx, int32_t* e_slot,
                           int32_t* e_bnum, int32_t* e_bcoord, int64_t* e_off, int32_t* e_len, int32_t* e_gc,
                           gpx_logindex_counts* counts) {
  int rc = li_file_rows_args(h, cap, {o_row, e_gidx, e_slot, e_bnum, e_bcoord, e_off, e_len, e_gc}, counts);
  if (rc != GPX_OK) return rc;
  const int32_t m = (int32_t)std::min<int64_t>(cap, h->li_ub);
  const size_t mm = (size_t)m;
  CtlStage t(h);
  int32_t *d_row = nullptr, *d_g = nullptr, *d_sl = nullptr, *d_bn = nullptr, *d_bc = nullptr, *d_l = nullptr,
          *d_gc = nullptr;
  int64_t* d_o = nullptr;
  if (m > 0) {
    d_row = t.out(o_row, mm), d_g = t.out(e_gidx, mm), d_sl = t.out(e_slot, mm), d_bn = t.out(e_bnum, mm);
    d_bc = t.out(e_bcoord, mm), d_o = t.out(e_off, mm), d_l = t.out(e_len, mm), d_gc = t.out(e_gc, mm);
  }
  if (t.ready()) return t.rc;
  if (t.ran(gpx_logindex_file_rows_dev(h, file, m, d_row, d_g, d_sl, d_bn, d_bc, d_o, d_l, d_gc,
                                       (gpx_logindex_counts*)h->li_counts)))
    return t.rc;
  if ((rc = li_fetch_counts(h, t, counts)) != GPX_OK) return rc;
  const size_t k = (size_t)std::max(0, std::min(counts->n_done, m));
  if (!k) return GPX_OK;
  return t.fetch({d_row, d_g, d_sl, d_bn, d_bc, d_o, d_l, d_gc}, k);
}

int gpx_logindex_relocate(gpx_engine* h, int32_t n, const int32_t* n_dev, int32_t generation, const int32_t* o_row,
                          const int32_t* k_src, int32_t new_file, const int64_t* k_off, const int32_t* k_len,
                          gpx_logindex_counts* counts) {
  int rc = li_relocate_args(h, n, o_row, new_file, k_off, k_len, counts);
  if (rc != GPX_OK) return rc;
  const size_t nn = (size_t)n;
  CtlStage t(h);
  const int32_t* d_n = n_dev ? t.in(n_dev, 1) : nullptr;
  const int32_t* d_row = n ? t.in(o_row, nn) : nullptr;
  const int32_t* d_src = n ? t.in_opt(k_src, nn) : nullptr;
  const int64_t* d_o = n ? t.in(k_off, nn) : nullptr;
  const int32_t* d_l = n ? t.in(k_len, nn) : nullptr;
  if (t.ready()) return t.rc;
  if (t.ran(gpx_logindex_relocate_dev(h, n, d_n, generation, d_row, d_src, new_file, d_o, d_l,
                                      (gpx_logindex_counts*)h->li_counts)))
    return t.rc;
  return li_fetch_counts(h, t, counts);
}

int gpx_logindex_files(gpx_engine* h, int32_t file_base, int32_t n_files, int32_t* o_rows, int32_t* o_groups,
                       int32_t* o_min_file, gpx_logindex_counts* counts) {
  int rc = li_files_args(h, n_files, counts);
  if (rc != GPX_OK) return rc;
  const size_t nf = (size_t)n_files;
  CtlStage t(h);
  int32_t* d_r = n_files && o_rows ? t.out(o_rows, nf) : nullptr;
  int32_t* d_g = n_files && o_groups ? t.out(o_groups, nf) : nullptr;
  int32_t* d_m = o_min_file ? t.out(o_min_file, 1) : nullptr;
  if (t.ready()) return t.rc;
  if (t.ran(gpx_logindex_files_dev(h, file_base, n_files, d_r, d_g, d_m, (gpx_logindex_counts*)h->li_counts)))
    return t.rc;
  if ((rc = li_fetch_counts(h, t, counts)) != GPX_OK) return rc;
  if (d_r) t.queue(d_r);
  if (d_g) t.queue(d_g);
  if (d_m) t.queue(d_m);
  return t.sync();
}

int gpx_logindex_compact(gpx_engine* h, gpx_logindex_counts* counts) {
  int rc = li_common(h, counts, 0);
  if (rc != GPX_OK) return rc;
  CtlStage t(h);
  if (t.ran(gpx_logindex_compact_dev(h, (gpx_logindex_counts*)h->li_counts))) return t.rc;
  return li_fetch_counts(h, t, counts);
}

} /* extern "C" */
