// Host-pointer side of the checkpoint transfer (include/gpx_checkpoint.h), staged through CtlStage around
// gpx_checkpoint_batch_dev.  Needs: gpx_host_stage.inc (CtlStage), cp_args / cp_open (gpx_checkpoint_dev.inc).

extern "C" {

int gpx_checkpoint_batch(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* cp_slot, int32_t flags,
                         int32_t* o_from, int32_t* o_to, uint8_t* o_flags, uint8_t* status, int32_t* x_gidx,
                         int32_t* x_first, int32_t* x_count, gpx_cp_counts* counts) {
  int rc = cp_args(h, n, gidx, cp_slot, flags, o_from, o_to, o_flags, status, x_gidx, x_first, x_count, counts);
  if (rc != GPX_OK) return rc;
  if ((rc = cp_open(h, n)) != GPX_OK) return rc;
  CtlStage t(h);
  const size_t m = (size_t)n;
  const bool runs = !(flags & GPX_CP_PEEK);
  const int32_t* d_g = t.in(gidx, m);
  const int32_t* d_c = t.in(cp_slot, m);
  /* not filled: the kernels write every dense entry below n, and only run entries below n_runs are fetched */
  int32_t* d_from = t.tmp<int32_t>(m, false);
  int32_t* d_to = t.tmp<int32_t>(m, false);
  uint8_t* d_fl = t.tmp<uint8_t>(m, false);
  uint8_t* d_st = t.tmp<uint8_t>(m, false);
  int32_t* d_xg = runs ? t.tmp<int32_t>(m, false) : nullptr;
  int32_t* d_xf = runs ? t.tmp<int32_t>(m, false) : nullptr;
  int32_t* d_xc = runs ? t.tmp<int32_t>(m, false) : nullptr;
  if (t.ready()) return t.rc;
  if (t.ran(gpx_checkpoint_batch_dev(h, n, d_g, d_c, flags, d_from, d_to, d_fl, d_st, d_xg, d_xf, d_xc,
                                     (gpx_cp_counts*)h->cp_counts)))
    return t.rc;
  t.d2h(counts, h->cp_counts, sizeof(*counts));
  if (m) {
    t.d2h(o_from, d_from, m * 4);
    t.d2h(o_to, d_to, m * 4);
    t.d2h(o_flags, d_fl, m);
    t.d2h(status, d_st, m);
  }
  if (t.sync()) return t.rc;
  const size_t k = runs ? (size_t)std::max(0, std::min(counts->n_runs, n)) : 0;
  if (!k) return GPX_OK;
  t.d2h(x_gidx, d_xg, k * 4);
  t.d2h(x_first, d_xf, k * 4);
  t.d2h(x_count, d_xc, k * 4);
  return t.sync();
}

} /* extern "C" */
