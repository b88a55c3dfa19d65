// Host-pointer side of the deactivation sweep (include/gpx_sweep.h), staged through CtlStage around gpx_pause_sweep_dev.
// Needs: gpx_host_stage.inc (CtlStage), sweep_args (gpx_ctl_args.inc), sweep_open (gpx_sweep_dev.inc).

extern "C" {

int gpx_pause_sweep(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t min_age, int32_t flags, int32_t cap,
                    int32_t* o_gidx, uint8_t* o_age, gpx_hri* o_rows, gpx_sweep_counts* counts) {
  int rc = sweep_args(h, n, min_age, flags, cap, o_gidx, o_age, o_rows, counts);
  if (rc != GPX_OK) return rc;
  if ((rc = sweep_open(h, n)) != GPX_OK) return rc;
  CtlStage t(h);
  const int32_t m = std::min(cap, n);
  const int32_t* d_g = n ? t.in_opt(gidx, (size_t)n) : nullptr;
  int32_t* d_og = m > 0 ? t.out(o_gidx, (size_t)m) : nullptr;
  uint8_t* d_oa = m > 0 ? t.out(o_age, (size_t)m) : nullptr;
  gpx_hri* d_or = m > 0 ? t.out(o_rows, (size_t)m) : nullptr;
  if (t.ready()) return t.rc;
  if (t.ran(gpx_pause_sweep_dev(h, n, d_g, min_age, flags, m, d_og, d_oa, d_or, (gpx_sweep_counts*)h->sweep_counts)))
    return t.rc;
  t.d2h(counts, h->sweep_counts, sizeof(*counts));
  if (t.sync()) return t.rc;
  /* the device saw min(cap, n) as its capacity; a count of hits is at most n: n_paused is already min(n_hits, cap) */
  const size_t k = (size_t)std::max(0, std::min(counts->n_hits, m));
  if (!k) return GPX_OK;
  return t.fetch({d_og, d_oa, d_or}, k);
}

} /* extern "C" */
