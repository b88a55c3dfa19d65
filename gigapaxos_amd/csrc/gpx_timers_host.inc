// Host-pointer side of the retransmission sweep (include/gpx_timers.h), staged through CtlStage around
// gpx_retransmit_sweep_dev.
// Needs: gpx_host_stage.inc (CtlStage), rtx_args / rtx_open (gpx_timers_dev.inc).

extern "C" {

int gpx_retransmit_sweep(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t now_ms, const gpx_rtx_cfg* cfg,
                         int32_t flags, int32_t cap, int32_t* o_gidx, uint8_t* o_poke, int32_t* o_slot, int32_t* o_bnum,
                         int32_t* o_bcoord, int32_t* o_median_cp, uint8_t* o_flags, uint32_t* o_heard, uint8_t* o_count,
                         int32_t* o_waited, gpx_rtx_counts* counts) {
  int rc = rtx_args(h, n, cfg, flags, cap,
                    {o_gidx, o_poke, o_slot, o_bnum, o_bcoord, o_median_cp, o_flags, o_heard, o_count, o_waited}, counts);
  if (rc != GPX_OK) return rc;
  if ((rc = rtx_open(h, n)) != GPX_OK) return rc;
  CtlStage t(h);
  const int32_t m = std::min(cap, n);
  const size_t mm = (size_t)std::max(m, 0);
  const int32_t* d_g = n ? t.in_opt(gidx, (size_t)n) : nullptr;
  int32_t* d_og = m > 0 ? t.out(o_gidx, mm) : nullptr;
  uint8_t* d_pk = m > 0 ? t.out(o_poke, mm) : nullptr;
  int32_t* d_sl = m > 0 ? t.out(o_slot, mm) : nullptr;
  int32_t* d_bn = m > 0 ? t.out(o_bnum, mm) : nullptr;
  int32_t* d_bc = m > 0 ? t.out(o_bcoord, mm) : nullptr;
  int32_t* d_md = m > 0 ? t.out(o_median_cp, mm) : nullptr;
  uint8_t* d_fl = m > 0 ? t.out(o_flags, mm) : nullptr;
  uint32_t* d_hd = m > 0 ? t.out(o_heard, mm) : nullptr;
  uint8_t* d_ct = m > 0 ? t.out(o_count, mm) : nullptr;
  int32_t* d_wt = m > 0 ? t.out(o_waited, mm) : nullptr;
  if (t.ready()) return t.rc;
  if (t.ran(gpx_retransmit_sweep_dev(h, n, d_g, now_ms, cfg, flags, m, d_og, d_pk, d_sl, d_bn, d_bc, d_md, d_fl, d_hd, d_ct,
                                     d_wt, (gpx_rtx_counts*)h->rtx_counts)))
    return t.rc;
  t.d2h(counts, h->rtx_counts, sizeof(*counts));
  if (t.sync()) return t.rc;
  /* the device saw min(cap, n) as its capacity; a count of hits is at most n: n_fired is already min(n_hits, cap) */
  const size_t k = (size_t)std::max(0, std::min(counts->n_hits, m));
  if (!k) return GPX_OK;
  return t.fetch({d_og, d_pk, d_sl, d_bn, d_bc, d_md, d_fl, d_hd, d_ct, d_wt}, k);
}

} /* extern "C" */
