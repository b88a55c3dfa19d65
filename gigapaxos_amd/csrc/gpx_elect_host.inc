// Host-pointer side of the coordinator half of the view change (include/gpx.h, "view change, coordinator side"): each
// call staged through CtlStage around its *_dev twin (gpx_elect_dev.inc).  Needs: gpx_host_stage.inc (CtlStage), check_batch.

extern "C" {

int gpx_election_begin(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* bnum,
                       uint8_t* e_status) {
  if (!h || n < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (!gidx || !bnum || !e_status) return GPX_EINVAL;
  { /* one record per group: two records of one group would race (each is handled by its own lane) */
    std::vector<int32_t> sorted(gidx, gidx + n);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return GPX_EINVAL;
  }
  const size_t nn = (size_t)n;
  CtlStage t(h);
  const int32_t *d_g = t.in(gidx, nn), *d_b = t.in(bnum, nn);
  uint8_t* d_s = t.out(e_status, nn);
  if (t.ready()) return t.rc;
  /* no wait here: apply_streams makes the engine's front, back and launch streams one stream, the twin runs behind the copies */
  if (t.ran(gpx_election_begin_dev(h, n, d_g, d_b, d_s))) return t.rc;
  return t.fetch({d_s});
}

int gpx_prepare_reply_batch(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* acceptor,
                            const int32_t* r_bnum, const int32_t* r_bcoord, const int32_t* first_slot,
                            const int32_t* pv_off, const int32_t* pv_slot, const int32_t* pv_bnum,
                            const int32_t* pv_bcoord, const int64_t* pv_handle,
                            const uint8_t* pv_flags, uint8_t* v_kind, int32_t* e_count,
                            int32_t* e_median, int32_t* e_slot, uint8_t* e_kind, int64_t* e_handle,
                            uint8_t* e_flags, uint8_t* status) {
  int rc = check_batch(h, n);
  if (rc != GPX_OK) return rc;
  if (n == 0) return GPX_OK;
  if (!gidx || !acceptor || !r_bnum || !r_bcoord || !first_slot || !pv_off || !v_kind || !e_count ||
      !e_median || !e_slot || !e_kind || !e_handle || !e_flags || !status)
    return GPX_EINVAL;
  if (pv_off[0] != 0) return GPX_EINVAL;
  for (int32_t i = 0; i < n; i++)
    if (pv_off[i + 1] < pv_off[i]) return GPX_EINVAL;
  const size_t m = (size_t)pv_off[n];
  if (m && (!pv_slot || !pv_bnum || !pv_bcoord)) return GPX_EINVAL;
  const size_t nn = (size_t)n, nw = nn * (size_t)h->S.W;
  CtlStage t(h);
  const int32_t *d_g = t.in(gidx, nn), *d_a = t.in(acceptor, nn), *d_rb = t.in(r_bnum, nn), *d_rc = t.in(r_bcoord, nn);
  const int32_t *d_f = t.in(first_slot, nn), *d_off = t.in(pv_off, nn + 1);
  /* the pvalues: m of them in all, none is a column of no entries (and may then be null) */
  const int32_t *d_ps = t.in(pv_slot, m), *d_pb = t.in(pv_bnum, m), *d_pc = t.in(pv_bcoord, m);
  const int64_t* d_ph = t.in_opt(pv_handle, m);
  const uint8_t* d_pf = t.in_opt(pv_flags, m);
  uint8_t *o_vk = t.out(v_kind, nn), *o_st = t.out(status, nn);
  int32_t *o_ec = t.out(e_count, nn), *o_em = t.out(e_median, nn), *o_es = t.out(e_slot, nw);
  uint8_t *o_ek = t.out(e_kind, nw), *o_ef = t.out(e_flags, nw);
  int64_t* o_eh = t.out(e_handle, nw);
  if (t.ready()) return t.rc;
  /* no wait here either: the twin's front end runs on the one stream the copies above were queued on (apply_streams) */
  if (t.ran(gpx_prepare_reply_batch_dev(h, n, d_g, d_a, d_rb, d_rc, d_f, d_off, (int32_t)m, d_ps, d_pb, d_pc, d_ph, d_pf,
                                        o_vk, o_ec, o_em, o_es, o_ek, o_eh, o_ef, o_st)))
    return t.rc;
  return t.fetch({o_vk, o_st, o_ec, o_em, o_es, o_ek, o_ef, o_eh});
}

} /* extern "C" */
