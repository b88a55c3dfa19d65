// Host-pointer side of the view change in list form (include/gpx_viewchange.h): each call staged through CtlStage around
// its *_dev twin (gpx_vclists_dev.inc).  The counts come back first, then only what was written.
// Needs: gpx_host_stage.inc (CtlStage), pl_args / pl_open / prl_* (gpx_vclists_dev.inc).

namespace {

/* The coordinator twins' rounds: _more from `from_hit` into staging of at most vcl_stage_hits hit rows and the entries
 * that go with them, each round's rows copied behind the last one's, until the caller's caps are reached or no hit is
 * left.  A round's caps never exceed what the caller has left, and its entry cap is at least `window` while the caller
 * has that much left: a round that writes nothing means the caller's caps are reached. */
int prl_rounds(gpx_engine* h, CtlStage& t, int32_t from_hit, int32_t cap_hits, int32_t cap_entries, const PrlOut& host,
               gpx_prl_counts* counts) {
  const int64_t W = h->cfg.window, n = h->prl_n;
  const int32_t sh = (int32_t)std::min<int64_t>({(int64_t)cap_hits, n, (int64_t)h->vcl_stage_hits});
  const int32_t se =
      (int32_t)std::min<int64_t>({(int64_t)cap_entries, n * W, std::max<int64_t>(W, 4 * (int64_t)h->vcl_stage_hits)});
  PrlOut D{};
  if (sh > 0) {
    D.h_rec = t.tmp<int32_t>(sh, false), D.h_gidx = t.tmp<int32_t>(sh, false), D.h_kind = t.tmp<uint8_t>(sh, false);
    D.h_status = t.tmp<uint8_t>(sh, false), D.h_median = t.tmp<int32_t>(sh, false), D.h_off = t.tmp<int32_t>(sh, false);
    D.h_count = t.tmp<int32_t>(sh, false);
  }
  if (se > 0) {
    D.e_slot = t.tmp<int32_t>(se, false), D.e_kind = t.tmp<uint8_t>(se, false), D.e_handle = t.tmp<int64_t>(se, false);
    D.e_flags = t.tmp<uint8_t>(se, false);
  }
  if (t.rc != GPX_OK) return t.rc;
  int32_t hd = 0, ed = 0;
  gpx_prl_counts c{};
  for (;;) {
    const int32_t ch = std::min(sh, cap_hits - hd), ce = std::min(se, cap_entries - ed);
    if (t.ran(prl_more(h, from_hit + hd, ch, ce, ed, D, (gpx_prl_counts*)h->prl_counts))) return t.rc;
    t.d2h(&c, h->prl_counts, sizeof(c));
    if (t.sync()) return t.rc;
    const size_t kh = (size_t)std::max(0, std::min(c.hits_done, ch)), ke = (size_t)std::max(0, std::min(c.entries_done, ce));
    if (kh) {
      t.d2h(host.h_rec + hd, D.h_rec, kh * 4), t.d2h(host.h_gidx + hd, D.h_gidx, kh * 4);
      t.d2h(host.h_kind + hd, D.h_kind, kh), t.d2h(host.h_status + hd, D.h_status, kh);
      t.d2h(host.h_median + hd, D.h_median, kh * 4), t.d2h(host.h_off + hd, D.h_off, kh * 4);
      t.d2h(host.h_count + hd, D.h_count, kh * 4);
    }
    if (ke) {
      t.d2h(host.e_slot + ed, D.e_slot, ke * 4), t.d2h(host.e_kind + ed, D.e_kind, ke);
      t.d2h(host.e_handle + ed, D.e_handle, ke * 8), t.d2h(host.e_flags + ed, D.e_flags, ke);
    }
    if ((kh || ke) && t.sync()) return t.rc; /* the staging is rewritten by the next round */
    hd += (int32_t)kh;
    ed += (int32_t)ke;
    if (!kh || (int64_t)from_hit + hd >= c.n_hits || hd >= cap_hits) break;
  }
  c.from_hit = from_hit;
  c.hits_done = hd;
  c.entries_done = ed;
  *counts = c;
  return GPX_OK;
}

}  // namespace

extern "C" {

int gpx_prepare_lists(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* bnum, const int32_t* bcoord,
                      const int32_t* first_slot, int32_t* r_bnum, int32_t* r_bcoord, int32_t* r_gc, uint8_t* r_flags,
                      uint8_t* status, int32_t cap_entries, int32_t* pv_off, int32_t* pv_slot, int32_t* pv_bnum,
                      int32_t* pv_bcoord, gpx_pl_counts* counts) {
  int rc = pl_args(h, n, gidx, bnum, bcoord, first_slot, r_bnum, r_bcoord, r_gc, r_flags, status, cap_entries, pv_off,
                   pv_slot, pv_bnum, pv_bcoord, counts);
  if (rc != GPX_OK) return rc;
  if ((rc = pl_open(h, n)) != GPX_OK) return rc;
  const size_t nn = (size_t)n;
  const size_t m = (size_t)std::min<int64_t>(cap_entries, (int64_t)n * h->cfg.window);
  CtlStage t(h);
  const int32_t *d_g = t.in(gidx, nn), *d_b = t.in(bnum, nn), *d_c = t.in(bcoord, nn), *d_f = t.in(first_slot, nn);
  int32_t *o_b = t.out(r_bnum, nn), *o_c = t.out(r_bcoord, nn), *o_gc = t.out(r_gc, nn);
  uint8_t *o_fl = t.out(r_flags, nn), *o_st = t.out(status, nn);
  /* the lists: written up to the cut and fetched up to the cut, so not cleared */
  int32_t* o_off = pv_off ? t.tmp<int32_t>(nn + 1, false) : nullptr;
  int32_t *o_ps = nullptr, *o_pb = nullptr, *o_pc = nullptr;
  if (m) o_ps = t.tmp<int32_t>(m, false), o_pb = t.tmp<int32_t>(m, false), o_pc = t.tmp<int32_t>(m, false);
  if (t.ready()) return t.rc;
  if (t.ran(gpx_prepare_lists_dev(h, n, d_g, d_b, d_c, d_f, o_b, o_c, o_gc, o_fl, o_st, (int32_t)m, o_off, o_ps, o_pb,
                                  o_pc, (gpx_pl_counts*)h->pl_counts)))
    return t.rc;
  t.d2h(counts, h->pl_counts, sizeof(*counts));
  if (t.sync()) return t.rc;
  if (n) {
    for (const void* d : {(const void*)o_b, (const void*)o_c, (const void*)o_gc, (const void*)o_fl, (const void*)o_st})
      t.queue(d);
  }
  if (o_off) t.d2h(pv_off, o_off, ((size_t)std::min(std::max(0, counts->recs_done), n) + 1) * 4);
  const size_t k = std::min((size_t)std::max(0, counts->entries_done), m);
  if (k) t.d2h(pv_slot, o_ps, k * 4), t.d2h(pv_bnum, o_pb, k * 4), t.d2h(pv_bcoord, o_pc, k * 4);
  return t.sync();
}

int gpx_prepare_reply_lists(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* acceptor,
                            const int32_t* r_bnum, const int32_t* r_bcoord, const int32_t* first_slot,
                            const int32_t* pv_off, const int32_t* pv_slot, const int32_t* pv_bnum,
                            const int32_t* pv_bcoord, const int64_t* pv_handle, const uint8_t* pv_flags, uint8_t* v_kind,
                            uint8_t* status, int32_t cap_hits, int32_t cap_entries, int32_t* h_rec, int32_t* h_gidx,
                            uint8_t* h_kind, uint8_t* h_status, int32_t* h_median, int32_t* h_off, int32_t* h_count,
                            int32_t* e_slot, uint8_t* e_kind, int64_t* e_handle, uint8_t* e_flags,
                            gpx_prl_counts* counts) {
  const PrlOut O{h_rec, h_gidx, h_kind, h_status, h_median, h_off, h_count, e_slot, e_kind, e_handle, e_flags};
  int rc = prl_out_args(h, 0, cap_hits, cap_entries, O, counts);
  if (rc != GPX_OK) return rc;
  if ((rc = prl_in_args(n, gidx, acceptor, r_bnum, r_bcoord, first_slot, pv_off, 0, nullptr, nullptr, nullptr)) != GPX_OK)
    return rc;
  size_t m = 0;
  if (n > 0) {
    if (pv_off[0] != 0) return GPX_EINVAL;
    for (int32_t i = 0; i < n; i++)
      if (pv_off[i + 1] < pv_off[i]) return GPX_EINVAL;
    m = (size_t)pv_off[n];
    if (m && (!pv_slot || !pv_bnum || !pv_bcoord)) return GPX_EINVAL;
  }
  if ((rc = prl_open(h, n)) != GPX_OK) return rc;
  const size_t nn = (size_t)n;
  CtlStage t(h);
  const int32_t *d_g = t.in(gidx, nn), *d_a = t.in(acceptor, nn), *d_rb = t.in(r_bnum, nn), *d_rc = t.in(r_bcoord, nn);
  const int32_t *d_f = t.in(first_slot, nn), *d_off = t.in(pv_off, n ? nn + 1 : 0);
  const int32_t *d_ps = t.in(pv_slot, m), *d_pb = t.in(pv_bnum, m), *d_pc = t.in(pv_bcoord, m);
  const int64_t* d_ph = t.in_opt(pv_handle, m);
  const uint8_t* d_pf = t.in_opt(pv_flags, m);
  uint8_t *o_vk = (v_kind && n) ? t.out(v_kind, nn) : nullptr, *o_st = (status && n) ? t.out(status, nn) : nullptr;
  if (t.ready()) return t.rc;
  if (t.ran(prl_apply(h, n, d_g, d_a, d_rb, d_rc, d_f, d_off, (int32_t)m, d_ps, d_pb, d_pc, d_ph, d_pf, o_vk, o_st)))
    return t.rc;
  if (o_vk) t.queue(o_vk);
  if (o_st) t.queue(o_st);
  return prl_rounds(h, t, 0, cap_hits, cap_entries, O, counts);
}

int gpx_prepare_reply_lists_more(gpx_engine* h, int32_t from_hit, int32_t cap_hits, int32_t cap_entries, int32_t* h_rec,
                                 int32_t* h_gidx, uint8_t* h_kind, uint8_t* h_status, int32_t* h_median, int32_t* h_off,
                                 int32_t* h_count, int32_t* e_slot, uint8_t* e_kind, int64_t* e_handle, uint8_t* e_flags,
                                 gpx_prl_counts* counts) {
  const PrlOut O{h_rec, h_gidx, h_kind, h_status, h_median, h_off, h_count, e_slot, e_kind, e_handle, e_flags};
  int rc = prl_out_args(h, from_hit, cap_hits, cap_entries, O, counts);
  if (rc != GPX_OK) return rc;
  if (h->prl_n < 0 || !h->prl_counts) return GPX_EINVAL; /* nothing parked */
  if ((rc = check_batch(h, 0)) != GPX_OK) return rc;
  CtlStage t(h);
  return prl_rounds(h, t, from_hit, cap_hits, cap_entries, O, counts);
}

} /* extern "C" */
