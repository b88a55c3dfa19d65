// Device-pointer side of the coordinator half of the view change (include/gpx.h, "view change, coordinator side"); the
// host-pointer twins: gpx_elect_host.inc.  Needs: the engine and the kernels of gpx_engine.hip.

namespace {

/* carried-over pvalues, heard-from masks and pre-active handles: allocated by the first election */
int elect_init(gpx_engine* e) {
  if (e->S.c_wait) return GPX_OK;
  const size_t G = (size_t)e->cfg.max_groups, W = (size_t)e->cfg.window;
  int rc;
  I4* co = nullptr;
  int64_t *coh = nullptr, *ph = nullptr;
  uint32_t* cw = nullptr;
  if ((rc = dev_alloc(e, &co, G * W, true)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &coh, G * W, true)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &ph, G * W, true)) != GPX_OK) return rc;
  if ((rc = dev_alloc(e, &cw, G, true)) != GPX_OK) return rc;
  e->S.co_ring = co;
  e->S.co_handle = coh;
  e->S.p_handle = ph;
  e->S.c_wait = cw; /* last: the marker */
  return GPX_OK;
}

template <int KMAX>
void launch_bucket_prepare_reply(gpx_engine* e, const PReplyIn& I, const PReplyOut& O) {
  /* WMAX = 64 for every window: with arrays that small the compiler keeps the 8- and 16-entry
   * variants in VGPRs and spills (150 spilled registers, 1.07 ms for the 1 M-group burst against 0.6 ms) */
  LAUNCH_B(e, "k_bucket_prepare_reply", (k_bucket_prepare_reply<KMAX, 64>), e->S, e->X, I, O);
}

}  // namespace

extern "C" {

int gpx_election_begin_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* bnum,
                           uint8_t* e_status) {
  if (!h || n < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (!gidx || !bnum || !e_status) return GPX_EINVAL;
  int rc = elect_init(h);
  if (rc != GPX_OK) return rc;
  h->stream = h->sB;
  LAUNCH(h, "k_election_begin", k_election_begin, grid_for(n), h->S, n, gidx, bnum, e_status);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

int gpx_prepare_reply_batch_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* acceptor,
                                const int32_t* r_bnum, const int32_t* r_bcoord,
                                const int32_t* first_slot, const int32_t* pv_off, int32_t pv_total,
                                const int32_t* pv_slot, const int32_t* pv_bnum,
                                const int32_t* pv_bcoord, const int64_t* pv_handle,
                                const uint8_t* pv_flags, uint8_t* v_kind, int32_t* e_count,
                                int32_t* e_median, int32_t* e_slot, uint8_t* e_kind,
                                int64_t* e_handle, uint8_t* e_flags, uint8_t* status) {
  int rc = check_batch(h, n);
  if (rc != GPX_OK) return rc;
  if (n == 0) return GPX_OK;
  if (!gidx || !acceptor || !r_bnum || !r_bcoord || !first_slot || !pv_off || pv_total < 0 || !v_kind ||
      !e_count || !e_median || !e_slot || !e_kind || !e_handle || !e_flags || !status)
    return GPX_EINVAL;
  if (pv_total && (!pv_slot || !pv_bnum || !pv_bcoord)) return GPX_EINVAL;
  if ((rc = elect_init(h)) != GPX_OK) return rc;
  gpx_engine* e = h;
  const size_t nn = (size_t)n, b4 = nn * 4;
  const int fs = begin_front(e);
  front_hist(e, n, gidx, status, 0);
  /* payload a = acceptor, b = firstSlot, ballot = the reply's ballot */
  launch_scatter_ac(e, n, gidx, r_bnum, r_bcoord, acceptor, first_slot, nullptr, nullptr, nullptr, nullptr,
                    nullptr);
  /* records of groups out of range never reach a bucket: their dense outputs are defined here */
  HIPCHK(hipMemsetAsync(v_kind, 0, nn, e->stream));
  HIPCHK(hipMemsetAsync(e_count, 0, b4, e->stream));
  HIPCHK(hipMemsetAsync(e_median, 0, b4, e->stream));
  begin_back(e, fs, n);
  PReplyIn I{pv_off, pv_total, pv_slot, pv_bnum, pv_bcoord, pv_handle, pv_flags};
  PReplyOut O{n, v_kind, e_count, e_median, e_slot, e_kind, e_handle, e_flags, status};
  if (e->cfg.kmax <= 4)
    launch_bucket_prepare_reply<4>(e, I, O);
  else if (e->cfg.kmax <= 8)
    launch_bucket_prepare_reply<8>(e, I, O);
  else
    launch_bucket_prepare_reply<16>(e, I, O);
  end_call(e, fs);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

int gpx_propose_batch_h_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const uint8_t* is_stop,
                            const int64_t* handle, int32_t* slot, int32_t* bnum, int32_t* bcoord,
                            int32_t* median_cp, uint8_t* status) {
  return propose_dev_impl(h, n, gidx, is_stop, handle, slot, bnum, bcoord, median_cp, status);
}

} /* extern "C" */
