// Device-pointer side of the view change in list form (include/gpx_viewchange.h; kernels in gpx_vclists.hip.h): the two
// scratch blocks, the checks and the *_dev calls; the host-pointer twins: gpx_vclists_host.inc.
// Needs: the engine and the kernels of gpx_engine.hip, gpx_prepare_reply_batch_dev (gpx_elect_dev.inc), gpx_ctl_block.inc.

namespace {

static_assert(GPX_VCL_TILE == GPX_VCL_TILE_, "include/gpx_viewchange.h and gpx_vclists.hip.h disagree on the tile");
static_assert(sizeof(gpx_pl_counts) == 32 && sizeof(PlCounts) == 32, "gpx_pl_counts is 32 bytes");
static_assert(sizeof(gpx_prl_counts) == 32 && sizeof(PrlCounts) == 32, "gpx_prl_counts is 32 bytes");

inline size_t vcl_tiles(const gpx_engine* e) { return (size_t)std::max(tiles_for(e->cfg.max_batch, GPX_VCL_TILE), 1); }

/* Acceptor side: the masks (8 bytes per record of max_batch), the per-tile words, the cut and the host twin's counts:
 * ONE block, allocated by the first gpx_prepare_lists*.  Not cleared.  A block of its own: a node is acceptor and
 * coordinator in one burst, and an acceptor call must not clobber the coordinator's parked lists. */
int pl_init(gpx_engine* e) {
  if (e->pl_counts) return GPX_OK;
  const size_t tiles = vcl_tiles(e), cap = tiles * GPX_VCL_TILE;
  PlMem M{};
  PlCounts* counts = nullptr;
  int rc = ctl_block(e, {ctl_col(&M.mask, cap), ctl_col(&M.t_ent, tiles), ctl_col(&M.t_drop, tiles), ctl_col(&M.t_nack, tiles),
                         ctl_col(&M.t_tolog, tiles), ctl_col(&M.t_off, tiles), ctl_col(&M.cut, 2), ctl_col(&counts, 1)},
                     false);
  if (rc != GPX_OK) return rc;
  e->pl = M;
  e->pl_counts = counts;
  return GPX_OK;
}

/* Coordinator side: the dense call's outputs ((10 + 14 * window) bytes per record of max_batch), the parked hits
 * (16 bytes per record), the per-tile words, the move pass's span and the host twins' counts: ONE block, allocated by
 * the first gpx_prepare_reply_lists*.  Not cleared. */
int prl_init(gpx_engine* e) {
  if (e->prl_counts) return GPX_OK;
  const size_t tiles = vcl_tiles(e), cap = tiles * GPX_VCL_TILE, W = (size_t)e->cfg.window;
  if (cap * W > (size_t)INT32_MAX) return GPX_ECAPACITY; /* entry offsets are int32 */
  PrlMem M{};
  PrlCounts* counts = nullptr;
  int rc = ctl_block(e, {ctl_col(&M.e_handle, cap * W), ctl_col(&M.e_slot, cap * W), ctl_col(&M.e_kind, cap * W),
                         ctl_col(&M.e_flags, cap * W), ctl_col(&M.e_count, cap), ctl_col(&M.e_median, cap),
                         ctl_col(&M.v_kind, cap), ctl_col(&M.status, cap), ctl_col(&M.p_rec, cap), ctl_col(&M.p_gidx, cap),
                         ctl_col(&M.p_pre, cap), ctl_col(&M.p_cnt, cap), ctl_col(&M.t_hits, tiles), ctl_col(&M.t_ent, tiles),
                         ctl_col(&M.t_el, tiles), ctl_col(&M.t_pre, tiles), ctl_col(&M.t_drop, tiles),
                         ctl_col(&M.t_hoff, tiles), ctl_col(&M.t_eoff, tiles), ctl_col(&M.ctl, 4), ctl_col(&counts, 1)},
                     false);
  if (rc != GPX_OK) return rc;
  e->prl = M;
  e->prl_counts = counts;
  if (const char* sv = getenv("GPX_TEST_VCL_STAGE")) e->vcl_stage_hits = (size_t)std::max(1, atoi(sv)); /* tests: rounds */
  return GPX_OK;
}

/* what the calls check before they use the handle */
int pl_args(const gpx_engine* h, int32_t n, const void* gidx, const void* bnum, const void* bcoord, const void* first_slot,
            const void* r_bnum, const void* r_bcoord, const void* r_gc, const void* r_flags, const void* status,
            int32_t cap_entries, const void* pv_off, const void* pv_slot, const void* pv_bnum, const void* pv_bcoord,
            const void* counts) {
  if (!h || !counts || n < 0 || cap_entries < 0) return GPX_EINVAL;
  if (cap_entries > 0 && (!pv_off || !pv_slot || !pv_bnum || !pv_bcoord)) return GPX_EINVAL;
  if (n > 0 && (!gidx || !bnum || !bcoord || !first_slot || !r_bnum || !r_bcoord || !r_gc || !r_flags || !status))
    return GPX_EINVAL;
  return GPX_OK;
}
int prl_out_args(const gpx_engine* h, int32_t from_hit, int32_t cap_hits, int32_t cap_entries, const PrlOut& O,
                 const void* counts) {
  if (!h || !counts || from_hit < 0 || cap_hits < 0 || cap_entries < 0) return GPX_EINVAL;
  if (cap_hits > 0 && (!O.h_rec || !O.h_gidx || !O.h_kind || !O.h_status || !O.h_median || !O.h_off || !O.h_count))
    return GPX_EINVAL;
  if (cap_entries > 0 && (!O.e_slot || !O.e_kind || !O.e_handle || !O.e_flags)) return GPX_EINVAL;
  return GPX_OK;
}
int prl_in_args(int32_t n, const void* gidx, const void* acceptor, const void* r_bnum, const void* r_bcoord,
                const void* first_slot, const void* pv_off, int32_t pv_total, const void* pv_slot, const void* pv_bnum,
                const void* pv_bcoord) {
  if (n < 0 || pv_total < 0) return GPX_EINVAL;
  if (n > 0 && (!gidx || !acceptor || !r_bnum || !r_bcoord || !first_slot || !pv_off)) return GPX_EINVAL;
  if (n > 0 && pv_total && (!pv_slot || !pv_bnum || !pv_bcoord)) return GPX_EINVAL;
  return GPX_OK;
}

int pl_open(gpx_engine* h, int32_t n) { return ctl_open(h, n, h->cfg.max_batch, pl_init); }
int prl_open(gpx_engine* h, int32_t n) { return ctl_open(h, n, h->cfg.max_batch, prl_init); }

/* offsets + move over what the last apply parked: everything a continuation runs.  `bias` is added to h_off (the host
 * twin's rounds: relative to the caller's arrays). */
int prl_more(gpx_engine* h, int32_t from_hit, int32_t cap_hits, int32_t cap_entries, int32_t bias, const PrlOut& O,
             gpx_prl_counts* counts) {
  h->stream = h->sB;
  const int ntiles = tiles_for(h->prl_n, GPX_VCL_TILE);
  LAUNCH(h, "k_vl_offsets", k_vl_offsets, 1, (int32_t)ntiles, from_hit, cap_hits, cap_entries, h->prl, (PrlCounts*)counts);
  if (ntiles && cap_hits > 0) LAUNCH(h, "k_vl_move", k_vl_move, ntiles, h->prl_n, bias, h->prl, O);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

/* the dense call into the engine's scratch, then the tile pass: what gpx_prepare_reply_lists* adds in front of _more(0) */
int prl_apply(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* acceptor, const int32_t* r_bnum,
              const int32_t* r_bcoord, const int32_t* first_slot, const int32_t* pv_off, int32_t pv_total,
              const int32_t* pv_slot, const int32_t* pv_bnum, const int32_t* pv_bcoord, const int64_t* pv_handle,
              const uint8_t* pv_flags, uint8_t* v_kind, uint8_t* status) {
  const PrlMem& M = h->prl;
  h->prl_n = -1; /* whatever was parked is about to be overwritten */
  if (n > 0) {
    int rc = gpx_prepare_reply_batch_dev(h, n, gidx, acceptor, r_bnum, r_bcoord, first_slot, pv_off, pv_total, pv_slot,
                                         pv_bnum, pv_bcoord, pv_handle, pv_flags, M.v_kind, M.e_count, M.e_median, M.e_slot,
                                         M.e_kind, M.e_handle, M.e_flags, M.status);
    if (rc != GPX_OK) return rc;
    h->stream = h->sB;
    if (v_kind) HIPCHK(hipMemcpyAsync(v_kind, M.v_kind, (size_t)n, hipMemcpyDeviceToDevice, h->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, M.status, (size_t)n, hipMemcpyDeviceToDevice, h->stream));
    LAUNCH(h, "k_vl_tile", k_vl_tile, tiles_for(n, GPX_VCL_TILE), n, (int32_t)h->cfg.window, gidx, M);
    HIPCHK(hipGetLastError());
  }
  h->prl_n = n;
  return GPX_OK;
}

}  // namespace

extern "C" {

int gpx_prepare_lists_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* bnum, const int32_t* bcoord,
                          const int32_t* first_slot, int32_t* r_bnum, int32_t* r_bcoord, int32_t* r_gc,
                          uint8_t* r_flags, uint8_t* status, int32_t cap_entries, int32_t* pv_off, int32_t* pv_slot,
                          int32_t* pv_bnum, int32_t* pv_bcoord, gpx_pl_counts* counts) {
  int rc = pl_args(h, n, gidx, bnum, bcoord, first_slot, r_bnum, r_bcoord, r_gc, r_flags, status, cap_entries, pv_off,
                   pv_slot, pv_bnum, pv_bcoord, counts);
  if (rc != GPX_OK) return rc;
  if ((rc = pl_open(h, n)) != GPX_OK) return rc;
  gpx_engine* e = h;
  const PlMem& M = e->pl;
  const int ntiles = tiles_for(n, GPX_VCL_TILE);
  if (n > 0) {
    /* gpx_prepare_batch_dev's front end and evaluation; the masks go to the scratch and no plane is written */
    const int fs = begin_front(e);
    front_hist(e, n, gidx, status, 0);
    launch_scatter_ac(e, n, gidx, bnum, bcoord, first_slot, first_slot, nullptr, r_bnum, r_bcoord, r_gc, r_flags);
    HIPCHK(hipMemsetAsync(M.mask, 0, (size_t)n * 8, e->stream));
    begin_back(e, fs, n);
    PrepOut O{n, r_bnum, r_bcoord, r_gc, r_flags, M.mask, nullptr, nullptr, nullptr, status};
    LAUNCH_B(e, "k_bucket_prepare_mask", k_bucket_prepare<false>, e->S, e->X, O);
    end_call(e, fs);
    e->stream = e->sB;
    LAUNCH(e, "k_pl_tile", k_pl_tile, ntiles, n, r_flags, status, M);
  }
  e->stream = e->sB;
  LAUNCH(e, "k_pl_offsets", k_pl_offsets, 1, n, (int32_t)ntiles, cap_entries, M, pv_off, (PlCounts*)counts);
  if (ntiles && pv_off) LAUNCH(e, "k_pl_move", k_pl_move, ntiles, e->S, n, gidx, M, pv_off, pv_slot, pv_bnum, pv_bcoord);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

int gpx_prepare_reply_lists_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* acceptor,
                                const int32_t* r_bnum, const int32_t* r_bcoord, const int32_t* first_slot,
                                const int32_t* pv_off, int32_t pv_total, const int32_t* pv_slot, const int32_t* pv_bnum,
                                const int32_t* pv_bcoord, const int64_t* pv_handle, const uint8_t* pv_flags,
                                uint8_t* v_kind, uint8_t* status, int32_t cap_hits, int32_t cap_entries, int32_t* h_rec,
                                int32_t* h_gidx, uint8_t* h_kind, uint8_t* h_status, int32_t* h_median, int32_t* h_off,
                                int32_t* h_count, int32_t* e_slot, uint8_t* e_kind, int64_t* e_handle, uint8_t* e_flags,
                                gpx_prl_counts* counts) {
  const PrlOut O{h_rec, h_gidx, h_kind, h_status, h_median, h_off, h_count, e_slot, e_kind, e_handle, e_flags};
  int rc = prl_out_args(h, 0, cap_hits, cap_entries, O, counts);
  if (rc != GPX_OK) return rc;
  if ((rc = prl_in_args(n, gidx, acceptor, r_bnum, r_bcoord, first_slot, pv_off, pv_total, pv_slot, pv_bnum, pv_bcoord)) !=
      GPX_OK)
    return rc;
  if ((rc = prl_open(h, n)) != GPX_OK) return rc;
  if ((rc = prl_apply(h, n, gidx, acceptor, r_bnum, r_bcoord, first_slot, pv_off, pv_total, pv_slot, pv_bnum, pv_bcoord,
                      pv_handle, pv_flags, v_kind, status)) != GPX_OK)
    return rc;
  return prl_more(h, 0, cap_hits, cap_entries, 0, O, counts);
}

int gpx_prepare_reply_lists_more_dev(gpx_engine* h, int32_t from_hit, int32_t cap_hits, int32_t cap_entries,
                                     int32_t* h_rec, int32_t* h_gidx, uint8_t* h_kind, uint8_t* h_status,
                                     int32_t* h_median, int32_t* h_off, int32_t* h_count, int32_t* e_slot,
                                     uint8_t* e_kind, int64_t* e_handle, uint8_t* e_flags, gpx_prl_counts* counts) {
  const PrlOut O{h_rec, h_gidx, h_kind, h_status, h_median, h_off, h_count, e_slot, e_kind, e_handle, e_flags};
  int rc = prl_out_args(h, from_hit, cap_hits, cap_entries, O, counts);
  if (rc != GPX_OK) return rc;
  if (h->prl_n < 0 || !h->prl_counts) return GPX_EINVAL; /* nothing parked */
  if ((rc = check_batch(h, 0)) != GPX_OK) return rc;
  return prl_more(h, from_hit, cap_hits, cap_entries, 0, O, counts);
}

} /* extern "C" */
