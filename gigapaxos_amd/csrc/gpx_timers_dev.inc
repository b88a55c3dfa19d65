// Device-pointer side of the retransmission sweep (include/gpx_timers.h; kernels in gpx_timers.hip.h): the timer words,
// the argument checks, the back-off table and gpx_retransmit_sweep_dev; the host-pointer twin: gpx_timers_host.inc.
// Needs: the engine and the kernels of gpx_engine.hip, gpx_ctl_block.inc.

namespace {

static_assert(GPX_RTX_PEEK == GPX_RTX_PEEK_ && GPX_RTX_MAX_STEPS == GPX_RTX_MAX_STEPS_,
              "include/gpx_timers.h and gpx_timers.hip.h disagree on the flag or the table size");
static_assert(GPX_RTX_TILE % GPX_BLOCK == 0, "a tile is whole passes of a workgroup");
static_assert(sizeof(gpx_rtx_counts) == 16 && sizeof(RtxCounts) == 16, "gpx_rtx_counts is 16 bytes");
static_assert(sizeof(gpx_rtx_cfg) == 260 && sizeof(RtxCfg) == 260, "gpx_rtx_cfg: the count and two tables of 32 words");

/* what the retransmission sweep checks before it uses the handle */
int rtx_args(const gpx_engine* h, int32_t n, const gpx_rtx_cfg* cfg, int32_t flags, int32_t cap,
             std::initializer_list<const void*> cols, const void* counts) {
  if (!h || !cfg || !counts || n < 0 || cap < 0 || (flags & ~GPX_RTX_PEEK)) return GPX_EINVAL;
  if (cfg->n_steps < 1 || cfg->n_steps > GPX_RTX_MAX_STEPS) return GPX_EINVAL;
  for (int32_t q = 0; q < cfg->n_steps; q++)
    if (cfg->accept_ms[q] < 0 || cfg->prepare_ms[q] < 0) return GPX_EINVAL;
  if (cap > 0)
    for (const void* c : cols)
      if (!c) return GPX_EINVAL;
  return GPX_OK;
}

/* The timer words, the parked hits, the per-tile words and the host twin's counts: ONE block (ctl_block), allocated by
 * the first sweep.  Zeroed: the timer words start at "waiting for nothing". */
int rtx_init(gpx_engine* e) {
  if (e->rtx_counts) return GPX_OK;
  const size_t G = (size_t)std::max(e->cfg.max_groups, 1);
  const size_t tiles = ctl_tiles(e, GPX_RTX_TILE), cap = tiles * GPX_RTX_TILE;
  RtxMem& M = e->rtx;
  return ctl_block(e,
                   {ctl_col(&M.key, G), ctl_col(&M.since, G), ctl_col(&M.count, G), ctl_col(&M.park_g, cap),
                    ctl_col(&M.park_wait, cap), ctl_col(&M.park_count, cap), ctl_col(&M.tile_hits, tiles),
                    ctl_col(&M.tile_nog, tiles), ctl_col(&M.tile_wait, tiles), ctl_col(&M.tile_off, tiles),
                    ctl_col(&e->rtx_counts, 1)},
                   true);
}

/* ctl_open for this family, under the name its host-pointer twin calls */
int rtx_open(gpx_engine* h, int32_t n) { return ctl_open(h, n, scan_max_n(h), rtx_init); }

/* the three launches (gpx_timers.hip.h) on the back-end stream */
template <int KMAX>
int rtx_run(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t now_ms, const RtxCfg& cfg, int32_t flags, int32_t cap,
            const RtxOut& O, gpx_rtx_counts* counts) {
  h->stream = h->sB;
  const int ntiles = tiles_for(n, GPX_RTX_TILE);
  if (ntiles) LAUNCH(h, "k_rtx_tile", k_rtx_tile<KMAX>, ntiles, h->S, n, gidx, now_ms, cfg, flags, h->rtx);
  LAUNCH(h, "k_rtx_offsets", k_rtx_offsets, 1, (int32_t)ntiles, h->rtx, cap, flags, (RtxCounts*)counts);
  if (ntiles && cap > 0) LAUNCH(h, "k_rtx_move", k_rtx_move<KMAX>, ntiles, h->S, h->rtx, now_ms, cap, flags, O);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

}  // namespace

extern "C" {

int gpx_rtx_backoff_table(int32_t timeout_ms, double factor, int32_t n_steps, int32_t* out) {
  if (!out || n_steps < 1 || n_steps > GPX_RTX_MAX_STEPS || timeout_ms < 0 || !(factor >= 1.0) || !std::isfinite(factor))
    return GPX_EINVAL;
  for (int32_t c = 0; c < n_steps; c++) {
    const double x = (double)timeout_ms * std::pow(factor, (double)c); /* TIMEOUT * Math.pow(FACTOR, count) */
    out[c] = x >= (double)INT32_MAX ? INT32_MAX : (int32_t)std::floor(x);
  }
  return GPX_OK;
}

int gpx_retransmit_sweep_dev(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t now_ms, const gpx_rtx_cfg* cfg,
                             int32_t flags, int32_t cap, int32_t* o_gidx, uint8_t* o_poke, int32_t* o_slot,
                             int32_t* o_bnum, int32_t* o_bcoord, int32_t* o_median_cp, uint8_t* o_flags,
                             uint32_t* o_heard, uint8_t* o_count, int32_t* o_waited, gpx_rtx_counts* counts) {
  int rc = rtx_args(h, n, cfg, flags, cap,
                    {o_gidx, o_poke, o_slot, o_bnum, o_bcoord, o_median_cp, o_flags, o_heard, o_count, o_waited}, counts);
  if (rc != GPX_OK) return rc;
  if ((rc = rtx_open(h, n)) != GPX_OK) return rc;
  RtxCfg c;
  memcpy(&c, cfg, sizeof(c));
  const RtxOut O{o_gidx, o_poke, o_slot, o_bnum, o_bcoord, o_median_cp, o_flags, o_heard, o_count, o_waited};
  if (h->cfg.kmax <= 4) return rtx_run<4>(h, n, gidx, now_ms, c, flags, cap, O, counts);
  if (h->cfg.kmax <= 8) return rtx_run<8>(h, n, gidx, now_ms, c, flags, cap, O, counts);
  return rtx_run<16>(h, n, gidx, now_ms, c, flags, cap, O, counts);
}

} /* extern "C" */
