// Device-pointer side of the deactivation sweep (include/gpx_sweep.h; kernels in gpx_sweep.hip.h): the sweep's words,
// the engine-side checks and gpx_pause_sweep_dev; the host-pointer twin: gpx_sweep_host.inc.
// Needs: the engine and the kernels of gpx_engine.hip, gpx_ctl_args.inc, gpx_ctl_block.inc.

namespace {

static_assert(GPX_SWEEP_PEEK == GPX_SWEEP_PEEK_ && GPX_SWEEP_HOLD == GPX_SWEEP_HOLD_,
              "include/gpx_sweep.h and gpx_sweep.hip.h disagree on the flags");
static_assert(GPX_SWEEP_TILE % GPX_BLOCK == 0, "a tile is whole passes of a workgroup");
static_assert(sizeof(gpx_sweep_counts) == 16 && sizeof(SweepCounts) == 16, "gpx_sweep_counts is 16 bytes");
static_assert(sizeof(gpx_hri) == 100, "the row of gpx_group_retire");

/* The idle words, the parked hits, the per-tile words and the host twin's counts: ONE block (ctl_block), allocated by the
 * first sweep.  Zeroed: the idle words start at "never seen". */
int sweep_init(gpx_engine* e) {
  if (e->sweep_counts) return GPX_OK;
  const size_t G = (size_t)std::max(e->cfg.max_groups, 1);
  const size_t tiles = ctl_tiles(e, GPX_SWEEP_TILE), cap = tiles * GPX_SWEEP_TILE;
  SweepMem& M = e->sweep;
  return ctl_block(e,
                   {ctl_col(&M.sig, G), ctl_col(&M.age, G), ctl_col(&M.park_g, cap), ctl_col(&M.park_age, cap),
                    ctl_col(&M.tile_hits, tiles), ctl_col(&M.tile_nog, tiles), ctl_col(&M.tile_busy, tiles),
                    ctl_col(&M.tile_off, tiles), ctl_col(&e->sweep_counts, 1)},
                   true);
}

/* ctl_open for this family, under the name its host-pointer twin calls */
int sweep_open(gpx_engine* h, int32_t n) { return ctl_open(h, n, scan_max_n(h), sweep_init); }

}  // namespace

extern "C" {

int gpx_pause_sweep_dev(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t min_age, int32_t flags, int32_t cap,
                        int32_t* o_gidx, uint8_t* o_age, gpx_hri* o_rows, gpx_sweep_counts* counts) {
  int rc = sweep_args(h, n, min_age, flags, cap, o_gidx, o_age, o_rows, counts);
  if (rc != GPX_OK) return rc;
  if ((rc = sweep_open(h, n)) != GPX_OK) return rc;
  h->stream = h->sB;
  const int ntiles = tiles_for(n, GPX_SWEEP_TILE);
  if (ntiles) LAUNCH(h, "k_sweep_tile", k_sweep_tile, ntiles, h->S, n, gidx, min_age, flags, h->sweep);
  LAUNCH(h, "k_sweep_offsets", k_sweep_offsets, 1, (int32_t)ntiles, h->sweep, cap, flags, (SweepCounts*)counts);
  if (ntiles && cap > 0)
    LAUNCH(h, "k_sweep_move", k_sweep_move, ntiles, h->S, h->sweep, NameCopies{h->N.rows, (uint8_t*)h->N.tab}, cap, flags,
           o_gidx, o_age, o_rows);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

} /* extern "C" */
