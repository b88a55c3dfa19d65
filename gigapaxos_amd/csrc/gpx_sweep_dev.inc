// Device-pointer side of the deactivation sweep (include/gpx_sweep.h; kernels in gpx_sweep.hip.h): the sweep's words,
// the engine-side checks and gpx_pause_sweep_dev; the host-pointer twin: gpx_sweep_host.inc.
// Needs: the engine and the kernels of gpx_engine.hip, scan_max_n (gpx_scan_dev.inc), gpx_ctl_args.inc.

namespace {

static_assert(GPX_SWEEP_PEEK == GPX_SWEEP_PEEK_ && GPX_SWEEP_HOLD == GPX_SWEEP_HOLD_,
              "include/gpx_sweep.h and gpx_sweep.hip.h disagree on the flags");
static_assert(GPX_SWEEP_TILE % GPX_BLOCK == 0, "a tile is whole passes of a workgroup");
static_assert(sizeof(gpx_sweep_counts) == 16 && sizeof(SweepCounts) == 16, "gpx_sweep_counts is 16 bytes");
static_assert(sizeof(gpx_hri) == 100, "the row of gpx_group_retire");

/* The idle words, the parked hits, the per-tile words and the host twin's counts: ONE block, allocated by the first
 * sweep.  Zeroed: the idle words start at "never seen" (the rest is scratch, of which a call reads only what it wrote).
 * A failed allocation leaves nothing behind and the engine usable. */
int sweep_init(gpx_engine* e) {
  if (e->sweep_counts) return GPX_OK;
  const size_t G = (size_t)std::max(e->cfg.max_groups, 1);
  const size_t tiles = std::max<size_t>(((size_t)scan_max_n(e) + GPX_SWEEP_TILE - 1) / GPX_SWEEP_TILE, 1);
  const size_t cap = tiles * GPX_SWEEP_TILE;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t b_sig = up(G * 4), b_age = up(G), b_pg = up(cap * 4), b_pa = up(cap), b_tl = up(tiles * 4);
  char* base = nullptr;
  int rc = dev_alloc(e, &base, b_sig + b_age + b_pg + b_pa + 4 * b_tl + 256, true);
  if (rc != GPX_OK) return rc;
  SweepMem& M = e->sweep;
  char* p = base;
  M.sig = (uint32_t*)p, p += b_sig;
  M.age = (uint8_t*)p, p += b_age;
  M.park_g = (int32_t*)p, p += b_pg;
  M.park_age = (uint8_t*)p, p += b_pa;
  M.tile_hits = (int32_t*)p, p += b_tl;
  M.tile_nog = (int32_t*)p, p += b_tl;
  M.tile_busy = (int32_t*)p, p += b_tl;
  M.tile_off = (int32_t*)p, p += b_tl;
  e->sweep_counts = (SweepCounts*)p; /* last: the marker */
  return GPX_OK;
}

/* what the sweep needs of the engine (its arguments: sweep_args, gpx_ctl_args.inc): the size limit, an engine an
 * exchange kernel gave up on, the sweep's words */
int sweep_open(gpx_engine* h, int32_t n) {
  if ((int64_t)n > scan_max_n(h)) return GPX_ECAPACITY;
  int rc = check_batch(h, 0);
  if (rc != GPX_OK) return rc;
  return sweep_init(h);
}

}  // namespace

extern "C" {

int gpx_pause_sweep_dev(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t min_age, int32_t flags, int32_t cap,
                        int32_t* o_gidx, uint8_t* o_age, gpx_hri* o_rows, gpx_sweep_counts* counts) {
  int rc = sweep_args(h, n, min_age, flags, cap, o_gidx, o_age, o_rows, counts);
  if (rc != GPX_OK) return rc;
  if ((rc = sweep_open(h, n)) != GPX_OK) return rc;
  h->stream = h->sB;
  const int ntiles = (int)(((int64_t)n + GPX_SWEEP_TILE - 1) / GPX_SWEEP_TILE);
  if (ntiles) LAUNCH(h, "k_sweep_tile", k_sweep_tile, ntiles, h->S, n, gidx, min_age, flags, h->sweep);
  LAUNCH(h, "k_sweep_offsets", k_sweep_offsets, 1, (int32_t)ntiles, h->sweep, cap, flags, (SweepCounts*)counts);
  if (ntiles && cap > 0)
    LAUNCH(h, "k_sweep_move", k_sweep_move, ntiles, h->S, h->sweep, NameCopies{h->N.rows, (uint8_t*)h->N.tab}, cap, flags,
           o_gidx, o_age, o_rows);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

} /* extern "C" */
