// Device-pointer side of the checkpoint transfer (include/gpx_checkpoint.h; kernels in gpx_checkpoint.hip.h): the
// scratch, the checks and gpx_checkpoint_batch_dev; the host-pointer twin: gpx_checkpoint_host.inc.
// Needs: the engine and the kernels of gpx_engine.hip, scan_init (gpx_scan_dev.inc), gpx_ctl_block.inc.

namespace {

static_assert(GPX_CP_PEEK == GPX_CP_PEEK_ && GPX_CP_ADOPT == GPX_CP_ADOPT_ && GPX_CP_MOVED == GPX_CP_MOVED_,
              "include/gpx_checkpoint.h and gpx_checkpoint.hip.h disagree on the flags");
static_assert(GPX_CP_TILE == GPX_BLOCK, "one lane per record of a tile");
static_assert(sizeof(gpx_cp_counts) == 16 && sizeof(CpCounts) == 16, "gpx_cp_counts is 16 bytes");

/* what the call checks before it uses the handle */
int cp_args(const gpx_engine* h, int32_t n, const void* gidx, const void* cp_slot, int32_t flags, const void* o_from,
            const void* o_to, const void* o_flags, const void* status, const void* x_gidx, const void* x_first,
            const void* x_count, const void* counts) {
  if (!h || n < 0 || (flags & ~GPX_CP_PEEK) || !counts) return GPX_EINVAL;
  if (!gidx || !cp_slot || !o_from || !o_to || !o_flags || !status) return GPX_EINVAL;
  if (!(flags & GPX_CP_PEEK) && (!x_gidx || !x_first || !x_count)) return GPX_EINVAL;
  return GPX_OK;
}

/* The parked runs (12 bytes per record of max(max_groups, max_batch) in whole tiles), the per-tile words (16 bytes) and
 * the host twin's counts.  They lie in the scan family's block where that is large enough, else in a block of their
 * own, allocated by the first call (ctl_block).  Not cleared. */
int cp_init(gpx_engine* e) {
  if (e->cp_counts) return GPX_OK;
  const size_t tiles = ctl_tiles(e, GPX_CP_TILE), cap = tiles * GPX_CP_TILE;
  int rc = scan_init(e);
  if (rc != GPX_OK) return rc;
  CpMem& M = e->cp;
  return ctl_block(e,
                   {ctl_col(&M.park_g, cap), ctl_col(&M.park_first, cap), ctl_col(&M.park_count, cap),
                    ctl_col(&M.tile, tiles), ctl_col(&e->cp_counts, 1)},
                   false, e->scan.base, (size_t)26 * e->scan.cap + (size_t)3 * e->scan.tl);
}

/* ctl_open for this family, under the name its host-pointer twin calls */
int cp_open(gpx_engine* h, int32_t n) { return ctl_open(h, n, scan_max_n(h), cp_init); }

}  // namespace

extern "C" {

int gpx_checkpoint_batch_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* cp_slot, int32_t flags,
                             int32_t* o_from, int32_t* o_to, uint8_t* o_flags, uint8_t* status, int32_t* x_gidx,
                             int32_t* x_first, int32_t* x_count, gpx_cp_counts* counts) {
  int rc = cp_args(h, n, gidx, cp_slot, flags, o_from, o_to, o_flags, status, x_gidx, x_first, x_count, counts);
  if (rc != GPX_OK) return rc;
  if ((rc = cp_open(h, n)) != GPX_OK) return rc;
  h->stream = h->sB;
  const bool peek = (flags & GPX_CP_PEEK) != 0;
  const int ntiles = tiles_for(n, GPX_CP_TILE);
  if (ntiles && peek)
    LAUNCH(h, "k_cp_tile_peek", (k_cp_tile<true>), ntiles, h->S, n, gidx, cp_slot, o_from, o_to, o_flags, status, h->cp);
  if (ntiles && !peek)
    LAUNCH(h, "k_cp_tile", (k_cp_tile<false>), ntiles, h->S, n, gidx, cp_slot, o_from, o_to, o_flags, status, h->cp);
  LAUNCH(h, "k_cp_offsets", k_cp_offsets, 1, (int32_t)ntiles, h->cp, (CpCounts*)counts);
  if (ntiles && !peek) LAUNCH(h, "k_cp_move", k_cp_move, ntiles, h->cp, x_gidx, x_first, x_count);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

} /* extern "C" */
