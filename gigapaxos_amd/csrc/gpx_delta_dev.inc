// Device-pointer side of the delta images (include/gpx_delta.h; kernels in gpx_delta.hip.h): the argument checks, the
// marks and the scratch, and the two *_dev calls; the host-pointer twins: gpx_delta_host.inc.
// Needs: gpx_image_dev.inc (image_open, image_import_open, image_names, image_idle), gpx_ctl_block.inc.

namespace {

static_assert(sizeof(gpx_delta_counts) == 32 && sizeof(DeltaCounts) == 32, "gpx_delta_counts is 32 bytes");
static_assert(GPX_DELTA_EVICT == GPX_DELTA_EVICT_ && GPX_DELTA_FULL == GPX_DELTA_FULL_ && GPX_DELTA_EVICT == GPX_IMG_EVICT,
              "include/gpx_delta.h and gpx_delta.hip.h disagree on the flags");

/* what the calls check before they use the handle */
int delta_export_args(const gpx_engine* h, int32_t n, int32_t flags, int32_t cap, const void* o_rows, int32_t cap_gone,
                      const void* o_gone, const void* counts, bool dev) {
  if (!h || n < 0 || cap < 0 || cap_gone < 0 || !counts || (flags & ~(GPX_DELTA_EVICT | GPX_DELTA_FULL))) return GPX_EINVAL;
  if ((cap > 0 && !o_rows) || (cap_gone > 0 && !o_gone)) return GPX_EINVAL;
  if (dev && (((uintptr_t)o_rows & 15) || ((uintptr_t)o_gone & 3))) return GPX_EINVAL;
  return GPX_OK;
}
int delta_apply_args(const gpx_engine* h, int32_t n_rows, const void* rows, int32_t flags, const void* status,
                     int32_t n_gone, const void* gone, const void* gone_status, bool dev) {
  if (!h || n_rows < 0 || n_gone < 0 || (flags & ~GPX_IMG_VIEWCHANGE)) return GPX_EINVAL;
  if ((n_rows > 0 && (!rows || !status)) || (n_gone > 0 && (!gone || !gone_status))) return GPX_EINVAL;
  if (dev && (((uintptr_t)rows & 15) || ((uintptr_t)gone & 3))) return GPX_EINVAL;
  return GPX_OK;
}

/* The marks over max_groups, the parked entries, the per-tile words and the host twins' counts: ONE block (ctl_block),
 * allocated by the first delta export.  Zeroed: a mark starts at "never written". */
int delta_init(gpx_engine* e) {
  if (e->delta_counts) return GPX_OK;
  const size_t G = (size_t)std::max(e->cfg.max_groups, 1);
  const size_t tiles = ctl_tiles(e, GPX_IMAGE_TILE), cap = tiles * GPX_IMAGE_TILE;
  DeltaMem& M = e->delta;
  return ctl_block(e,
                   {ctl_col(&M.marks, G), ctl_col(&M.park_sig, cap), ctl_col(&M.park, cap), ctl_col(&M.park_gone, cap),
                    ctl_col(&M.tile_live, tiles), ctl_col(&M.tile_chg, tiles), ctl_col(&M.tile_rows, tiles),
                    ctl_col(&M.tile_gone, tiles), ctl_col(&M.tile_off, tiles), ctl_col(&M.tile_goff, tiles),
                    ctl_col(&M.tile_xoff, tiles), ctl_col(&e->delta_counts, 1)},
                   true);
}

int delta_export_open(gpx_engine* h, int32_t n) {
  int rc = image_open(h, n, scan_max_n(h));
  if (rc != GPX_OK) return rc;
  return delta_init(h);
}

/* the three launches of a delta export over entries g_base .. g_base + n - 1 (gidx == null) or gidx[0 .. n) */
int delta_export_run(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t g_base, int32_t flags, int32_t cap,
                     void* o_rows, int32_t cap_gone, int32_t* o_gone, gpx_delta_counts* counts) {
  h->stream = h->sB;
  const int ntiles = tiles_for(n, GPX_IMAGE_TILE);
  if (ntiles) LAUNCH(h, "k_delta_tile", k_delta_tile, ntiles, h->S, n, gidx, g_base, flags, h->delta);
  LAUNCH(h, "k_delta_offsets", k_delta_offsets, 1, (int32_t)ntiles, h->delta, cap, cap_gone, (DeltaCounts*)counts);
  if (ntiles && (cap > 0 || cap_gone > 0))
    LAUNCH(h, "k_delta_move", k_delta_move, ntiles, h->S, h->delta, image_names(h), image_idle(h), cap, cap_gone, flags,
           (int32_t*)o_rows, o_gone);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

/* the import's two launches with the replace rule */
int delta_rows_run(gpx_engine* h, int32_t n_rows, const void* rows, const int32_t* gidx, uint8_t* status) {
  h->stream = h->sB;
  const int ntiles = tiles_for(n_rows, GPX_IMAGE_TILE);
  if (!ntiles) return GPX_OK;
  LAUNCH(h, "k_delta_check", k_delta_rows<false>, ntiles, h->S, h->img, image_names(h), image_idle(h), n_rows,
         (const int32_t*)rows, gidx, status);
  LAUNCH(h, "k_delta_apply", k_delta_rows<true>, ntiles, h->S, h->img, image_names(h), image_idle(h), n_rows,
         (const int32_t*)rows, gidx, status);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

/* ... and the retire pass over the groups the source no longer has */
int delta_gone_run(gpx_engine* h, int32_t n_gone, const int32_t* gone, uint8_t* gone_status) {
  h->stream = h->sB;
  if (!n_gone) return GPX_OK;
  LAUNCH(h, "k_delta_gone", k_delta_gone, (n_gone + GPX_BLOCK - 1) / GPX_BLOCK, h->S, image_names(h), image_idle(h), n_gone,
         gone, gone_status);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

int delta_apply_open(gpx_engine* h, int32_t n_rows, int32_t n_gone, int32_t flags) {
  if ((int64_t)n_gone > scan_max_n(h)) return GPX_ECAPACITY;
  return image_import_open(h, n_rows, flags);
}

}  // namespace

extern "C" {

int gpx_group_export_delta_dev(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t flags, int32_t cap, void* o_rows,
                               int32_t cap_gone, int32_t* o_gone, gpx_delta_counts* counts) {
  int rc = delta_export_args(h, n, flags, cap, o_rows, cap_gone, o_gone, counts, true);
  if (rc != GPX_OK) return rc;
  if ((rc = delta_export_open(h, n)) != GPX_OK) return rc;
  return delta_export_run(h, n, gidx, 0, flags, cap, o_rows, cap_gone, o_gone, counts);
}

int gpx_group_apply_delta_dev(gpx_engine* h, int32_t n_rows, const void* rows, const int32_t* gidx, int32_t flags,
                              uint8_t* status, int32_t n_gone, const int32_t* gone, uint8_t* gone_status) {
  int rc = delta_apply_args(h, n_rows, rows, flags, status, n_gone, gone, gone_status, true);
  if (rc != GPX_OK) return rc;
  if ((rc = delta_apply_open(h, n_rows, n_gone, flags)) != GPX_OK) return rc;
  if ((rc = delta_rows_run(h, n_rows, rows, gidx, status)) != GPX_OK) return rc;
  return delta_gone_run(h, n_gone, gone, gone_status);
}

} /* extern "C" */
