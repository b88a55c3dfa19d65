// Device-pointer side of the group images (include/gpx_image.h; kernels in gpx_image.hip.h): the argument checks, the
// scratch, gpx_image_stride and the two *_dev calls; the host-pointer twins: gpx_image_host.inc.
// Needs: the engine and the kernels of gpx_engine.hip, gpx_ctl_block.inc, elect_init (gpx_elect_dev.inc).

namespace {

static_assert(sizeof(gpx_image_counts) == 16 && sizeof(ImageCounts) == 16, "gpx_image_counts is 16 bytes");
static_assert(GPX_IMAGE_TILE == GPX_BLOCK && GPX_IMAGE_TILE == GPX_IMAGE_TILE_ENTRIES,
              "one lane per entry of a tile; the header names the tile the kernels use");
static_assert(GPX_IMAGE_HEADER_WORDS <= GPX_IMAGE_CW && GPX_IMAGE_CW % 16 == 0 && GPX_IMAGE_LS >= GPX_IMAGE_CW && GPX_IMAGE_LS % 4 == 0,
              "the header lies in the first chunk; chunks are whole 64-byte segments; staged rows stay 16-byte aligned");
static_assert(GPX_IMG_P_PRESENT == PR_PRESENT && GPX_IMG_P_STOP == PR_STOP && GPX_IMG_R_PRESENT == RF_PRESENT &&
                  GPX_IMG_R_STOP == RF_STOP && GPX_IMG_R_HASVALUE == RF_HASVALUE && GPX_IMG_CO_PRESENT == CO_PRESENT,
              "the ring words of an image are the engine's");

/* what the calls check before they use the handle */
int image_export_args(const gpx_engine* h, int32_t n, int32_t flags, int32_t cap, const void* o_rows, const void* counts,
                      bool dev) {
  if (!h || n < 0 || cap < 0 || !counts || (flags & ~GPX_IMG_EVICT)) return GPX_EINVAL;
  if (cap > 0 && !o_rows) return GPX_EINVAL;
  if (dev && ((uintptr_t)o_rows & 15)) return GPX_EINVAL;
  return GPX_OK;
}
int image_import_args(const gpx_engine* h, int32_t n_rows, const void* rows, int32_t flags, const void* status, bool dev) {
  if (!h || n_rows < 0 || !status || (flags & ~GPX_IMG_VIEWCHANGE)) return GPX_EINVAL;
  if (n_rows > 0 && !rows) return GPX_EINVAL;
  if (dev && ((uintptr_t)rows & 15)) return GPX_EINVAL;
  return GPX_OK;
}

inline size_t image_stride_bytes(const gpx_engine* e) { return (size_t)image_stride_words(e->cfg.kmax, e->cfg.window) * 4; }

/* The export's parked entries and per-tile words, the import's row words and the host twins' counts: ONE block
 * (ctl_block), allocated by the first call of either kind.  Not cleared. */
int image_init(gpx_engine* e) {
  if (e->img_counts) return GPX_OK;
  const size_t tiles = ctl_tiles(e, GPX_IMAGE_TILE), cap = tiles * GPX_IMAGE_TILE;
  ImageMem& M = e->img;
  return ctl_block(e,
                   {ctl_col(&M.park, cap), ctl_col(&M.tile_live, tiles), ctl_col(&M.tile_rows, tiles),
                    ctl_col(&M.tile_off, tiles), ctl_col(&M.tile_goff, tiles), ctl_col(&M.desc, 2 * cap),
                    ctl_col(&M.src, 2 * cap), ctl_col(&e->img_counts, 1)},
                   false);
}

/* what a call needs of the engine: at most `limit` entries or rows, then ctl_open's checks and the scratch */
int image_open(gpx_engine* h, int64_t n, int64_t limit) { return ctl_open(h, n, limit, image_init); }

inline ImageIdle image_idle(const gpx_engine* h) { return ImageIdle{h->sweep.sig, h->sweep.age}; }
inline NameCopies image_names(const gpx_engine* h) { return NameCopies{h->N.rows, (uint8_t*)h->N.tab}; }

/* the three launches of an export over entries g_base .. g_base + n - 1 (gidx == null) or gidx[0 .. n) */
int image_export_run(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t g_base, int32_t flags, int32_t cap,
                     void* o_rows, gpx_image_counts* counts) {
  h->stream = h->sB;
  const int ntiles = tiles_for(n, GPX_IMAGE_TILE);
  if (ntiles) LAUNCH(h, "k_image_tile", k_image_tile, ntiles, h->S, n, gidx, g_base, h->img);
  LAUNCH(h, "k_image_offsets", k_image_offsets, 1, (int32_t)ntiles, h->img, cap, (ImageCounts*)counts);
  if (ntiles && cap > 0)
    LAUNCH(h, "k_image_move", k_image_move, ntiles, h->S, h->img, image_names(h), image_idle(h), cap, flags, (int32_t*)o_rows);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

/* the two launches of an import (the election arrays: the caller's business) */
int image_import_run(gpx_engine* h, int32_t n_rows, const void* rows, const int32_t* gidx, uint8_t* status) {
  h->stream = h->sB;
  const int ntiles = tiles_for(n_rows, GPX_IMAGE_TILE);
  if (!ntiles) return GPX_OK;
  LAUNCH(h, "k_image_check", k_image_rows<false>, ntiles, h->S, h->img, image_names(h), image_idle(h), n_rows,
         (const int32_t*)rows, gidx, status);
  LAUNCH(h, "k_image_apply", k_image_rows<true>, ntiles, h->S, h->img, image_names(h), image_idle(h), n_rows,
         (const int32_t*)rows, gidx, status);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

int image_import_open(gpx_engine* h, int32_t n_rows, int32_t flags) {
  int rc = image_open(h, n_rows, 2 * scan_max_n(h));
  if (rc != GPX_OK) return rc;
  return (flags & GPX_IMG_VIEWCHANGE) ? elect_init(h) : GPX_OK;
}

}  // namespace

extern "C" {

int64_t gpx_image_stride(int32_t kmax, int32_t window) {
  if (kmax < 1 || kmax > GPX_KMAX_LIMIT || window < 4 || window > 64 || (window & (window - 1))) return -1;
  return (int64_t)image_stride_words(kmax, window) * 4;
}

int gpx_group_export_dev(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t flags, int32_t cap, void* o_rows,
                         gpx_image_counts* counts) {
  int rc = image_export_args(h, n, flags, cap, o_rows, counts, true);
  if (rc != GPX_OK) return rc;
  if ((rc = image_open(h, n, scan_max_n(h))) != GPX_OK) return rc;
  return image_export_run(h, n, gidx, 0, flags, cap, o_rows, counts);
}

int gpx_group_import_dev(gpx_engine* h, int32_t n_rows, const void* rows, const int32_t* gidx, int32_t flags,
                         uint8_t* status) {
  int rc = image_import_args(h, n_rows, rows, flags, status, true);
  if (rc != GPX_OK) return rc;
  if ((rc = image_import_open(h, n_rows, flags)) != GPX_OK) return rc;
  return image_import_run(h, n_rows, rows, gidx, status);
}

} /* extern "C" */
