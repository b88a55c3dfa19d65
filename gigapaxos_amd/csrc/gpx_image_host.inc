// Host-pointer side of the group images (include/gpx_image.h), staged through CtlStage around the *_dev forms.
// Needs: gpx_host_stage.inc (CtlStage), gpx_image_dev.inc.

namespace {

/* The rows of a host-pointer call pass through ONE engine-owned device block of at most img_stage_max bytes (64 MiB;
 * GPX_TEST_IMAGE_STAGE at creation: tests), allocated on first use and grown to the largest demand seen.  Nothing is in
 * flight on it between calls: the twins are synchronous. */
int image_stage(gpx_engine* e, size_t bytes) {
  if (bytes <= e->img_stage_cap) return GPX_OK;
  if (e->img_stage) HIPQ(hipFree(e->img_stage));
  e->img_stage = nullptr;
  e->img_stage_cap = 0;
  void* q = nullptr;
  const hipError_t err = hipMalloc(&q, bytes);
  if (err != hipSuccess) {
    (void)hipGetLastError();
    snprintf(g_err, sizeof(g_err), "hipMalloc(%zu) -> %s", bytes, hipGetErrorString(err));
    return GPX_ENOMEM;
  }
  e->img_stage = (char*)q;
  e->img_stage_cap = bytes;
  return GPX_OK;
}
inline size_t image_stage_bound(const gpx_engine* e) { return std::max(e->img_stage_max, 2 * image_stride_bytes(e)); }

}  // namespace

extern "C" {

int gpx_group_export(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t flags, int32_t cap, void* o_rows,
                     gpx_image_counts* counts) {
  int rc = image_export_args(h, n, flags, cap, o_rows, counts, false);
  if (rc != GPX_OK) return rc;
  if ((rc = image_open(h, n, scan_max_n(h))) != GPX_OK) return rc;
  const size_t stride = image_stride_bytes(h);
  /* entries per chunk: every one of them may need two rows */
  const int64_t per = std::max<int64_t>(1, (int64_t)(image_stage_bound(h) / (2 * stride)));
  gpx_image_counts tot = {0, 0, 0, 0};
  bool cut = false; /* a group did not fit: nothing after it is written, the later chunks only count */
  int64_t i0 = 0;
  do {
    const int32_t m = (int32_t)std::min<int64_t>(per, (int64_t)n - i0);
    const int32_t capc = cut ? 0 : (int32_t)std::min<int64_t>((int64_t)cap - tot.n_rows_done, 2 * (int64_t)m);
    if (capc > 0 && (rc = image_stage(h, (size_t)capc * stride)) != GPX_OK) return rc;
    CtlStage t(h);
    const int32_t* d_g = (gidx && m) ? t.in(gidx + i0, (size_t)m) : nullptr;
    if (t.ready()) return t.rc;
    if (t.ran(image_export_run(h, m, d_g, (int32_t)i0, flags, capc, capc > 0 ? h->img_stage : nullptr,
                               (gpx_image_counts*)h->img_counts)))
      return t.rc;
    gpx_image_counts c;
    t.d2h(&c, h->img_counts, sizeof(c));
    if (t.sync()) return t.rc;
    if (c.n_rows_done > 0) {
      t.d2h((char*)o_rows + (size_t)tot.n_rows_done * stride, h->img_stage, (size_t)c.n_rows_done * stride);
      if (t.sync()) return t.rc;
    }
    tot.n_live += c.n_live;
    tot.n_rows += c.n_rows;
    tot.n_done += c.n_done;
    tot.n_rows_done += c.n_rows_done;
    cut = cut || c.n_done < c.n_live;
    i0 += m;
  } while (i0 < n);
  *counts = tot;
  return GPX_OK;
}

int gpx_group_import(gpx_engine* h, int32_t n_rows, const void* rows, const int32_t* gidx, int32_t flags,
                     uint8_t* status) {
  int rc = image_import_args(h, n_rows, rows, flags, status, false);
  if (rc != GPX_OK) return rc;
  if ((rc = image_import_open(h, n_rows, flags)) != GPX_OK) return rc;
  const size_t stride = image_stride_bytes(h);
  const int64_t per = std::max<int64_t>(2, (int64_t)(image_stage_bound(h) / stride));
  auto kind_of = [&](int64_t r) { return ((const int32_t*)((const char*)rows + (size_t)r * stride))[1]; };
  for (int64_t r0 = 0; r0 < n_rows;) {
    int64_t m = std::min<int64_t>(per, (int64_t)n_rows - r0);
    /* a main row and the continuation row behind it stay in one chunk (m >= 2 here: per >= 2) */
    if (r0 + m < n_rows && kind_of(r0 + m) == GPX_IMAGE_CONT && kind_of(r0 + m - 1) == GPX_IMAGE_MAIN && m > 1) m--;
    if ((rc = image_stage(h, (size_t)m * stride)) != GPX_OK) return rc;
    CtlStage t(h);
    const int32_t* d_g = gidx ? t.in(gidx + r0, (size_t)m) : nullptr;
    uint8_t* d_st = t.out(status + r0, (size_t)m);
    t.h2d(h->img_stage, (const char*)rows + (size_t)r0 * stride, (size_t)m * stride);
    if (t.ready()) return t.rc;
    if (t.ran(image_import_run(h, (int32_t)m, h->img_stage, d_g, d_st))) return t.rc;
    if ((rc = t.fetch({d_st})) != GPX_OK) return rc;
    r0 += m;
  }
  return GPX_OK;
}

} /* extern "C" */
