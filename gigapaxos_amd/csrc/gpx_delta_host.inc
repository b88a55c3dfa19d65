// Host-pointer side of the delta images (include/gpx_delta.h), staged through CtlStage around the *_dev forms.
// Needs: gpx_host_stage.inc (CtlStage), gpx_image_host.inc (image_stage), gpx_delta_dev.inc.

namespace {
constexpr int32_t DELTA_GONE_CHUNK = 1 << 18; /* gone entries of one staged piece (== GPX_GROUP_CHUNK) */
}  // namespace

extern "C" {

int gpx_group_export_delta(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t flags, int32_t cap, void* o_rows,
                           int32_t cap_gone, int32_t* o_gone, gpx_delta_counts* counts) {
  int rc = delta_export_args(h, n, flags, cap, o_rows, cap_gone, o_gone, counts, false);
  if (rc != GPX_OK) return rc;
  if ((rc = delta_export_open(h, n)) != GPX_OK) return rc;
  const size_t stride = image_stride_bytes(h);
  /* entries per chunk: every one of them may need two rows */
  const int64_t per = std::max<int64_t>(1, (int64_t)(image_stage_bound(h) / (2 * stride)));
  gpx_delta_counts tot = {0, 0, 0, 0, 0, 0, 0, 0};
  bool cut = false; /* a group did not fit: nothing after it is written, the later chunks only count (and list the gone) */
  int64_t i0 = 0;
  do {
    const int32_t m = (int32_t)std::min<int64_t>(per, (int64_t)n - i0);
    const int32_t capc = cut ? 0 : (int32_t)std::min<int64_t>((int64_t)cap - tot.n_rows_done, 2 * (int64_t)m);
    const int32_t capg = (int32_t)std::min<int64_t>((int64_t)cap_gone - tot.n_gone_done, (int64_t)m);
    if (capc > 0 && (rc = image_stage(h, (size_t)capc * stride)) != GPX_OK) return rc;
    CtlStage t(h);
    const int32_t* d_g = (gidx && m) ? t.in(gidx + i0, (size_t)m) : nullptr;
    int32_t* d_x = capg > 0 ? t.tmp<int32_t>((size_t)capg, false) : nullptr;
    if (t.ready()) return t.rc;
    if (t.ran(delta_export_run(h, m, d_g, (int32_t)i0, flags, capc, capc > 0 ? h->img_stage : nullptr, capg, d_x,
                               (gpx_delta_counts*)h->delta_counts)))
      return t.rc;
    gpx_delta_counts c;
    t.d2h(&c, h->delta_counts, sizeof(c));
    if (t.sync()) return t.rc;
    if (c.n_rows_done > 0) t.d2h((char*)o_rows + (size_t)tot.n_rows_done * stride, h->img_stage, (size_t)c.n_rows_done * stride);
    if (c.n_gone_done > 0) t.d2h(o_gone + tot.n_gone_done, d_x, (size_t)c.n_gone_done * 4);
    if (t.sync()) return t.rc;
    tot.n_live += c.n_live;
    tot.n_changed += c.n_changed;
    tot.n_rows += c.n_rows;
    tot.n_done += c.n_done;
    tot.n_rows_done += c.n_rows_done;
    tot.n_gone += c.n_gone;
    tot.n_gone_done += c.n_gone_done;
    cut = cut || c.n_done < c.n_changed;
    i0 += m;
  } while (i0 < n);
  *counts = tot;
  return GPX_OK;
}

int gpx_group_apply_delta(gpx_engine* h, int32_t n_rows, const void* rows, const int32_t* gidx, int32_t flags,
                          uint8_t* status, int32_t n_gone, const int32_t* gone, uint8_t* gone_status) {
  int rc = delta_apply_args(h, n_rows, rows, flags, status, n_gone, gone, gone_status, false);
  if (rc != GPX_OK) return rc;
  if ((rc = delta_apply_open(h, n_rows, n_gone, flags)) != GPX_OK) return rc;
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
    if (t.ran(delta_rows_run(h, (int32_t)m, h->img_stage, d_g, d_st))) return t.rc;
    if ((rc = t.fetch({d_st})) != GPX_OK) return rc;
    r0 += m;
  }
  /* the gone list in chunks of 2^18 entries outside the arena, as the lifecycle calls go (gpx_group_host.inc): a long
   * list must not leave the arena grown for the life of the engine */
  for (int32_t i0 = 0; i0 < n_gone;) {
    const int32_t m = std::min<int32_t>(DELTA_GONE_CHUNK, n_gone - i0);
    CtlStage t(h, false);
    const int32_t* d_x = t.in(gone + i0, (size_t)m);
    uint8_t* d_st = t.out(gone_status + i0, (size_t)m);
    if (t.ready()) return t.rc;
    if (t.ran(delta_gone_run(h, m, d_x, d_st))) return t.rc;
    if ((rc = t.fetch({d_st})) != GPX_OK) return rc;
    i0 += m;
  }
  return GPX_OK;
}

} /* extern "C" */
