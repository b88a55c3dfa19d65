// Lifecycle calls of include/gpx.h: gpx_group_create, gpx_group_retire, gpx_group_snapshot.  They change group state:
// everything on the back-end stream, in call order.
// Needs: gpx_host_stage.inc (CtlStage), check_batch, LAUNCH, grid_for, NameCopies.

namespace {

/* records per launch: creation and retirement are not on the data path, a table of any size goes through buffers of
 * this many records, allocated once per call and outside the arena */
constexpr int32_t GPX_GROUP_CHUNK = 1 << 18;

int retire_impl(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t mode, gpx_hri* rows, uint8_t* status) {
  if (!h || n < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (!gidx) return GPX_EINVAL;
  const size_t c0 = (size_t)std::min(n, GPX_GROUP_CHUNK);
  CtlStage t(h, false);
  int32_t* d_g = t.tmp<int32_t>(c0, false);
  uint8_t* d_s = t.tmp<uint8_t>(c0, false);
  gpx_hri* d_r = t.tmp<gpx_hri>(c0, false);
  int rc = t.rc;
  for (int32_t o = 0; o < n && rc == GPX_OK; o += GPX_GROUP_CHUNK) {
    const size_t c = (size_t)std::min(GPX_GROUP_CHUNK, n - o);
    t.h2d(d_g, gidx + o, c * 4);
    if (t.rc != GPX_OK) return t.rc;
    LAUNCH(h, "k_group_retire", k_group_retire, grid_for(c), h->S, (int32_t)c, (const int32_t*)d_g, mode, d_r, d_s,
           NameCopies{h->N.rows, (uint8_t*)h->N.tab});
    if (rows) t.d2h(rows + o, d_r, c * sizeof(gpx_hri));
    if (status) t.d2h(status + o, d_s, c);
    if (t.sync()) return t.rc;
    rc = check_batch(h, 0); /* a snapshot of a table an exchange kernel left half-written is not a snapshot (ADVICE r5) */
  }
  return rc;
}

}  // namespace

extern "C" {

int gpx_group_create(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* members,
                     const uint8_t* k, const gpx_hri* rows, uint8_t* status) {
  if (!h || n < 0) return GPX_EINVAL;
  if (n == 0) return GPX_OK;
  if (!gidx || !members || !k || !rows) return GPX_EINVAL;
  const size_t c0 = (size_t)std::min(n, GPX_GROUP_CHUNK), K = (size_t)h->cfg.kmax;
  CtlStage t(h, false);
  int32_t *d_g = t.tmp<int32_t>(c0, false), *d_m = t.tmp<int32_t>(c0 * K, false);
  uint8_t *d_k = t.tmp<uint8_t>(c0, false), *d_s = t.tmp<uint8_t>(c0, false);
  gpx_hri* d_r = t.tmp<gpx_hri>(c0, false);
  int rc = t.rc;
  for (int32_t o = 0; o < n && rc == GPX_OK; o += GPX_GROUP_CHUNK) {
    const size_t c = (size_t)std::min(GPX_GROUP_CHUNK, n - o);
    t.h2d(d_g, gidx + o, c * 4);
    t.h2d(d_m, members + (size_t)o * K, c * 4 * K);
    t.h2d(d_k, k + o, c);
    t.h2d(d_r, rows + o, c * sizeof(gpx_hri));
    if (t.rc != GPX_OK) return t.rc;
    LAUNCH(h, "k_group_create", k_group_create, grid_for(c), h->S, (int32_t)c, (const int32_t*)d_g, (const int32_t*)d_m,
           (const uint8_t*)d_k, (const gpx_hri*)d_r, d_s, NameCopies{h->N.rows, (uint8_t*)h->N.tab});
    if (status) t.d2h(status + o, d_s, c);
    if (t.sync()) return t.rc;
    rc = check_batch(h, 0); /* (an exchange kernel that gave up before this call: the table is not to be built on) */
  }
  return rc;
}

int gpx_group_retire(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t mode, gpx_hri* rows,
                     uint8_t* status) {
  if (mode != GPX_RETIRE_PAUSE && mode != GPX_RETIRE_KILL) return GPX_EINVAL;
  return retire_impl(h, n, gidx, mode, rows, status);
}

int gpx_group_snapshot(gpx_engine* h, int32_t n, const int32_t* gidx, gpx_hri* rows,
                       uint8_t* status) {
  if (!rows) return GPX_EINVAL;
  return retire_impl(h, n, gidx, 2, rows, status);
}

} /* extern "C" */
