// Argument checks of the scans and the sweep that look at nothing but the arguments: shared by the *_dev calls
// (gpx_scan_dev.inc, gpx_sweep_dev.inc) and their host-pointer twins.
// Needs: NodeLists / GPX_MAX_NODE_LIST, include/gpx_sweep.h (GPX_SWEEP_PEEK / HOLD); the handle is only tested for null.

namespace {

/* what every scan checks before it uses the handle */
int scan_args(const gpx_engine* h, int32_t n, int32_t cap, const void* counts, std::initializer_list<const void*> cols) {
  if (!h || n < 0 || cap < 0 || !counts) return GPX_EINVAL;
  if (cap > 0)
    for (const void* c : cols)
      if (!c) return GPX_EINVAL;
  return GPX_OK;
}
int scan_lists(const int32_t* down_nodes, int32_t n_down, const int32_t* long_dead_nodes, int32_t n_long_dead,
               NodeLists* L) {
  if (n_down < 0 || n_long_dead < 0) return GPX_EINVAL;
  if (n_down > GPX_MAX_NODE_LIST || n_long_dead > GPX_MAX_NODE_LIST) return GPX_ECAPACITY;
  if ((n_down && !down_nodes) || (n_long_dead && !long_dead_nodes)) return GPX_EINVAL;
  memset(L, 0, sizeof(*L));
  L->n_down = n_down;
  L->n_long = n_long_dead;
  for (int32_t q = 0; q < n_down; q++) L->down[q] = down_nodes[q];
  for (int32_t q = 0; q < n_long_dead; q++) L->longdead[q] = long_dead_nodes[q];
  return GPX_OK;
}

/* what the sweep checks before it uses the handle */
int sweep_args(const gpx_engine* h, int32_t n, int32_t min_age, int32_t flags, int32_t cap, const void* o_gidx,
               const void* o_age, const void* o_rows, const void* counts) {
  if (!h || n < 0 || cap < 0 || !counts) return GPX_EINVAL;
  if (min_age < 0 || min_age > 255 || (flags & ~(GPX_SWEEP_PEEK | GPX_SWEEP_HOLD))) return GPX_EINVAL;
  if (cap > 0 && (!o_gidx || !o_age || !o_rows)) return GPX_EINVAL;
  return GPX_OK;
}

}  // namespace
