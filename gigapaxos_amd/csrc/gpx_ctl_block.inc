// What the six tile-compaction families (gpx_compact.hip.h) share on the host side: the size limit, the launch grid, the
// checks before a call uses the engine, and the ONE device block each family keeps its words in.
// Needs: the engine, dev_alloc and check_batch of gpx_engine.hip.

namespace {

/* the entries a call may name: a table scan covers max_groups, a listed call max_batch */
inline int64_t scan_max_n(const gpx_engine* e) { return std::max<int64_t>(e->cfg.max_groups, e->cfg.max_batch); }

/* the tile kernels' grid for n entries */
inline int tiles_for(int64_t n, int tile) { return (int)((n + tile - 1) / tile); }
/* ... and the tiles a family's parked columns and per-tile words are sized for, once: at least one */
inline size_t ctl_tiles(const gpx_engine* e, int tile) { return (size_t)std::max(tiles_for(scan_max_n(e), tile), 1); }

/* What a call needs of the engine once its arguments have passed: the size limit, an engine an exchange kernel gave up
 * on, the family's block - in this order, which decides the error a call with several faults returns. */
inline int ctl_open(gpx_engine* h, int64_t n, int64_t limit, int (*init)(gpx_engine*)) {
  if (n > limit) return GPX_ECAPACITY;
  int rc = check_batch(h, 0);
  if (rc != GPX_OK) return rc;
  return init(h);
}

/* One column of a family's block: the pointer field that will name it and its bytes. */
struct CtlCol {
  void* field;
  size_t bytes;
};
template <class T>
CtlCol ctl_col(T** field, size_t count) {
  return CtlCol{field, count * sizeof(T)};
}

/* A family's block: the columns in the order listed, each rounded up to 256 bytes, in ONE allocation - or at `into`
 * where a block of into_bytes that another family owns is large enough and may be shared (calls on one stream, of which
 * each reads only what it wrote).  A family lists its counts LAST: that pointer is the marker its init tests, and the
 * words the host twins fetch.  `zero` for a family that keeps engine state in the block; scratch is never cleared
 * (gpx_compact.hip.h).  No field is assigned before the allocation has succeeded: a failed one leaves nothing behind
 * and the engine usable. */
int ctl_block(gpx_engine* e, std::initializer_list<CtlCol> cols, bool zero, char* into = nullptr, size_t into_bytes = 0) {
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  size_t need = 0;
  for (const CtlCol& c : cols) need += up(c.bytes);
  char* p = into_bytes >= need ? into : nullptr;
  if (!p) {
    int rc = dev_alloc(e, &p, need, zero);
    if (rc != GPX_OK) return rc;
  }
  for (const CtlCol& c : cols) {
    memcpy(c.field, &p, sizeof(p)); /* every object pointer has char*'s representation here */
    p += up(c.bytes);
  }
  return GPX_OK;
}

}  // namespace
