// Device-pointer side of the log index (include/gpx_logindex.h; kernels in gpx_logindex.hip.h): open, the argument
// checks and the seven _dev calls; the host-pointer twins: gpx_logindex_host.inc.
// Needs: the engine and the kernels of gpx_engine.hip, gpx_ctl_block.inc.

namespace {

static_assert(GPX_LI_ADDED == GPX_LI_ADDED_ && GPX_LI_STALE == GPX_LI_STALE_ && GPX_LI_NOGROUP == GPX_LI_NOGROUP_ &&
                  GPX_LI_FULL == GPX_LI_FULL_ && GPX_LI_REPEAT == GPX_LI_REPEAT_,
              "include/gpx_logindex.h and gpx_logindex.hip.h disagree on the status bytes");
static_assert(GPX_LI_RESET == GPX_LI_RESET_ && GPX_LI_MAX_FILES == GPX_LI_MAX_FILES_,
              "include/gpx_logindex.h and gpx_logindex.hip.h disagree on the flag or the bins");
static_assert(sizeof(gpx_logindex_counts) == 32 && sizeof(LiCounts) == 32, "gpx_logindex_counts is 32 bytes");
static_assert(GPX_LI_TILE == GPX_BLOCK, "a tile is one pass of a workgroup");

#define GPX_LI_MAX_ROWS (INT32_MAX - 511) /* the last tile's rows still fit an int32 */

/* The checks every call but open shares, in the order that decides the error: the handle and counts, the batch limit,
 * then whether the index is open.  Of the handle only cfg.max_batch is read before that last test. */
int li_common(const gpx_engine* h, const void* counts, int64_t n) {
  if (!h || !counts || n < 0) return GPX_EINVAL;
  if (n > h->cfg.max_batch) return GPX_ECAPACITY;
  return h->li_counts ? GPX_OK : GPX_EINVAL;
}

bool li_any_null(std::initializer_list<const void*> cols) {
  for (const void* c : cols)
    if (!c) return true;
  return false;
}

/* an engine an exchange kernel gave up on is refused; then every launch goes to the back-end stream */
int li_begin(gpx_engine* h) {
  int rc = check_batch(h, 0);
  if (rc != GPX_OK) return rc;
  h->stream = h->sB;
  return GPX_OK;
}

/* the grid of a scan over the table: the host's upper bound of the tail (gpx_logindex.hip.h) */
int li_row_tiles(const gpx_engine* h) { return tiles_for(h->li_ub, GPX_LI_TILE); }

int li_add_args(const gpx_engine* h, int32_t n, const int32_t* e_gidx, const int32_t* e_slot, const int32_t* e_bnum,
                const int32_t* e_bcoord, const int64_t* e_off, const int32_t* e_len, int32_t file, const void* counts) {
  if (file < 0 || (n > 0 && li_any_null({e_gidx, e_slot, e_bnum, e_bcoord, e_off, e_len}))) return GPX_EINVAL;
  return li_common(h, counts, n);
}
int li_set_gc_args(const gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* gc_slot, int32_t flags,
                   const void* counts) {
  if ((flags & ~GPX_LI_RESET) || (n > 0 && (!gidx || (!gc_slot && !(flags & GPX_LI_RESET))))) return GPX_EINVAL;
  return li_common(h, counts, n);
}
int li_lookup_args(const gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* min_slot, const int32_t* max_slot,
                   const uint8_t* has_max, int32_t cap, std::initializer_list<const void*> outs, const void* counts) {
  if (cap < 0 || (n > 0 && (!gidx || !min_slot || (has_max && !max_slot))) || (cap > 0 && li_any_null(outs)))
    return GPX_EINVAL;
  return li_common(h, counts, n);
}
int li_file_rows_args(const gpx_engine* h, int32_t cap, std::initializer_list<const void*> outs, const void* counts) {
  if (cap < 0 || (cap > 0 && li_any_null(outs))) return GPX_EINVAL;
  return li_common(h, counts, 0);
}
int li_relocate_args(const gpx_engine* h, int32_t n, const int32_t* o_row, int32_t new_file, const int64_t* k_off,
                     const int32_t* k_len, const void* counts) {
  if (new_file < 0 || (n > 0 && li_any_null({o_row, k_off, k_len}))) return GPX_EINVAL;
  return li_common(h, counts, n);
}
int li_files_args(const gpx_engine* h, int32_t n_files, const void* counts) {
  if (n_files < 0 || n_files > GPX_LI_MAX_FILES) return GPX_EINVAL;
  return li_common(h, counts, 0);
}

}  // namespace

extern "C" {

/* ONE block: the two blocks of row columns, the per-group words, the header words, the parked entries, the per-tile
 * words and the host twins' counts.  The per-group words start at -1 / idle (all bits set), the header at zero; the rest
 * is scratch or lies past the tail.  Nothing of the engine changes before everything has succeeded. */
int gpx_logindex_open(gpx_engine* h, int32_t cap_rows) {
  if (!h || h->li_counts || cap_rows < 1 || cap_rows > GPX_LI_MAX_ROWS) return GPX_EINVAL;
  int rc = check_batch(h, 0);
  if (rc != GPX_OK) return rc;
  const size_t R = (size_t)cap_rows, G = (size_t)std::max(h->cfg.max_groups, 1);
  const size_t B = (size_t)std::max(h->cfg.max_batch, 1);
  const size_t tiles = (size_t)tiles_for((int64_t)std::max({R, G, B}), GPX_LI_TILE);
  const size_t rec_tiles = (size_t)tiles_for((int64_t)B, GPX_LI_TILE);
  const size_t park = (size_t)tiles_for((int64_t)std::max(R, B), GPX_LI_TILE) * GPX_LI_TILE;
  LiMem M{};
  LiCounts* counts = nullptr;
  M.cap_rows = cap_rows, M.G = h->cfg.max_groups;
  rc = ctl_block(h,
                 {ctl_col(&M.gc, G), ctl_col(&M.min_file, G), ctl_col(&M.arm, G), ctl_col(&M.first, G),
                  ctl_col(&M.hdr, (size_t)LI_HDR_WORDS), ctl_col(&M.T.gidx, R), ctl_col(&M.T.slot, R), ctl_col(&M.T.bnum, R),
                  ctl_col(&M.T.bcoord, R), ctl_col(&M.T.file, R), ctl_col(&M.T.off, R), ctl_col(&M.T.len, R),
                  ctl_col(&M.T.alive, R), ctl_col(&M.U.gidx, R), ctl_col(&M.U.slot, R), ctl_col(&M.U.bnum, R),
                  ctl_col(&M.U.bcoord, R), ctl_col(&M.U.file, R), ctl_col(&M.U.off, R), ctl_col(&M.U.len, R),
                  ctl_col(&M.U.alive, R), ctl_col(&M.park, park), ctl_col(&M.tile_cnt, tiles), ctl_col(&M.tile_off, tiles),
                  ctl_col(&M.rt_a, rec_tiles), ctl_col(&M.rt_b, rec_tiles), ctl_col(&M.rt_c, rec_tiles),
                  ctl_col(&counts, (size_t)1)},
                 false);
  if (rc != GPX_OK) return rc;
  HIPCHK(hipMemsetAsync(M.gc, 0xff, G * 4, h->sB));
  HIPCHK(hipMemsetAsync(M.min_file, 0xff, G * 4, h->sB));
  HIPCHK(hipMemsetAsync(M.arm, 0xff, G * 4, h->sB));
  HIPCHK(hipMemsetAsync(M.first, 0xff, G * 4, h->sB));
  HIPCHK(hipMemsetAsync(M.hdr, 0, LI_HDR_WORDS * 4, h->sB));
  HIPCHK(hipStreamSynchronize(h->sB));
  h->li = M;
  h->li_ub = 0;
  h->li_counts = counts; /* last: the marker */
  return GPX_OK;
}

int gpx_logindex_add_dev(gpx_engine* h, int32_t n, const int32_t* n_dev, const int32_t* e_gidx, const int32_t* e_slot,
                         const int32_t* e_bnum, const int32_t* e_bcoord, const int64_t* e_off, const int32_t* e_len,
                         int32_t file, uint8_t* status, gpx_logindex_counts* counts) {
  int rc = li_add_args(h, n, e_gidx, e_slot, e_bnum, e_bcoord, e_off, e_len, file, counts);
  if (rc != GPX_OK) return rc;
  if ((rc = li_begin(h)) != GPX_OK) return rc;
  const int ntiles = tiles_for(n, GPX_LI_TILE);
  const LiRowsIn I{e_gidx, e_slot, e_bnum, e_bcoord, (const long long*)e_off, e_len};
  if (ntiles) LAUNCH(h, "k_li_add_tile", k_li_add_tile, ntiles, h->li, n, n_dev, e_gidx, e_slot, status);
  LAUNCH(h, "k_li_add_offsets", k_li_add_offsets, 1, (int32_t)ntiles, h->li, (LiCounts*)counts);
  if (ntiles) LAUNCH(h, "k_li_add_move", k_li_add_move, ntiles, h->li, I, file, status);
  HIPCHK(hipGetLastError());
  h->li_ub = std::min<int64_t>(h->li.cap_rows, h->li_ub + n);
  return GPX_OK;
}

int gpx_logindex_set_gc_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* gc_slot, int32_t flags,
                            uint8_t* status, gpx_logindex_counts* counts) {
  int rc = li_set_gc_args(h, n, gidx, gc_slot, flags, counts);
  if (rc != GPX_OK) return rc;
  if ((rc = li_begin(h)) != GPX_OK) return rc;
  const int ntiles = tiles_for(n, GPX_LI_TILE), rows = ntiles ? li_row_tiles(h) : 0;
  if (ntiles) {
    LAUNCH(h, "k_li_arm", k_li_arm, ntiles, h->li, n, gidx);
    LAUNCH(h, "k_li_mark_gc", k_li_mark<true>, ntiles, h->li, n, gidx, gc_slot, flags, status);
    if (rows) LAUNCH(h, "k_li_gc_scan", k_li_gc_scan, rows, h->li, flags);
    LAUNCH(h, "k_li_gc_finish", k_li_gc_finish, ntiles, h->li, n, gidx);
  }
  LAUNCH(h, "k_li_gc_sum", k_li_gc_sum, 1, (int32_t)ntiles, (int32_t)rows, h->li, (LiCounts*)counts);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

int gpx_logindex_lookup_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* min_slot,
                            const int32_t* max_slot, const uint8_t* has_max, int32_t cap, int32_t* o_rec, int32_t* o_row,
                            int32_t* o_slot, int32_t* o_bnum, int32_t* o_bcoord, int32_t* o_file, int64_t* o_off,
                            int32_t* o_len, uint8_t* status, gpx_logindex_counts* counts) {
  int rc = li_lookup_args(h, n, gidx, min_slot, max_slot, has_max, cap,
                          {o_rec, o_row, o_slot, o_bnum, o_bcoord, o_file, o_off, o_len}, counts);
  if (rc != GPX_OK) return rc;
  if ((rc = li_begin(h)) != GPX_OK) return rc;
  const int ntiles = tiles_for(n, GPX_LI_TILE), rows = ntiles ? li_row_tiles(h) : 0;
  const LiQuery Q{min_slot, max_slot, has_max};
  const LiOut O{o_rec, o_row, nullptr, o_slot, o_bnum, o_bcoord, o_file, (long long*)o_off, o_len, nullptr};
  if (ntiles) {
    LAUNCH(h, "k_li_arm", k_li_arm, ntiles, h->li, n, gidx);
    LAUNCH(h, "k_li_mark", k_li_mark<false>, ntiles, h->li, n, gidx, (const int32_t*)nullptr, 0, status);
    if (rows) LAUNCH(h, "k_li_scan_lookup", k_li_scan<LI_SCAN_LOOKUP>, rows, h->li, Q, 0);
  }
  LAUNCH(h, "k_li_offsets_lookup", k_li_scan_offsets<LI_SCAN_LOOKUP>, 1, (int32_t)ntiles, (int32_t)rows, h->li, cap,
         (LiCounts*)counts);
  if (rows && cap > 0) LAUNCH(h, "k_li_move_lookup", k_li_scan_move<LI_SCAN_LOOKUP>, rows, h->li, cap, O);
  if (ntiles) LAUNCH(h, "k_li_disarm", k_li_disarm, ntiles, h->li, n, gidx);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

int gpx_logindex_file_rows_dev(gpx_engine* h, int32_t file, int32_t cap, int32_t* o_row, int32_t* e_gidx, int32_t* e_slot,
                               int32_t* e_bnum, int32_t* e_bcoord, int64_t* e_off, int32_t* e_len, int32_t* e_gc,
                               gpx_logindex_counts* counts) {
  int rc = li_file_rows_args(h, cap, {o_row, e_gidx, e_slot, e_bnum, e_bcoord, e_off, e_len, e_gc}, counts);
  if (rc != GPX_OK) return rc;
  if ((rc = li_begin(h)) != GPX_OK) return rc;
  const int rows = li_row_tiles(h);
  const LiOut O{nullptr, o_row, e_gidx, e_slot, e_bnum, e_bcoord, nullptr, (long long*)e_off, e_len, e_gc};
  if (rows) LAUNCH(h, "k_li_scan_file", k_li_scan<LI_SCAN_FILE>, rows, h->li, LiQuery{}, file);
  LAUNCH(h, "k_li_offsets_file", k_li_scan_offsets<LI_SCAN_FILE>, 1, 0, (int32_t)rows, h->li, cap, (LiCounts*)counts);
  if (rows && cap > 0) LAUNCH(h, "k_li_move_file", k_li_scan_move<LI_SCAN_FILE>, rows, h->li, cap, O);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

int gpx_logindex_relocate_dev(gpx_engine* h, int32_t n, const int32_t* n_dev, int32_t generation, const int32_t* o_row,
                              const int32_t* k_src, int32_t new_file, const int64_t* k_off, const int32_t* k_len,
                              gpx_logindex_counts* counts) {
  int rc = li_relocate_args(h, n, o_row, new_file, k_off, k_len, counts);
  if (rc != GPX_OK) return rc;
  if ((rc = li_begin(h)) != GPX_OK) return rc;
  const int ntiles = tiles_for(n, GPX_LI_TILE);
  if (ntiles)
    LAUNCH(h, "k_li_reloc", k_li_reloc, ntiles, h->li, n, n_dev, generation, o_row, k_src, new_file,
           (const long long*)k_off, k_len);
  LAUNCH(h, "k_li_reloc_sum", k_li_reloc_sum, 1, (int32_t)ntiles, h->li, (LiCounts*)counts);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

int gpx_logindex_files_dev(gpx_engine* h, int32_t file_base, int32_t n_files, int32_t* o_rows, int32_t* o_groups,
                           int32_t* o_min_file, gpx_logindex_counts* counts) {
  int rc = li_files_args(h, n_files, counts);
  if (rc != GPX_OK) return rc;
  if ((rc = li_begin(h)) != GPX_OK) return rc;
  const int row_wgs = std::min(li_row_tiles(h), GPX_LI_HIST_GRID);
  const int grp_wgs = std::min(tiles_for(h->li.G, GPX_LI_TILE), GPX_LI_HIST_GRID);
  LAUNCH(h, "k_li_files_init", k_li_files_init, std::max(tiles_for(n_files, GPX_BLOCK), 1), h->li, n_files, o_rows,
         o_groups);
  if (row_wgs)
    LAUNCH(h, "k_li_files_rows", k_li_files_hist<false>, row_wgs, h->li, file_base, n_files, o_rows, h->li.tile_cnt);
  if (grp_wgs)
    LAUNCH(h, "k_li_files_groups", k_li_files_hist<true>, grp_wgs, h->li, file_base, n_files, o_groups, h->li.tile_off);
  LAUNCH(h, "k_li_files_sum", k_li_files_sum, 1, (int32_t)row_wgs, (int32_t)grp_wgs, h->li, o_min_file,
         (LiCounts*)counts);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

/* The host's record of the blocks is swapped when the call is queued: every later call is queued behind it. */
int gpx_logindex_compact_dev(gpx_engine* h, gpx_logindex_counts* counts) {
  int rc = li_common(h, counts, 0);
  if (rc != GPX_OK) return rc;
  if ((rc = li_begin(h)) != GPX_OK) return rc;
  const int rows = li_row_tiles(h);
  if (rows) LAUNCH(h, "k_li_scan_alive", k_li_scan<LI_SCAN_ALIVE>, rows, h->li, LiQuery{}, 0);
  LAUNCH(h, "k_li_offsets_alive", k_li_scan_offsets<LI_SCAN_ALIVE>, 1, 0, (int32_t)rows, h->li, INT32_MAX,
         (LiCounts*)counts);
  if (rows) LAUNCH(h, "k_li_move_alive", k_li_scan_move<LI_SCAN_ALIVE>, rows, h->li, INT32_MAX, LiOut{});
  HIPCHK(hipGetLastError());
  std::swap(h->li.T, h->li.U);
  return GPX_OK;
}

} /* extern "C" */
