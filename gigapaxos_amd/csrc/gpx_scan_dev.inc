// Device-pointer side of the hit-compacting scans (include/gpx_scan.h; kernels in gpx_scan.hip.h): the scratch, the
// engine-side checks and the *_dev calls; the host-pointer twins: gpx_scan_host.inc.
// Needs: the engine and the kernels of gpx_engine.hip, elect_init (gpx_elect_dev.inc), gpx_ctl_args.inc, gpx_ctl_block.inc.

namespace {

static_assert(GPX_SCAN_TILE == GPX_SCAN_TILE_, "include/gpx_scan.h and gpx_scan.hip.h disagree on the tile");
static_assert(GPX_SCAN_TILE % GPX_BLOCK == 0, "a tile is whole passes of a workgroup");
static_assert(sizeof(gpx_scan_counts) == 16 && sizeof(ScanCounts) == 16, "gpx_scan_counts is 16 bytes");

/* The parked rows, the per-tile words and the host twins' counts: ONE block (ctl_block), allocated by the first scan
 * and sized once for max(max_groups, max_batch) entries in whole tiles.  Not cleared. */
int scan_init(gpx_engine* e) {
  if (e->scan_counts) return GPX_OK;
  const size_t tiles = ctl_tiles(e, GPX_SCAN_TILE), cap = tiles * GPX_SCAN_TILE, tl = (tiles * 4 + 255) & ~(size_t)255;
  if (cap > UINT32_MAX) return GPX_ECAPACITY;
  ScanScratch X{nullptr, (uint32_t)cap, (uint32_t)tl};
  int rc = ctl_block(e, {ctl_col(&X.base, 26 * cap + 3 * tl) /* ScanScratch's layout */, ctl_col(&e->scan_counts, 1)}, false);
  if (rc == GPX_OK) e->scan = X;
  return rc;
}

/* ctl_open for this family, under the name its host-pointer twin calls */
int scan_open(gpx_engine* h, int32_t n) { return ctl_open(h, n, scan_max_n(h), scan_init); }

/* the three launches of one scan on the back-end stream (gpx_scan.hip.h) */
template <class E>
int scan_run(gpx_engine* h, const char* tile_name, const char* move_name, int32_t n, const int32_t* gidx, const E& ev,
             int32_t cap, const ScanOut& O, gpx_scan_counts* counts) {
  h->stream = h->sB;
  const int ntiles = tiles_for(n, GPX_SCAN_TILE);
  if (ntiles) LAUNCH(h, tile_name, (k_scan_tile<E>), ntiles, h->S, n, gidx, ev, h->scan);
  LAUNCH(h, "k_scan_offsets", k_scan_offsets, 1, (int32_t)ntiles, h->scan, (ScanCounts*)counts);
  if (ntiles && cap > 0) LAUNCH(h, move_name, (k_scan_move<E>), ntiles, h->scan, O, cap);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

}  // namespace

extern "C" {

int gpx_election_scan_hits_dev(gpx_engine* h, int32_t n, const int32_t* gidx, const int32_t* down_nodes,
                               int32_t n_down, const int32_t* long_dead_nodes, int32_t n_long_dead, int32_t force,
                               int32_t cap, int32_t* o_gidx, uint8_t* o_run, int32_t* o_bnum, int32_t* o_first,
                               gpx_scan_counts* counts) {
  int rc = scan_args(h, n, cap, counts, {o_gidx, o_run, o_bnum, o_first});
  if (rc != GPX_OK) return rc;
  ScanElection ev;
  if ((rc = scan_lists(down_nodes, n_down, long_dead_nodes, n_long_dead, &ev.L)) != GPX_OK) return rc;
  ev.force = force;
  if ((rc = scan_open(h, n)) != GPX_OK) return rc;
  ScanOut O{};
  O.i32[0] = o_gidx, O.u8[0] = o_run, O.i32[1] = o_bnum, O.i32[2] = o_first;
  return scan_run(h, "k_scan_election_tile", "k_scan_election_move", n, gidx, ev, cap, O, counts);
}

int gpx_poke_scan_hits_dev(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t cap, int32_t* o_gidx,
                           uint8_t* o_poke, int32_t* o_slot, int32_t* o_bnum, int32_t* o_bcoord,
                           int32_t* o_median_cp, uint8_t* o_flags, uint32_t* o_heard, gpx_scan_counts* counts) {
  int rc = scan_args(h, n, cap, counts, {o_gidx, o_poke, o_slot, o_bnum, o_bcoord, o_median_cp, o_flags, o_heard});
  if (rc != GPX_OK) return rc;
  if ((rc = scan_open(h, n)) != GPX_OK) return rc;
  ScanOut O{};
  O.i32[0] = o_gidx, O.u8[0] = o_poke, O.i32[1] = o_slot, O.i32[2] = o_bnum, O.i32[3] = o_bcoord;
  O.i32[4] = o_median_cp, O.u8[1] = o_flags, O.i32[5] = (int32_t*)o_heard;
  const char *tn = "k_scan_poke_tile", *mn = "k_scan_poke_move";
  if (h->cfg.kmax <= 4) return scan_run(h, tn, mn, n, gidx, ScanPoke<4>{}, cap, O, counts);
  if (h->cfg.kmax <= 8) return scan_run(h, tn, mn, n, gidx, ScanPoke<8>{}, cap, O, counts);
  return scan_run(h, tn, mn, n, gidx, ScanPoke<16>{}, cap, O, counts);
}

int gpx_gap_scan_hits_dev(gpx_engine* h, int32_t n, const int32_t* gidx, int32_t threshold, int32_t sync_mode,
                          int32_t size_limit, int32_t require, int32_t cap, int32_t* o_gidx, int32_t* o_first,
                          int32_t* o_max_committed, uint64_t* o_missing, uint8_t* o_sync, gpx_scan_counts* counts) {
  int rc = scan_args(h, n, cap, counts, {o_gidx, o_first, o_max_committed, o_missing, o_sync});
  if (rc != GPX_OK) return rc;
  if ((rc = scan_open(h, n)) != GPX_OK) return rc;
  ScanOut O{};
  O.i32[0] = o_gidx, O.i32[1] = o_first, O.i32[2] = o_max_committed, O.u64 = (unsigned long long*)o_missing;
  O.u8[0] = o_sync;
  return scan_run(h, "k_scan_gap_tile", "k_scan_gap_move", n, gidx, ScanGap{threshold, sync_mode, size_limit, require},
                  cap, O, counts);
}

int gpx_election_begin_hits_dev(gpx_engine* h, int32_t cap, const gpx_scan_counts* counts, const int32_t* gidx,
                                const int32_t* bnum, uint8_t* e_status) {
  if (!h || cap < 0) return GPX_EINVAL;
  if (cap == 0) return GPX_OK;
  if (!counts || !gidx || !bnum || !e_status) return GPX_EINVAL;
  if ((int64_t)cap > scan_max_n(h)) return GPX_ECAPACITY;
  int rc = check_batch(h, 0);
  if (rc != GPX_OK) return rc;
  if ((rc = elect_init(h)) != GPX_OK) return rc;
  h->stream = h->sB;
  LAUNCH(h, "k_scan_election_begin", k_scan_election_begin, grid_for(cap), h->S, cap, (const ScanCounts*)counts, gidx,
         bnum, e_status);
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

} /* extern "C" */
