// Device-pointer side of the journal compaction (include/gpx_journal_gc.h; kernels in gpx_journal_gc.hip.h): the
// scratch, the argument checks and gpx_journal_gc_dev; the host-pointer twin: gpx_journal_gc_host.inc.
// Needs: the engine and the kernels of gpx_engine.hip.

namespace {

static_assert(GPX_JG_COUNT_ONLY == GPX_JG_COUNT_ONLY_ && GPX_JG_SKIP_UNCHANGED == GPX_JG_SKIP_UNCHANGED_,
              "include/gpx_journal_gc.h and gpx_journal_gc.hip.h disagree on the flags");
static_assert(GPX_JG_DROP == GPX_JG_DROP_ && GPX_JG_KEEP == GPX_JG_KEEP_ && GPX_JG_KEEP_UNJUDGED == GPX_JG_KEEP_UNJUDGED_ &&
                  GPX_JG_BAD == GPX_JG_BAD_,
              "include/gpx_journal_gc.h and gpx_journal_gc.hip.h disagree on the verdicts");
static_assert(GPX_JG_GF_EXISTS == GF_EXISTS, "gpx_journal_gc.hip.h and gpx_kernels.hip.h disagree on the exists bit");
static_assert(sizeof(gpx_journal_gc_counts) == 64 && sizeof(JgCounts) == 64, "gpx_journal_gc_counts is 64 bytes");

/* the arguments of one call, as both forms take them */
struct JgArgs {
  int32_t n;
  const uint8_t* in;
  int64_t in_bytes, in_base;
  const int32_t *e_gidx, *e_slot;
  const int64_t* e_off;
  const int32_t *e_len, *e_bnum, *e_bcoord, *cp_slot;
  int64_t out_base;
  int32_t flags;
  uint8_t* out;
  int64_t cap_bytes;
  int32_t cap_entries;
  uint8_t* verdict;
  int32_t *k_src, *k_gidx, *k_slot, *k_bnum, *k_bcoord;
  int64_t* k_off;
  int32_t* k_len;
  gpx_journal_gc_counts* counts;
};

/* what a compaction call checks before it does anything else; of the handle only cfg.max_batch is read */
int jg_args(const gpx_engine* h, const JgArgs& a) {
  if (!h || !a.counts || a.n < 0 || a.in_bytes < 0 || a.cap_bytes < 0 || a.cap_entries < 0 ||
      (a.flags & ~(GPX_JG_COUNT_ONLY | GPX_JG_SKIP_UNCHANGED)))
    return GPX_EINVAL;
  if (((uintptr_t)a.in & 15) || ((uintptr_t)a.out & 15)) return GPX_EINVAL;
  if (a.n > 0) {
    if (!a.e_gidx || !a.e_slot || !a.e_off || !a.e_len) return GPX_EINVAL;
    if ((a.k_bnum && !a.e_bnum) || (a.k_bcoord && !a.e_bcoord)) return GPX_EINVAL;
    if (!(a.flags & GPX_JG_COUNT_ONLY) && (!a.in || !a.out || !a.k_off || !a.k_len)) return GPX_EINVAL;
  }
  if (a.n > h->cfg.max_batch) return GPX_ECAPACITY;
  return GPX_OK;
}

/* The per-tile words, one descriptor per row of the largest batch and the host twin's counts: ONE block, allocated by
 * the first call.  All of it is scratch of which a call reads only what it wrote: not zeroed.  A failed allocation
 * leaves nothing behind and the engine usable. */
int jg_init(gpx_engine* e) {
  if (e->jg_counts) return GPX_OK;
  const size_t N = (size_t)std::max(e->cfg.max_batch, 1);
  const size_t tiles = (N + GPX_JR_TILE - 1) / GPX_JR_TILE;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t b_t4 = up(tiles * 4), b_t8 = up(tiles * 8), b_d8 = up(N * 8);
  char* base = nullptr;
  int rc = dev_alloc(e, &base, 6 * b_t4 + 3 * b_t8 + 2 * b_d8 + 256 + 256, false);
  if (rc != GPX_OK) return rc;
  if (const char* sv = getenv("GPX_TEST_JOURNAL_STAGE")) { /* tests: the host twin's windows */
    const long long v = atoll(sv);
    if (v > 0) e->jr_stage_max = (size_t)v;
  }
  JgMem& M = e->jg;
  char* p = base;
  M.tile_bytes = (long long*)p, p += b_t8;
  M.tile_named = (long long*)p, p += b_t8;
  M.tile_boff = (long long*)p, p += b_t8;
  M.d_pos = (long long*)p, p += b_d8;
  M.d_src = (long long*)p, p += b_d8;
  M.tile_cnt = (int32_t*)p, p += b_t4;
  M.tile_heads = (int32_t*)p, p += b_t4;
  M.tile_bad = (int32_t*)p, p += b_t4;
  M.tile_unj = (int32_t*)p, p += b_t4;
  M.tile_eoff = (int32_t*)p, p += b_t4;
  M.tile_hoff = (int32_t*)p, p += b_t4;
  M.first_ok = (int32_t*)p, p += 256;
  e->jg_counts = (JgCounts*)p; /* last: the marker */
  return GPX_OK;
}

/* what the call needs of the engine: one an exchange kernel gave up on is refused; the scratch */
int jg_open(gpx_engine* h) {
  int rc = check_batch(h, 0);
  if (rc != GPX_OK) return rc;
  return jg_init(h);
}

/* The launches (gpx_journal_gc.hip.h) on the back-end stream, behind everything queued on the engine so far.  `in` is
 * device memory that holds bytes [win_lo, win_hi) of the caller's block, or null (no prefix test, nothing copied): the
 * _dev form passes its block and [0, in_bytes), the host twin's second pass the window it staged, its rows [row_base,
 * row_base + a.n) and in `force` the verdicts of its first pass. */
int jg_run(gpx_engine* h, const JgArgs& a, const uint8_t* in, int64_t win_lo, int64_t win_hi, int32_t row_base,
           const uint8_t* force) {
  h->stream = h->sB;
  JgIn I;
  I.in = in, I.win_lo = win_lo, I.win_hi = win_hi, I.in_base = a.in_base;
  I.e_gidx = a.e_gidx, I.e_slot = a.e_slot, I.e_off = (const long long*)a.e_off, I.e_len = a.e_len;
  I.e_bnum = a.e_bnum, I.e_bcoord = a.e_bcoord, I.cp_slot = a.cp_slot, I.force = force;
  I.g_flags = h->S.g_flags, I.a_gc = h->S.a_gc, I.max_groups = h->S.G;
  I.n = a.n, I.row_base = row_base;
  const JgOut O{a.out,    (long long)a.cap_bytes, (long long)a.out_base, a.cap_entries,       a.k_src, a.k_gidx,
                a.k_slot, a.k_bnum,               a.k_bcoord,            (long long*)a.k_off, a.k_len};
  JgCounts* counts = (JgCounts*)a.counts;
  const int ntiles = (int)(((int64_t)a.n + GPX_JR_TILE - 1) / GPX_JR_TILE);
  if (ntiles) LAUNCH(h, "k_jg_tile", k_jg_tile, ntiles, I, h->jg, a.verdict);
  LAUNCH(h, "k_jg_offsets", k_jg_offsets, 1, (int32_t)ntiles, I, h->jg, (long long)a.cap_bytes, a.cap_entries, a.flags,
         (long long)a.in_bytes, counts);
  /* an entry is at least 4 bytes: below that nothing can be done */
  if (ntiles && !(a.flags & GPX_JG_COUNT_ONLY) && a.cap_entries > 0 && a.cap_bytes >= 4) {
    LAUNCH(h, "k_jg_rows", k_jg_rows, ntiles, I, h->jg, O, (const JgCounts*)counts);
    /* copy: persistent workgroups over the 16 KB tiles of what fits cap_bytes (bytes_done is still on the device; rows
     * may name a range twice, so in_bytes bounds nothing): eight per CU of the chip's 256, as k_jr_copy */
    const int64_t tiles = a.cap_bytes / GPX_JR_CTILE + 1;
    LAUNCH(h, "k_jg_copy", k_jg_copy, (int)std::min<int64_t>(tiles, 2048), in, h->jg, a.out, (const JgCounts*)counts);
  }
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

}  // namespace

extern "C" {

int gpx_journal_gc_dev(gpx_engine* h, int32_t n, const uint8_t* in, int64_t in_bytes, int64_t in_base,
                       const int32_t* e_gidx, const int32_t* e_slot, const int64_t* e_off, const int32_t* e_len,
                       const int32_t* e_bnum, const int32_t* e_bcoord, const int32_t* cp_slot, int64_t out_base,
                       int32_t flags, uint8_t* out, int64_t cap_bytes, int32_t cap_entries, uint8_t* verdict,
                       int32_t* k_src, int32_t* k_gidx, int32_t* k_slot, int32_t* k_bnum, int32_t* k_bcoord,
                       int64_t* k_off, int32_t* k_len, gpx_journal_gc_counts* counts) {
  const JgArgs a{n,       in,     in_bytes, in_base,   e_gidx,      e_slot,  e_off,  e_len,  e_bnum,
                 e_bcoord, cp_slot, out_base, flags,     out,         cap_bytes, cap_entries, verdict, k_src,
                 k_gidx,  k_slot, k_bnum,   k_bcoord,  k_off,       k_len,   counts};
  int rc = jg_args(h, a);
  if (rc != GPX_OK) return rc;
  if ((rc = jg_open(h)) != GPX_OK) return rc;
  return jg_run(h, a, in, 0, in_bytes, 0, nullptr);
}

} /* extern "C" */
