// Device-pointer side of the journal batches (include/gpx_journal.h; kernels in gpx_journal.hip.h): the scratch, the
// argument checks, gpx_journal_pack_dev and the engine-free gpx_journal_walk; the host-pointer twin:
// gpx_journal_host.inc.
// Needs: the engine and the kernels of gpx_engine.hip.

namespace {

static_assert(GPX_JR_COUNT_ONLY == GPX_JR_COUNT_ONLY_, "include/gpx_journal.h and gpx_journal.hip.h disagree on the flag");
static_assert(sizeof(gpx_journal_counts) == 32 && sizeof(JrCounts) == 32, "gpx_journal_counts is 32 bytes");
static_assert(GPX_JR_TILE == GPX_BLOCK && GPX_JR_SPAN == GPX_BLOCK, "one record, one descriptor per lane");
static_assert(GPX_JR_CTILE % (16 * GPX_BLOCK) == 0, "an output tile is whole passes of 16-byte chunks");

/* the arguments of one call, as both forms take them */
struct JrArgs {
  int32_t n;
  const uint8_t* frames;
  int64_t frames_bytes;
  int32_t n_frames;
  const int64_t* frame_off;
  const int32_t *frame_len, *rec_frame, *gidx, *slot, *bnum, *bcoord;
  const uint8_t *r_flags, *status;
  int64_t base_offset;
  int32_t flags;
  uint8_t* out;
  int64_t cap_bytes;
  int32_t cap_entries;
  int32_t *e_rec, *e_gidx, *e_slot, *e_bnum, *e_bcoord;
  int64_t* e_off;
  int32_t* e_len;
  gpx_journal_counts* counts;
};

/* what a journal call checks before it does anything else; of the handle only cfg.max_batch is read */
int jr_args(const gpx_engine* h, const JrArgs& a) {
  if (!h || !a.counts || a.n < 0 || a.n_frames < 0 || a.frames_bytes < 0 || a.cap_bytes < 0 || a.cap_entries < 0 ||
      (a.flags & ~GPX_JR_COUNT_ONLY))
    return GPX_EINVAL;
  if (a.n > 0) {
    if (!a.frame_off || !a.r_flags || !a.status || (a.frames_bytes > 0 && !a.frames)) return GPX_EINVAL;
    if (!(a.flags & GPX_JR_COUNT_ONLY) && (!a.gidx || !a.slot || !a.bnum || !a.bcoord || !a.out || !a.e_off || !a.e_len))
      return GPX_EINVAL;
  }
  if (!(a.flags & GPX_JR_COUNT_ONLY) && ((uintptr_t)a.out & 15)) return GPX_EINVAL;
  if (a.n > h->cfg.max_batch) return GPX_ECAPACITY;
  return GPX_OK;
}

/* The per-tile words, the descriptors of max_batch entries and the host twin's counts: ONE block, allocated by the first
 * call.  All of it is scratch of which a call reads only what it wrote: not zeroed.  A failed allocation leaves nothing
 * behind and the engine usable. */
int jr_init(gpx_engine* e) {
  if (e->jr_counts) return GPX_OK;
  const size_t N = (size_t)std::max(e->cfg.max_batch, 1);
  const size_t tiles = (N + GPX_JR_TILE - 1) / GPX_JR_TILE;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t b_t4 = up(tiles * 4), b_t8 = up(tiles * 8), b_d8 = up(N * 8), b_d4 = up(N * 4);
  char* base = nullptr;
  int rc = dev_alloc(e, &base, 3 * b_t4 + 2 * b_t8 + 2 * b_d8 + b_d4 + 256, false);
  if (rc != GPX_OK) return rc;
  if (const char* sv = getenv("GPX_TEST_JOURNAL_STAGE")) { /* tests: the host twin's chunks */
    const long long v = atoll(sv);
    if (v > 0) e->jr_stage_max = (size_t)v;
  }
  JrMem& M = e->jr;
  char* p = base;
  M.tile_bytes = (long long*)p, p += b_t8;
  M.tile_boff = (long long*)p, p += b_t8;
  M.d_pos = (long long*)p, p += b_d8;
  M.d_src = (long long*)p, p += b_d8;
  M.d_len = (int32_t*)p, p += b_d4;
  M.tile_cnt = (int32_t*)p, p += b_t4;
  M.tile_bad = (int32_t*)p, p += b_t4;
  M.tile_eoff = (int32_t*)p, p += b_t4;
  e->jr_counts = (JrCounts*)p; /* last: the marker */
  return GPX_OK;
}

/* what the call needs of the engine: one an exchange kernel gave up on is refused; the scratch */
int jr_open(gpx_engine* h) {
  int rc = check_batch(h, 0);
  if (rc != GPX_OK) return rc;
  return jr_init(h);
}

/* The launches (gpx_journal.hip.h) on the back-end stream.  `frames` is device memory that holds bytes [win_lo, win_hi)
 * of the caller's block, and a frame outside that range is refused: the _dev form passes its block and
 * [0, frames_bytes), the host twin the window it staged (the union of the usable frames of its records).  Record i is
 * record rec_base + i of the caller's call. */
int jr_run(gpx_engine* h, const JrArgs& a, const uint8_t* frames, int64_t win_lo, int64_t win_hi, int32_t rec_base) {
  h->stream = h->sB;
  JrIn I;
  I.frames = frames, I.win_lo = win_lo, I.win_hi = win_hi, I.n_frames = a.n_frames;
  I.frame_off = (const long long*)a.frame_off, I.frame_len = a.frame_len, I.rec_frame = a.rec_frame;
  I.gidx = a.gidx, I.slot = a.slot, I.bnum = a.bnum, I.bcoord = a.bcoord, I.r_flags = a.r_flags, I.status = a.status;
  I.n = a.n, I.rec_base = rec_base;
  const JrOut O{a.out, (long long)a.cap_bytes, (long long)a.base_offset, a.cap_entries, a.e_rec, a.e_gidx, a.e_slot,
                a.e_bnum, a.e_bcoord, (long long*)a.e_off, a.e_len};
  JrCounts* counts = (JrCounts*)a.counts;
  const int ntiles = (int)(((int64_t)a.n + GPX_JR_TILE - 1) / GPX_JR_TILE);
  if (ntiles) LAUNCH(h, "k_jr_tile", k_jr_tile, ntiles, I, h->jr);
  LAUNCH(h, "k_jr_offsets", k_jr_offsets, 1, (int32_t)ntiles, I, h->jr, (long long)a.cap_bytes, a.cap_entries, a.flags, counts);
  /* an entry is at least 4 bytes: below that nothing can be done */
  if (ntiles && !(a.flags & GPX_JR_COUNT_ONLY) && a.cap_entries > 0 && a.cap_bytes >= 4) {
    LAUNCH(h, "k_jr_rows", k_jr_rows, ntiles, I, h->jr, O, (const JrCounts*)counts);
    /* copy: persistent workgroups over the 16 KB tiles of what fits cap_bytes (bytes_done is still on the device;
     * records may share a frame, so the frame block bounds nothing): eight per CU of the chip's 256, as k_acc_copy */
    const int64_t tiles = a.cap_bytes / GPX_JR_CTILE + 1;
    LAUNCH(h, "k_jr_copy", k_jr_copy, (int)std::min<int64_t>(tiles, 2048), frames, h->jr, a.out, (const JrCounts*)counts);
  }
  HIPCHK(hipGetLastError());
  return GPX_OK;
}

}  // namespace

extern "C" {

int gpx_journal_walk(const uint8_t* buf, int64_t bytes, int64_t base_offset, int32_t cap, int64_t* e_off, int32_t* e_len,
                     int32_t* n_entries, int64_t* good_bytes) {
  if (bytes < 0 || cap < 0 || (bytes > 0 && !buf) || !n_entries || !good_bytes || (cap > 0 && (!e_off || !e_len)))
    return GPX_EINVAL;
  int64_t pos = 0;
  int32_t k = 0;
  while (bytes - pos >= 4 && k < INT32_MAX) {
    const uint32_t u = (uint32_t)buf[pos] << 24 | (uint32_t)buf[pos + 1] << 16 | (uint32_t)buf[pos + 2] << 8 | buf[pos + 3];
    const int32_t len = (int32_t)u; /* readInt() */
    if (len < 0 || (int64_t)len > bytes - pos - 4) break;
    if (k < cap) e_off[k] = base_offset + pos, e_len[k] = len;
    k++;
    pos += 4 + (int64_t)len;
  }
  *n_entries = k;
  *good_bytes = pos;
  return GPX_OK;
}

int gpx_journal_pack_dev(gpx_engine* h, int32_t n, const uint8_t* frames, int64_t frames_bytes, int32_t n_frames,
                         const int64_t* frame_off, const int32_t* frame_len, const int32_t* rec_frame,
                         const int32_t* gidx, const int32_t* slot, const int32_t* bnum, const int32_t* bcoord,
                         const uint8_t* r_flags, const uint8_t* status, int64_t base_offset, int32_t flags, uint8_t* out,
                         int64_t cap_bytes, int32_t cap_entries, int32_t* e_rec, int32_t* e_gidx, int32_t* e_slot,
                         int32_t* e_bnum, int32_t* e_bcoord, int64_t* e_off, int32_t* e_len, gpx_journal_counts* counts) {
  const JrArgs a{n,       frames,  frames_bytes, n_frames,  frame_off,   frame_len, rec_frame, gidx,   slot,
                 bnum,    bcoord,  r_flags,      status,    base_offset, flags,     out,       cap_bytes, cap_entries,
                 e_rec,   e_gidx,  e_slot,       e_bnum,    e_bcoord,    e_off,     e_len,     counts};
  int rc = jr_args(h, a);
  if (rc != GPX_OK) return rc;
  if ((rc = jr_open(h)) != GPX_OK) return rc;
  return jr_run(h, a, frames, 0, frames_bytes, 0);
}

} /* extern "C" */
