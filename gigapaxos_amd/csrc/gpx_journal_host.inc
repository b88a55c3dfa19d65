// Host-pointer side of the journal batches (include/gpx_journal.h), staged through CtlStage around jr_run.
// Needs: gpx_host_stage.inc (CtlStage), jr_args / jr_open / jr_run (gpx_journal_dev.inc).

extern "C" {

/* The call goes through in chunks of consecutive records.  A chunk's usable frames lie inside one window of the
 * caller's block of at most jr_stage_max bytes (64 MiB; GPX_TEST_JOURNAL_STAGE when the scratch is made: tests) - or it
 * is one record, whose frame may be larger - and only that window is copied in.  Finding the chunks is a host loop over
 * the records' frame ranges: indices and offsets, no frame byte.  Per chunk the counts come back first (they size the
 * copies), then the done rows and bytes with one wait.  Entry positions, record numbers and what is left of the caps are
 * carried from chunk to chunk; once a cap has cut, the later chunks only count. */
int gpx_journal_pack(gpx_engine* h, int32_t n, const uint8_t* frames, int64_t frames_bytes, int32_t n_frames,
                     const int64_t* frame_off, const int32_t* frame_len, const int32_t* rec_frame, const int32_t* gidx,
                     const int32_t* slot, const int32_t* bnum, const int32_t* bcoord, const uint8_t* r_flags,
                     const uint8_t* status, int64_t base_offset, int32_t flags, uint8_t* out, int64_t cap_bytes,
                     int32_t cap_entries, int32_t* e_rec, int32_t* e_gidx, int32_t* e_slot, int32_t* e_bnum,
                     int32_t* e_bcoord, int64_t* e_off, int32_t* e_len, gpx_journal_counts* counts) {
  const JrArgs a{n,       frames,  frames_bytes, n_frames,  frame_off,   frame_len, rec_frame, gidx,   slot,
                 bnum,    bcoord,  r_flags,      status,    base_offset, flags,     out,       cap_bytes, cap_entries,
                 e_rec,   e_gidx,  e_slot,       e_bnum,    e_bcoord,    e_off,     e_len,     counts};
  int rc = jr_args(h, a);
  if (rc != GPX_OK) return rc;
  if ((rc = jr_open(h)) != GPX_OK) return rc;
  const bool count_only = (flags & GPX_JR_COUNT_ONLY) != 0;
  const int64_t bound = (int64_t)h->jr_stage_max;
  const size_t n_off = (size_t)n_frames + (frame_len ? 0 : 1);
  gpx_journal_counts tot = {0, 0, 0, 0, 0, 0};
  bool cut = false;
  for (int64_t i0 = 0; i0 < n;) {
    /* records [i0, i1): the window [lo, hi) of their usable frames (jr_eval's test), the bytes their entries need */
    int64_t lo = INT64_MAX, hi = 0, need = 0, i1 = i0;
    for (; i1 < n; i1++) {
      const int64_t f = rec_frame ? (int64_t)rec_frame[i1] : i1;
      if (f < 0 || f >= n_frames) continue;
      const int64_t s = frame_off[f];
      if (s < 0) continue;
      const int64_t L = frame_len ? (int64_t)frame_len[f] : (frame_off[f + 1] < s ? -1 : frame_off[f + 1] - s);
      if (L < 0 || L > GPX_JR_MAX_LEN || s > frames_bytes - L) continue;
      const int64_t nlo = std::min(lo, s), nhi = std::max(hi, s + L);
      if (i1 > i0 && nhi - nlo > bound) break;
      lo = nlo, hi = nhi, need += 4 + L;
    }
    if (lo > hi) lo = hi = 0; /* no usable frame: an empty window */
    const int32_t m = (int32_t)(i1 - i0);
    const bool pack = !count_only && !cut;
    const int64_t capb = pack ? std::min(cap_bytes - tot.bytes_done, need) : 0;
    const int32_t cape = pack && capb >= 4 ? (int32_t)std::min<int64_t>((int64_t)cap_entries - tot.n_done, m) : 0;
    CtlStage t(h);
    const size_t mm = (size_t)m, ce = (size_t)cape;
    JrArgs c = a;
    c.n = m;
    c.frame_off = t.in(frame_off, n_off);
    c.frame_len = t.in_opt(frame_len, (size_t)n_frames);
    c.rec_frame = rec_frame ? t.in(rec_frame + i0, mm) : nullptr;
    c.gidx = gidx ? t.in(gidx + i0, mm) : nullptr;
    c.slot = slot ? t.in(slot + i0, mm) : nullptr;
    c.bnum = bnum ? t.in(bnum + i0, mm) : nullptr;
    c.bcoord = bcoord ? t.in(bcoord + i0, mm) : nullptr;
    c.r_flags = t.in(r_flags + i0, mm);
    c.status = t.in(status + i0, mm);
    /* the window, its first byte at a 256-byte boundary; k_jr_copy may read the whole aligned word of the last byte */
    uint8_t* d_fr = (uint8_t*)t.tmp_bytes((size_t)(hi - lo) + 4, 1, false);
    c.base_offset = base_offset + tot.n_bytes; /* == bytes_done as long as nothing is cut */
    c.flags = pack ? 0 : GPX_JR_COUNT_ONLY;
    c.cap_bytes = capb, c.cap_entries = cape;
    c.out = cape ? (uint8_t*)t.tmp_bytes((size_t)capb, 1, false) : nullptr;
    c.e_rec = cape && e_rec ? t.tmp<int32_t>(ce, false) : nullptr;
    c.e_gidx = cape && e_gidx ? t.tmp<int32_t>(ce, false) : nullptr;
    c.e_slot = cape && e_slot ? t.tmp<int32_t>(ce, false) : nullptr;
    c.e_bnum = cape && e_bnum ? t.tmp<int32_t>(ce, false) : nullptr;
    c.e_bcoord = cape && e_bcoord ? t.tmp<int32_t>(ce, false) : nullptr;
    c.e_off = cape ? t.tmp<int64_t>(ce, false) : nullptr;
    c.e_len = cape ? t.tmp<int32_t>(ce, false) : nullptr;
    c.counts = (gpx_journal_counts*)h->jr_counts;
    if (hi > lo) t.h2d(d_fr, frames + lo, (size_t)(hi - lo));
    if (t.ready()) return t.rc;
    if (t.ran(jr_run(h, c, d_fr, lo, hi, (int32_t)i0))) return t.rc;
    gpx_journal_counts cc;
    t.d2h(&cc, h->jr_counts, sizeof(cc));
    if (t.sync()) return t.rc;
    if (cc.n_done > 0) {
      const size_t k = (size_t)cc.n_done, r0 = (size_t)tot.n_done;
      if (e_rec) t.d2h(e_rec + r0, c.e_rec, k * 4);
      if (e_gidx) t.d2h(e_gidx + r0, c.e_gidx, k * 4);
      if (e_slot) t.d2h(e_slot + r0, c.e_slot, k * 4);
      if (e_bnum) t.d2h(e_bnum + r0, c.e_bnum, k * 4);
      if (e_bcoord) t.d2h(e_bcoord + r0, c.e_bcoord, k * 4);
      t.d2h(e_off + r0, c.e_off, k * 8);
      t.d2h(e_len + r0, c.e_len, k * 4);
      t.d2h(out + tot.bytes_done, c.out, (size_t)cc.bytes_done);
      if (t.sync()) return t.rc;
    }
    tot.n_entries += cc.n_entries, tot.n_bad += cc.n_bad, tot.n_bytes += cc.n_bytes;
    tot.n_done += cc.n_done, tot.bytes_done += cc.bytes_done;
    cut = cut || cc.n_done < cc.n_entries;
    i0 = i1;
  }
  *counts = tot;
  return GPX_OK;
}

} /* extern "C" */
