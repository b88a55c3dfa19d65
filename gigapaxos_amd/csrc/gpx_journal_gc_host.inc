// Host-pointer side of the journal compaction (include/gpx_journal_gc.h), staged through CtlStage around jg_run.
// Needs: gpx_host_stage.inc (CtlStage), jg_args / jg_open / jg_run (gpx_journal_gc_dev.inc).

extern "C" {

/* Two passes, so that a dead or an untouched file costs its rows only.
 * Pass 1 sends the rows alone (counts only, no `in`) and gets the counts and the verdicts back.  The length prefix of
 * every row whose range checked out is then compared here, on the host: the row turns GPX_JG_BAD and the counts move as
 * the _dev form's prefix test would have moved them.  If nothing is kept, if GPX_JG_COUNT_ONLY is set or
 * GPX_JG_SKIP_UNCHANGED applies, that is the call: no file byte has crossed the link.
 * Pass 2 first finds the done prefix of the kept rows (both caps, a host loop over the verdicts and lengths), then goes
 * over those rows in chunks of consecutive rows.  A chunk's kept entries lie inside one window of the caller's block of
 * at most jr_stage_max bytes (64 MiB; GPX_TEST_JOURNAL_STAGE when the scratch is made: tests) - or it is one kept row,
 * whose entry may be larger - and only that window is copied in.  The device gets the first pass' verdicts with the
 * chunk and judges nothing again: group state that moves between the passes cannot make the two disagree.  Positions
 * are carried from chunk to chunk; a chunk's caps are exactly what its done rows need. */
int gpx_journal_gc(gpx_engine* h, int32_t n, const uint8_t* in, int64_t in_bytes, int64_t in_base,
                   const int32_t* e_gidx, const int32_t* e_slot, const int64_t* e_off, const int32_t* e_len,
                   const int32_t* e_bnum, const int32_t* e_bcoord, const int32_t* cp_slot, int64_t out_base,
                   int32_t flags, uint8_t* out, int64_t cap_bytes, int32_t cap_entries, uint8_t* verdict, int32_t* k_src,
                   int32_t* k_gidx, int32_t* k_slot, int32_t* k_bnum, int32_t* k_bcoord, int64_t* k_off, int32_t* k_len,
                   gpx_journal_gc_counts* counts) {
  const JgArgs a{n,       in,     in_bytes, in_base,   e_gidx,      e_slot,  e_off,  e_len,  e_bnum,
                 e_bcoord, cp_slot, out_base, flags,     out,         cap_bytes, cap_entries, verdict, k_src,
                 k_gidx,  k_slot, k_bnum,   k_bcoord,  k_off,       k_len,   counts};
  int rc = jg_args(h, a);
  if (rc != GPX_OK) return rc;
  if ((rc = jg_open(h)) != GPX_OK) return rc;
  const size_t nn = (size_t)n;
  std::vector<uint8_t> ver(nn);
  gpx_journal_gc_counts tot;
  { /* pass 1 */
    CtlStage t(h);
    JgArgs c = a;
    c.in = nullptr, c.flags = GPX_JG_COUNT_ONLY, c.out = nullptr, c.cap_bytes = 0, c.cap_entries = 0;
    c.k_src = c.k_gidx = c.k_slot = c.k_bnum = c.k_bcoord = c.k_len = nullptr, c.k_off = nullptr;
    c.e_gidx = t.in(e_gidx, nn), c.e_slot = t.in(e_slot, nn), c.e_off = t.in(e_off, nn), c.e_len = t.in(e_len, nn);
    c.e_bnum = c.e_bcoord = nullptr;
    c.cp_slot = t.in_opt(cp_slot, nn);
    c.verdict = t.tmp<uint8_t>(nn, false);
    c.counts = (gpx_journal_gc_counts*)h->jg_counts;
    if (t.ready()) return t.rc;
    if (t.ran(jg_run(h, c, nullptr, 0, in_bytes, 0, nullptr))) return t.rc;
    t.d2h(&tot, h->jg_counts, sizeof(tot));
    if (n) t.d2h(ver.data(), c.verdict, nn);
    if (t.sync()) return t.rc;
  }
  if (in) /* the prefix test of the _dev form: the range of these rows lies inside [0, in_bytes) */
    for (size_t i = 0; i < nn; i++) {
      if (ver[i] == GPX_JG_BAD) continue;
      const uint8_t* p = in + (e_off[i] - in_base);
      const uint32_t u = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
      if (u == (uint32_t)e_len[i]) continue;
      const int64_t v = 4 + (int64_t)e_len[i];
      tot.n_usable--, tot.n_bad++, tot.named_bytes -= v, tot.unchanged = 0;
      if (ver[i] != GPX_JG_DROP) tot.n_keep--, tot.keep_bytes -= v;
      if (ver[i] == GPX_JG_KEEP_UNJUDGED) tot.n_unjudged--;
      ver[i] = GPX_JG_BAD;
    }
  if (verdict && n) memcpy(verdict, ver.data(), nn);
  if (tot.n_keep == 0 || (flags & GPX_JG_COUNT_ONLY) || ((flags & GPX_JG_SKIP_UNCHANGED) && tot.unchanged)) {
    *counts = tot;
    return GPX_OK;
  }
  /* the done prefix of the kept rows: rows [0, end_row) hold all of them */
  auto kept = [&](size_t i) { return ver[i] == GPX_JG_KEEP || ver[i] == GPX_JG_KEEP_UNJUDGED; };
  size_t end_row = 0;
  {
    int64_t pos = 0;
    int32_t e = 0;
    for (size_t i = 0; i < nn; i++) {
      if (!kept(i)) continue;
      const int64_t v = 4 + (int64_t)e_len[i];
      if (e >= cap_entries || pos + v > cap_bytes) break;
      e++, pos += v, end_row = i + 1;
    }
  }
  const int64_t bound = (int64_t)h->jr_stage_max;
  for (size_t i0 = 0; i0 < end_row;) {
    /* rows [i0, i1): the window [lo, hi) of their kept entries, the bytes and rows those need */
    int64_t lo = INT64_MAX, hi = 0, need = 0;
    size_t i1 = i0, kc = 0;
    for (; i1 < end_row; i1++) {
      if (!kept(i1)) continue;
      const int64_t s = e_off[i1] - in_base, v = 4 + (int64_t)e_len[i1];
      const int64_t nlo = std::min(lo, s), nhi = std::max(hi, s + v);
      if (kc > 0 && nhi - nlo > bound) break;
      lo = nlo, hi = nhi, need += v, kc++;
    }
    if (kc == 0) break; /* end_row is behind a kept row: not reached */
    const size_t m = i1 - i0;
    CtlStage t(h);
    JgArgs c = a;
    c.n = (int32_t)m;
    c.e_gidx = t.in(e_gidx + i0, m), c.e_slot = t.in(e_slot + i0, m), c.e_off = t.in(e_off + i0, m);
    c.e_len = t.in(e_len + i0, m);
    c.e_bnum = k_bnum ? t.in(e_bnum + i0, m) : nullptr;
    c.e_bcoord = k_bcoord ? t.in(e_bcoord + i0, m) : nullptr;
    c.cp_slot = nullptr;
    const uint8_t* force = t.in(ver.data() + i0, m);
    /* the window, its first byte at a 256-byte boundary, rounded up to whole 16-byte words */
    uint8_t* d_in = (uint8_t*)t.tmp_bytes(((size_t)(hi - lo) + 15) & ~(size_t)15, 1, false);
    c.out_base = out_base + tot.bytes_done;
    c.flags = 0, c.in_bytes = hi - lo;
    c.cap_bytes = need, c.cap_entries = (int32_t)kc;
    c.out = (uint8_t*)t.tmp_bytes((size_t)need, 1, false);
    c.verdict = nullptr;
    c.k_src = k_src ? t.tmp<int32_t>(kc, false) : nullptr;
    c.k_gidx = k_gidx ? t.tmp<int32_t>(kc, false) : nullptr;
    c.k_slot = k_slot ? t.tmp<int32_t>(kc, false) : nullptr;
    c.k_bnum = k_bnum ? t.tmp<int32_t>(kc, false) : nullptr;
    c.k_bcoord = k_bcoord ? t.tmp<int32_t>(kc, false) : nullptr;
    c.k_off = t.tmp<int64_t>(kc, false);
    c.k_len = t.tmp<int32_t>(kc, false);
    c.counts = (gpx_journal_gc_counts*)h->jg_counts;
    t.h2d(d_in, in + lo, (size_t)(hi - lo));
    if (t.ready()) return t.rc;
    if (t.ran(jg_run(h, c, d_in, lo, hi, (int32_t)i0, force))) return t.rc;
    gpx_journal_gc_counts cc;
    t.d2h(&cc, h->jg_counts, sizeof(cc));
    if (t.sync()) return t.rc;
    if (cc.n_done != (int32_t)kc || cc.bytes_done != need) { /* the device counted other rows than the host */
      snprintf(g_err, sizeof(g_err), "gpx_journal_gc: a chunk of %zu kept rows, %lld bytes came back as %d rows, %lld bytes",
               kc, (long long)need, cc.n_done, (long long)cc.bytes_done);
      return GPX_EDEVICE;
    }
    const size_t r0 = (size_t)tot.n_done;
    if (k_src) t.d2h(k_src + r0, c.k_src, kc * 4);
    if (k_gidx) t.d2h(k_gidx + r0, c.k_gidx, kc * 4);
    if (k_slot) t.d2h(k_slot + r0, c.k_slot, kc * 4);
    if (k_bnum) t.d2h(k_bnum + r0, c.k_bnum, kc * 4);
    if (k_bcoord) t.d2h(k_bcoord + r0, c.k_bcoord, kc * 4);
    t.d2h(k_off + r0, c.k_off, kc * 8);
    t.d2h(k_len + r0, c.k_len, kc * 4);
    t.d2h(out + tot.bytes_done, c.out, (size_t)need);
    if (t.sync()) return t.rc;
    tot.n_done += cc.n_done, tot.bytes_done += cc.bytes_done, tot.n_runs_done += cc.n_runs_done;
    i0 = i1;
  }
  *counts = tot;
  return GPX_OK;
}

} /* extern "C" */
