// Lockstep CPU emulation of the kernels of gigapaxos_amd/csrc/gpx_logindex.hip.h (tests/test_logindex_abi.py compiles
// and runs this with AddressSanitizer): the real header, unmodified, on top of the real gpx_compact.hip.h.  One
// std::thread per lane of a workgroup, one workgroup at a time (tests/lockstep_runtime.h).  Every buffer is a heap block
// of its exact size, the scratch starts as garbage and every output carries a sentinel, so an index past an end is a
// sanitizer report and an entry written beyond what is done a failure.  The launches and their conditions are those of
// gpx_logindex_dev.inc.  The expected answer is a plain loop over per-group vectors that restates LogIndex.java next
// to the table's row order.  The case list is that of tests/test_logindex_gpu.py (tests/logindex_model.py).  What this
// cannot show is what only the GPU has: the compiler's code and memory ordering between launches.
#include <algorithm>
#include <barrier>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "lockstep_runtime.h"

static uint32_t atomicMin(uint32_t* p, uint32_t v) {
  uint32_t o = __atomic_load_n(p, __ATOMIC_SEQ_CST);
  while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
  return o;
}
static int32_t atomicMin(int32_t* p, int32_t v) {
  int32_t o = __atomic_load_n(p, __ATOMIC_SEQ_CST);
  while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
  return o;
}
static int32_t atomicCAS(int32_t* p, int32_t cmp, int32_t v) {
  __atomic_compare_exchange_n(p, &cmp, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST);
  return cmp;
}

#include "gpx_compact.hip.h"
#include "gpx_logindex.hip.h"

static void fail(const std::string& what, const char* msg, long long a = 0, long long b = 0) {
  printf("%s: %s (%lld, %lld)\n", what.c_str(), msg, a, b);
  exit(1);
}
static int tiles_for(long long n) { return (int)((n + GPX_LI_TILE - 1) / GPX_LI_TILE); }
static int32_t wdiff(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }

#define SENT 0x5A
template <class T> static T* out_blk(size_t n) { return blk<T>(n, SENT); }
template <class T> static bool sent_from(const T* p, size_t from, size_t n) {
  const uint8_t* b = (const uint8_t*)p;
  for (size_t q = from * sizeof(T); q < n * sizeof(T); q++)
    if (b[q] != SENT) return false;
  return true;
}
template <class T> static T* in_blk(const std::vector<T>& v) {
  T* p = (T*)malloc(std::max<size_t>(v.size(), 1) * sizeof(T));
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

struct Entry {
  int32_t g, slot, bnum, bcoord, file;
  long long off;
  int32_t len;
  bool alive;
};

/* the expected side: the table as a vector in append order, LogIndex's per-group words beside it */
struct Ref {
  int32_t G, cap, gen = 0;
  std::vector<Entry> rows;
  std::vector<int32_t> gc, min_file;
  Ref(int32_t G_, int32_t cap_) : G(G_), cap(cap_), gc(G_, -1), min_file(G_, -1) {}
  int32_t alive() const {
    int32_t a = 0;
    for (const Entry& e : rows) a += e.alive;
    return a;
  }
};

/* the engine side: exact-size blocks, garbage in the scratch */
struct Dev {
  LiMem M{};
  long long ub = 0;
  int32_t max_batch;
  std::vector<void*> blocks;
  template <class T> T* get(size_t n, int fill) {
    T* p = blk<T>(n, fill);
    blocks.push_back(p);
    return p;
  }
  Dev(int32_t G, int32_t cap, int32_t batch) : max_batch(batch) {
    const size_t R = cap, tiles = tiles_for(std::max({cap, G, batch})), rt = tiles_for(batch);
    const size_t park = (size_t)tiles_for(std::max(cap, batch)) * GPX_LI_TILE;
    M.cap_rows = cap, M.G = G;
    for (LiCols* c : {&M.T, &M.U}) {
      c->gidx = get<int32_t>(R, 0x77), c->slot = get<int32_t>(R, 0x77), c->bnum = get<int32_t>(R, 0x77);
      c->bcoord = get<int32_t>(R, 0x77), c->file = get<int32_t>(R, 0x77), c->off = get<long long>(R, 0x77);
      c->len = get<int32_t>(R, 0x77), c->alive = get<uint8_t>(R, 0x77);
    }
    M.gc = get<int32_t>(G, 0xff), M.min_file = get<int32_t>(G, 0xff);
    M.arm = get<uint32_t>(G, 0xff), M.first = get<uint32_t>(G, 0xff);
    M.hdr = get<int32_t>(LI_HDR_WORDS, 0);
    M.park = get<int32_t>(park, 0x77);
    M.tile_cnt = get<int32_t>(tiles, 0x77), M.tile_off = get<int32_t>(tiles, 0x77);
    M.rt_a = get<int32_t>(rt, 0x77), M.rt_b = get<int32_t>(rt, 0x77), M.rt_c = get<int32_t>(rt, 0x77);
  }
  ~Dev() {
    for (void* p : blocks) free(p);
  }
  int row_tiles() const { return tiles_for(ub); }
};

struct Sys {
  Ref R;
  Dev D;
  int checks = 0;
  Sys(int32_t G, int32_t cap, int32_t batch) : R(G, cap), D(G, cap, batch) {}

  void counts_are(const std::string& w, const LiCounts& c, int32_t done, int32_t hits, int32_t stale, int32_t nog, int32_t rep) {
    const int32_t want[8] = {(int32_t)R.rows.size(), R.alive(), R.gen, done, hits, stale, nog, rep};
    const int32_t got[8] = {c.n_rows, c.n_alive, c.generation, c.n_done, c.n_hits, c.n_stale, c.n_nogroup, c.n_repeat};
    for (int k = 0; k < 8; k++)
      if (want[k] != got[k]) fail(w, "counts field", k, got[k]);
  }
  /* the table, the per-group words and the idle arming words, after every call */
  void state_is(const std::string& w) {
    const LiMem& M = D.M;
    if (M.hdr[LI_ROWS] != (int32_t)R.rows.size() || M.hdr[LI_ALIVE] != R.alive() || M.hdr[LI_GEN] != R.gen)
      fail(w, "header", M.hdr[LI_ROWS], M.hdr[LI_ALIVE]);
    for (size_t r = 0; r < R.rows.size(); r++) {
      const Entry& e = R.rows[r];
      if ((M.T.alive[r] != 0) != e.alive) fail(w, "alive", (long long)r);
      if (M.T.gidx[r] != e.g || M.T.slot[r] != e.slot || M.T.bnum[r] != e.bnum || M.T.bcoord[r] != e.bcoord ||
          M.T.file[r] != e.file || M.T.off[r] != e.off || M.T.len[r] != e.len)
        fail(w, "row", (long long)r);
    }
    for (int32_t g = 0; g < R.G; g++) {
      if (M.gc[g] != R.gc[g]) fail(w, "gc", g, M.gc[g]);
      if (M.min_file[g] != R.min_file[g]) fail(w, "min file", g, M.min_file[g]);
      if (M.arm[g] != GPX_LI_IDLE || M.first[g] != GPX_LI_IDLE) fail(w, "an arming word left set", g);
    }
    printf("%s: ok\n", w.c_str());
    checks++;
  }

  /* ---- add ---- */
  void add(const std::string& w, const std::vector<int32_t>& g, const std::vector<int32_t>& s, int32_t file,
           const int32_t* n_dev_val = nullptr) {
    const int32_t n = (int32_t)g.size();
    std::vector<int32_t> bn(n), bc(n), ln(n);
    std::vector<long long> off(n);
    for (int32_t i = 0; i < n; i++) bn[i] = i % 3, bc[i] = 100 + i % 2, ln[i] = 1 + i % 37, off[i] = 1000 + 41ll * i;
    const int32_t m = n_dev_val ? std::min(n, std::max(*n_dev_val, 0)) : n;
    std::vector<uint8_t> want(m);
    int32_t done = 0, stale = 0, nog = 0;
    for (int32_t i = 0; i < m; i++) {
      if (g[i] < 0 || g[i] >= R.G) want[i] = GPX_LI_NOGROUP_, nog++;
      else if (wdiff(s[i], R.gc[g[i]]) <= 0) want[i] = GPX_LI_STALE_, stale++;
      else if ((int32_t)R.rows.size() >= R.cap) want[i] = GPX_LI_FULL_;
      else {
        want[i] = GPX_LI_ADDED_, done++;
        R.rows.push_back(Entry{g[i], s[i], bn[i], bc[i], file, off[i], ln[i], true});
        if (R.min_file[g[i]] == -1) R.min_file[g[i]] = file;
      }
    }
    int32_t *dg = in_blk(g), *ds = in_blk(s), *dbn = in_blk(bn), *dbc = in_blk(bc), *dl = in_blk(ln);
    long long* doff = in_blk(off);
    int32_t* dn = n_dev_val ? in_blk(std::vector<int32_t>{*n_dev_val}) : nullptr;
    uint8_t* st = out_blk<uint8_t>(n);
    LiCounts* c = out_blk<LiCounts>(1);
    const int nt = tiles_for(n);
    const LiMem M = D.M;
    if (nt) launch(nt, [=] { k_li_add_tile(M, n, dn, dg, ds, st); });
    launch(1, [=] { k_li_add_offsets(nt, M, c); });
    const LiRowsIn I{dg, ds, dbn, dbc, doff, dl};
    if (nt) launch(nt, [=] { k_li_add_move(M, I, file, st); });
    D.ub = std::min<long long>(M.cap_rows, D.ub + n);
    counts_are(w, *c, done, 0, stale, nog, 0);
    for (int32_t i = 0; i < m; i++)
      if (st[i] != want[i]) fail(w, "status", i, st[i]);
    if (!sent_from(st, m, n)) fail(w, "a status beyond the records taken");
    state_is(w);
    for (void* p : {(void*)dg, (void*)ds, (void*)dbn, (void*)dbc, (void*)dl, (void*)doff, (void*)dn, (void*)st, (void*)c}) free(p);
  }

  /* the first record of each group and the status of every record */
  std::vector<int32_t> firsts(const std::vector<int32_t>& g, std::vector<uint8_t>& st, int32_t& nog, int32_t& rep) {
    std::vector<int32_t> rec(R.G, -1);
    st.assign(g.size(), GPX_LI_ADDED_);
    nog = rep = 0;
    for (size_t i = 0; i < g.size(); i++) {
      if (g[i] < 0 || g[i] >= R.G) st[i] = GPX_LI_NOGROUP_, nog++;
      else if (rec[g[i]] >= 0) st[i] = GPX_LI_REPEAT_, rep++;
      else rec[g[i]] = (int32_t)i;
    }
    return rec;
  }

  /* ---- set_gc ---- */
  void set_gc(const std::string& w, const std::vector<int32_t>& g, const std::vector<int32_t>& gc, int32_t flags = 0) {
    const int32_t n = (int32_t)g.size();
    std::vector<uint8_t> want;
    int32_t nog, rep, died = 0, applied = 0;
    const std::vector<int32_t> rec = firsts(g, want, nog, rep);
    const bool reset = flags & GPX_LI_RESET_;
    for (int32_t q = 0; q < R.G; q++)
      if (rec[q] >= 0) R.gc[q] = reset ? -1 : gc[rec[q]], applied++;
    for (Entry& e : R.rows)
      if (e.alive && rec[e.g] >= 0 && (reset || wdiff(e.slot, R.gc[e.g]) <= 0)) e.alive = false, died++;
    for (int32_t q = 0; q < R.G; q++)
      if (rec[q] >= 0) {
        R.min_file[q] = -1;
        for (const Entry& e : R.rows)
          if (e.alive && e.g == q) {
            R.min_file[q] = e.file;
            break;
          }
      }
    int32_t *dg = in_blk(g), *dgc = reset ? nullptr : in_blk(gc);
    uint8_t* st = out_blk<uint8_t>(n);
    LiCounts* c = out_blk<LiCounts>(1);
    const int nt = tiles_for(n), rows = nt ? D.row_tiles() : 0;
    const LiMem M = D.M;
    if (nt) {
      launch(nt, [=] { k_li_arm(M, n, dg); });
      launch(nt, [=] { k_li_mark<true>(M, n, dg, dgc, flags, st); });
      if (rows) launch(rows, [=] { k_li_gc_scan(M, flags); });
      launch(nt, [=] { k_li_gc_finish(M, n, dg); });
    }
    launch(1, [=] { k_li_gc_sum(nt, rows, M, c); });
    counts_are(w, *c, applied, 0, died, nog, rep);
    for (int32_t i = 0; i < n; i++)
      if (st[i] != want[i]) fail(w, "status", i, st[i]);
    state_is(w);
    for (void* p : {(void*)dg, (void*)dgc, (void*)st, (void*)c}) free(p);
  }

  /* ---- lookup ---- */
  int32_t lookup(const std::string& w, const std::vector<int32_t>& g, const std::vector<int32_t>& lo,
                 const std::vector<int32_t>& hi, const std::vector<uint8_t>& hm, int32_t cap) {
    const int32_t n = (int32_t)g.size();
    std::vector<uint8_t> want;
    int32_t nog, rep;
    const std::vector<int32_t> rec = firsts(g, want, nog, rep);
    std::vector<int32_t> hrow, hrec;
    for (size_t r = 0; r < R.rows.size(); r++) {
      const Entry& e = R.rows[r];
      const int32_t a = rec[e.g];
      if (!e.alive || a < 0) continue;
      if (wdiff(e.slot, lo[a]) >= 0 && (hm.empty() || !hm[a] || wdiff(e.slot, hi[a]) <= 0)) hrow.push_back((int32_t)r), hrec.push_back(a);
    }
    const int32_t hits = (int32_t)hrow.size(), done = std::min(hits, cap);
    int32_t *dg = in_blk(g), *dlo = in_blk(lo), *dhi = hm.empty() ? nullptr : in_blk(hi);
    uint8_t* dhm = hm.empty() ? nullptr : in_blk(hm);
    uint8_t* st = out_blk<uint8_t>(n);
    LiCounts* c = out_blk<LiCounts>(1);
    LiOut O{};
    if (cap > 0) {
      O.rec = out_blk<int32_t>(cap), O.row = out_blk<int32_t>(cap), O.slot = out_blk<int32_t>(cap), O.bnum = out_blk<int32_t>(cap);
      O.bcoord = out_blk<int32_t>(cap), O.file = out_blk<int32_t>(cap), O.off = out_blk<long long>(cap), O.len = out_blk<int32_t>(cap);
    }
    const int nt = tiles_for(n), rows = nt ? D.row_tiles() : 0;
    const LiMem M = D.M;
    const LiQuery Q{dlo, dhi, dhm};
    if (nt) {
      launch(nt, [=] { k_li_arm(M, n, dg); });
      launch(nt, [=] { k_li_mark<false>(M, n, dg, nullptr, 0, st); });
      if (rows) launch(rows, [=] { k_li_scan<LI_SCAN_LOOKUP>(M, Q, 0); });
    }
    launch(1, [=] { k_li_scan_offsets<LI_SCAN_LOOKUP>(nt, rows, M, cap, c); });
    if (rows && cap > 0) launch(rows, [=] { k_li_scan_move<LI_SCAN_LOOKUP>(M, cap, O); });
    if (nt) launch(nt, [=] { k_li_disarm(M, n, dg); });
    counts_are(w, *c, done, hits, 0, nog, rep);
    for (int32_t i = 0; i < n; i++)
      if (st[i] != want[i]) fail(w, "status", i, st[i]);
    for (int32_t o = 0; o < done; o++) {
      const Entry& e = R.rows[hrow[o]];
      if (O.rec[o] != hrec[o] || O.row[o] != hrow[o] || O.slot[o] != e.slot || O.bnum[o] != e.bnum || O.bcoord[o] != e.bcoord ||
          O.file[o] != e.file || O.off[o] != e.off || O.len[o] != e.len)
        fail(w, "hit", o, O.row[o]);
    }
    if (cap > 0 && !(sent_from(O.rec, done, cap) && sent_from(O.row, done, cap) && sent_from(O.slot, done, cap) &&
                     sent_from(O.bnum, done, cap) && sent_from(O.bcoord, done, cap) && sent_from(O.file, done, cap) &&
                     sent_from(O.off, done, cap) && sent_from(O.len, done, cap)))
      fail(w, "written at or beyond n_done");
    state_is(w);
    for (void* p : {(void*)dg, (void*)dlo, (void*)dhi, (void*)dhm, (void*)st, (void*)c, (void*)O.rec, (void*)O.row, (void*)O.slot,
                    (void*)O.bnum, (void*)O.bcoord, (void*)O.file, (void*)O.off, (void*)O.len})
      free(p);
    return hits;
  }

  /* ---- file_rows: -> the rows handed out ---- */
  std::vector<int32_t> file_rows(const std::string& w, int32_t file, int32_t cap) {
    std::vector<int32_t> hrow;
    for (size_t r = 0; r < R.rows.size(); r++)
      if (R.rows[r].alive && R.rows[r].file == file) hrow.push_back((int32_t)r);
    const int32_t hits = (int32_t)hrow.size(), done = std::min(hits, cap);
    LiCounts* c = out_blk<LiCounts>(1);
    LiOut O{};
    if (cap > 0) {
      O.row = out_blk<int32_t>(cap), O.gidx = out_blk<int32_t>(cap), O.slot = out_blk<int32_t>(cap), O.bnum = out_blk<int32_t>(cap);
      O.bcoord = out_blk<int32_t>(cap), O.off = out_blk<long long>(cap), O.len = out_blk<int32_t>(cap), O.gc = out_blk<int32_t>(cap);
    }
    const int rows = D.row_tiles();
    const LiMem M = D.M;
    if (rows) launch(rows, [=] { k_li_scan<LI_SCAN_FILE>(M, LiQuery{}, file); });
    launch(1, [=] { k_li_scan_offsets<LI_SCAN_FILE>(0, rows, M, cap, c); });
    if (rows && cap > 0) launch(rows, [=] { k_li_scan_move<LI_SCAN_FILE>(M, cap, O); });
    counts_are(w, *c, done, hits, 0, 0, 0);
    for (int32_t o = 0; o < done; o++) {
      const Entry& e = R.rows[hrow[o]];
      if (O.row[o] != hrow[o] || O.gidx[o] != e.g || O.slot[o] != e.slot || O.bnum[o] != e.bnum || O.bcoord[o] != e.bcoord ||
          O.off[o] != e.off || O.len[o] != e.len || O.gc[o] != R.gc[e.g])
        fail(w, "row", o, O.row[o]);
      if (wdiff(e.slot, O.gc[o]) <= 0) fail(w, "an alive row at or below its group's GC slot", o);
    }
    if (cap > 0 && !(sent_from(O.row, done, cap) && sent_from(O.gidx, done, cap) && sent_from(O.gc, done, cap) &&
                     sent_from(O.off, done, cap)))
      fail(w, "written at or beyond n_done");
    state_is(w);
    for (void* p : {(void*)c, (void*)O.row, (void*)O.gidx, (void*)O.slot, (void*)O.bnum, (void*)O.bcoord, (void*)O.off, (void*)O.len,
                    (void*)O.gc})
      free(p);
    hrow.resize(done);
    return hrow;
  }

  /* ---- relocate ---- */
  void relocate(const std::string& w, int32_t gen, const std::vector<int32_t>& o_row, const std::vector<int32_t>& k_src,
                int32_t new_file, const int32_t* n_dev_val = nullptr) {
    const int32_t n = (int32_t)o_row.size();
    const int32_t m = n_dev_val ? std::min(n, std::max(*n_dev_val, 0)) : n;
    std::vector<long long> off(n);
    std::vector<int32_t> ln(n);
    for (int32_t j = 0; j < n; j++) off[j] = 7 + 13ll * j, ln[j] = 3 + j % 11;
    int32_t done = 0;
    for (int32_t j = 0; j < m; j++) {
      const long long src = k_src.empty() ? j : k_src[j];
      if (gen != R.gen || src < 0 || src >= n) continue;
      const long long r = o_row[src];
      if (r < 0 || r >= (long long)R.rows.size() || !R.rows[r].alive) continue;
      R.rows[r].file = new_file, R.rows[r].off = off[j], R.rows[r].len = ln[j], done++;
    }
    int32_t *dr = in_blk(o_row), *dsrc = k_src.empty() ? nullptr : in_blk(k_src), *dl = in_blk(ln);
    long long* doff = in_blk(off);
    int32_t* dn = n_dev_val ? in_blk(std::vector<int32_t>{*n_dev_val}) : nullptr;
    LiCounts* c = out_blk<LiCounts>(1);
    const int nt = tiles_for(n);
    const LiMem M = D.M;
    if (nt) launch(nt, [=] { k_li_reloc(M, n, dn, gen, dr, dsrc, new_file, doff, dl); });
    launch(1, [=] { k_li_reloc_sum(nt, M, c); });
    counts_are(w, *c, done, 0, m - done, 0, 0);
    state_is(w);
    for (void* p : {(void*)dr, (void*)dsrc, (void*)dl, (void*)doff, (void*)dn, (void*)c}) free(p);
  }

  /* ---- files ---- */
  void files(const std::string& w, int32_t base, int32_t nf) {
    std::vector<int32_t> wr(nf, 0), wg(nf, 0);
    int32_t out = 0, lo = INT32_MAX;
    for (const Entry& e : R.rows) {
      if (!e.alive) continue;
      const long long d = (long long)e.file - base;
      if (d >= 0 && d < nf) wr[d]++;
      else out++;
    }
    for (int32_t g = 0; g < R.G; g++) {
      if (R.min_file[g] == -1) continue;
      lo = std::min(lo, R.min_file[g]);
      const long long d = (long long)R.min_file[g] - base;
      if (d >= 0 && d < nf) wg[d]++;
      else out++;
    }
    int32_t *o_r = out_blk<int32_t>(nf), *o_g = out_blk<int32_t>(nf), *o_m = out_blk<int32_t>(1);
    LiCounts* c = out_blk<LiCounts>(1);
    const int row_wgs = std::min(D.row_tiles(), GPX_LI_HIST_GRID), grp_wgs = std::min(tiles_for(R.G), GPX_LI_HIST_GRID);
    const LiMem M = D.M;
    launch(std::max(tiles_for(nf), 1), [=] { k_li_files_init(M, nf, o_r, o_g); });
    if (row_wgs) launch(row_wgs, [=] { k_li_files_hist<false>(M, base, nf, o_r, M.tile_cnt); });
    if (grp_wgs) launch(grp_wgs, [=] { k_li_files_hist<true>(M, base, nf, o_g, M.tile_off); });
    launch(1, [=] { k_li_files_sum(row_wgs, grp_wgs, M, o_m, c); });
    counts_are(w, *c, 0, 0, out, 0, 0);
    for (int32_t f = 0; f < nf; f++)
      if (o_r[f] != wr[f] || o_g[f] != wg[f]) fail(w, "bin", f, o_r[f]);
    if (*o_m != (lo == INT32_MAX ? -1 : lo)) fail(w, "the smallest min file", *o_m);
    state_is(w);
    for (void* p : {(void*)o_r, (void*)o_g, (void*)o_m, (void*)c}) free(p);
  }

  /* ---- compact ---- */
  void compact(const std::string& w) {
    std::vector<Entry> keep;
    for (const Entry& e : R.rows)
      if (e.alive) keep.push_back(e);
    R.rows = keep;
    R.gen++;
    LiCounts* c = out_blk<LiCounts>(1);
    const int rows = D.row_tiles();
    const LiMem M = D.M;
    if (rows) launch(rows, [=] { k_li_scan<LI_SCAN_ALIVE>(M, LiQuery{}, 0); });
    launch(1, [=] { k_li_scan_offsets<LI_SCAN_ALIVE>(0, rows, M, INT32_MAX, c); });
    if (rows) launch(rows, [=] { k_li_scan_move<LI_SCAN_ALIVE>(M, INT32_MAX, LiOut{}); });
    std::swap(D.M.T, D.M.U);
    counts_are(w, *c, (int32_t)keep.size(), 0, 0, 0, 0);
    state_is(w);
    free(c);
  }
};

static std::vector<int32_t> seq(int32_t n, int32_t a, int32_t step = 1) {
  std::vector<int32_t> v(n);
  for (int32_t i = 0; i < n; i++) v[i] = (int32_t)((uint32_t)a + (uint32_t)step * (uint32_t)i);
  return v;
}
static std::vector<int32_t> rep(int32_t n, int32_t a) { return std::vector<int32_t>(n, a); }

#define NG 128
#define NCAP 1024

static int case_tile_edges() {
  Sys S(NG, NCAP, 1024);
  S.set_gc("a: two groups refuse small slots", {5, 6}, {10, INT32_MAX});
  auto mixed = [&](int32_t n, const char* w) {
    std::vector<int32_t> g(n), s(n);
    for (int32_t i = 0; i < n; i++) {
      g[i] = (i * 7) % NG, s[i] = 20 + i;
      if (i % 64 == 62) g[i] = -1;
      if (i % 256 == 0) g[i] = 5, s[i] = 3;
      if (i % 256 == 255) g[i] = NG;
    }
    S.add(w, g, s, n % 5);
  };
  auto fill_to = [&](int32_t tail, const char* w) {
    const int32_t k = tail - (int32_t)S.R.rows.size();
    S.add(w, rep(k, 1), seq(k, 50), 1);
    if ((int32_t)S.R.rows.size() != tail) fail(w, "tail");
  };
  mixed(255, "a: 255 records onto a tail at 0");
  fill_to(255, "a: fill to 255");
  mixed(1, "a: one stale record at 255");
  S.add("a: one record at 255", {2}, {9}, 1);
  mixed(256, "a: 256 records at 256");
  mixed(257, "a: 257 records");
  fill_to(1023, "a: fill to 1,023");
  std::vector<int32_t> g(513), s = seq(513, 1000);
  for (int32_t i = 0; i < 513; i++) g[i] = i % 5 == 0 ? 6 : i % 4;
  S.add("a: 513 records into one row of room", g, s, 7);
  if (S.R.rows.size() != NCAP) fail("a", "the table is not full");
  S.set_gc("a: everything up to 900 dies", seq(NG, 0), rep(NG, 900));
  S.compact("a: compact");
  if (S.R.rows.size() != 1) fail("a", "rows after the compaction");
  const std::vector<int32_t> g2(g.begin() + 1, g.end()), s2(s.begin() + 1, s.end());
  for (int32_t nd : {-3, 0, 2, 512, 521}) S.add("a: n_dev " + std::to_string(nd), g2, s2, 8, &nd);
  S.add("a: no records", {}, {}, 1);
  S.lookup("a: everything", seq(NG, 0), rep(NG, 0), {}, {}, NCAP);
  return S.checks;
}

static int case_gc_reset() {
  Sys S(NG, NCAP, 1024);
  std::vector<int32_t> g(900);
  for (int32_t i = 0; i < 900; i++) g[i] = i % 3 == 0 ? 9 : i % 7;
  S.add("b: file 2", std::vector<int32_t>(g.begin(), g.begin() + 450), seq(450, 1), 2);
  S.add("b: file 3", std::vector<int32_t>(g.begin() + 450, g.end()), seq(450, 451), 3);
  S.set_gc("b: a group three times, one unknown", {9, 9, 200, 9, 1}, {100, 400, 5, 7, 2});
  S.set_gc("b: forwards, the min file moves", {9}, {460});
  S.set_gc("b: backwards", {9}, {50});
  S.add("b: slot 60 is needed again, 40 is not", {9, 9}, {60, 40}, 4);
  S.set_gc("b: equal", {9}, {50});
  S.set_gc("b: all die", {9}, {5000});
  S.add("b: a later add", {9}, {5001}, 5);
  const std::vector<int32_t> w = {INT32_MAX - 2, INT32_MAX - 1, INT32_MAX, INT32_MIN, INT32_MIN + 1, INT32_MIN + 2};
  std::vector<int32_t> ww = w;
  ww.insert(ww.end(), w.begin(), w.end());
  std::vector<int32_t> gg = rep(6, 20);
  gg.insert(gg.end(), 6, 21);
  S.set_gc("b: GC slots below the wrap", {20, 21}, {INT32_MAX - 3, INT32_MAX - 3});
  S.add("b: slots across the wrap", gg, ww, 6);
  S.set_gc("b: GC slots at MAX_VALUE and MIN_VALUE", {20, 21}, {INT32_MAX, INT32_MIN});
  S.add("b: stale and added at the wrap", {20, 20, 21, 21}, {INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN + 1}, 6);
  S.lookup("b: a range across the wrap", {20, 21, 9}, rep(3, INT32_MAX - 5), rep(3, INT32_MIN + 5), {1, 1, 0}, 64);
  S.set_gc("b: RESET", {1, 9, 1}, {}, GPX_LI_RESET_);
  S.add("b: a fresh index takes slot 1", {9, 1}, {1, 1}, 7);
  S.files("b: files", 0, 8);
  S.set_gc("b: no records", {}, {});
  return S.checks;
}

static int case_lookup() {
  Sys S(NG, NCAP, 1024);
  std::vector<int32_t> g(700), s(700);
  for (int32_t i = 0; i < 700; i++) g[i] = i % 10, s[i] = 1 + i / 10;
  S.add("c: 70 slots of ten groups", g, s, 0);
  S.add("c: slot 30 three more times", {3, 3, 3}, {30, 30, 30}, 1);
  S.set_gc("c: group 11 near the wrap", {11}, {INT32_MAX - 10});
  S.add("c: group 11 across the wrap", rep(8, 11), seq(8, INT32_MAX - 3), 1);
  const std::vector<int32_t> q = {0, 1, 2, 3, 4, 5, 6, 0, 50, 11, 11, 7};
  const std::vector<int32_t> lo = {1, 10, 80, 30, 40, 5, INT32_MIN, 1, 1, INT32_MAX - 1, 0, 71};
  const std::vector<int32_t> hi = {70, 20, 90, 30, 39, 0, 0, 3, 9, INT32_MIN + 1, 0, 0};
  const std::vector<uint8_t> hm = {1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0};
  const int32_t hits = S.lookup("c: every kind of range", q, lo, hi, hm, NCAP);
  if (hits != 70 + 11 + 4 + 66 + 4) fail("c", "hits", hits);
  int32_t edge = 0; /* the hits of the table's first tile */
  for (int32_t r = 0; r < 256; r++) {
    const Entry& e = S.R.rows[r];
    edge += (e.g == 0) || (e.g == 1 && e.slot >= 10 && e.slot <= 20) || (e.g == 3 && e.slot == 30) || (e.g == 5 && e.slot >= 5);
  }
  for (int32_t cap : {0, 1, edge - 1, edge, edge + 1, hits - 1, hits})
    S.lookup("c: cap " + std::to_string(cap), q, lo, hi, hm, cap);
  S.lookup("c: no max anywhere", q, lo, {}, {}, NCAP);
  S.lookup("c: no records", {}, {}, {}, {}, 16);
  return S.checks;
}

static int case_relocate() {
  Sys S(NG, NCAP, 1024);
  std::vector<int32_t> g(300), s(300);
  for (int32_t i = 0; i < 300; i++) g[i] = i % 6, s[i] = 1 + i / 6;
  S.add("d: 300 rows", g, s, 0);
  S.set_gc("d: ten rows die", {0}, {10});
  const std::vector<int32_t> rows = S.file_rows("d: the rows of file 0", 0, NCAP);
  const int32_t n = (int32_t)rows.size();
  if (n != 290) fail("d", "rows", n);
  S.file_rows("d: cut", 0, 100);
  S.file_rows("d: counted", 0, 0);
  S.file_rows("d: no such file", 3, 16);
  S.relocate("d: a stale generation", 1, rows, {}, 9);
  std::vector<int32_t> bad = rows, src = seq(n, 0);
  bad[0] = -1, bad[1] = (int32_t)S.R.rows.size(), bad[2] = INT32_MAX, bad[3] = 0;
  src[5] = -1, src[6] = n, src[7] = INT32_MAX;
  S.relocate("d: garbage rows, a dead row, k_src out of range", 0, bad, src, 9);
  const int32_t half = n / 2, neg = -1, over = n + 5;
  S.relocate("d: n_dev half", 0, rows, {}, 10, &half);
  S.relocate("d: n_dev negative", 0, rows, {}, 11, &neg);
  S.relocate("d: n_dev larger", 0, rows, {}, 12, &over);
  S.files("d: the min files did not move", 0, 16);
  S.compact("d: compact");
  S.relocate("d: row indices from before the compaction", 0, rows, {}, 13);
  S.relocate("d: no records", 1, {}, {}, 13);
  return S.checks;
}

static int case_files() {
  Sys S(NG, NCAP, 1024);
  S.files("e: an empty index, one bin", 0, 1);
  S.add("e: one group", {4, 4, 4}, {1, 2, 3}, 4000);
  S.files("e: 4,096 bins, one group", 0, GPX_LI_MAX_FILES_);
  for (int32_t f : {17, 5000, 4095, 0, 4096}) {
    std::vector<int32_t> g(NG + 3), s(NG + 3);
    for (int32_t i = 0; i < NG + 3; i++) g[i] = i % NG, s[i] = 10 + f % 97 + i / NG;
    S.add("e: file " + std::to_string(f), g, s, f);
  }
  S.files("e: 4,096 bins, all groups", 0, GPX_LI_MAX_FILES_);
  S.files("e: one bin", 17, 1);
  S.files("e: above", 4001, 100);
  S.files("e: a base below zero", -50, 60);
  S.files("e: no bins", 0, 0);
  return S.checks;
}

static int case_compact() {
  Sys S(NG, NCAP, 1024);
  std::vector<int32_t> g(600);
  for (int32_t i = 0; i < 600; i++) g[i] = i % 8;
  S.add("f: 600 rows", g, seq(600, 1), 1);
  S.compact("f: no dead rows");
  S.set_gc("f: every other row dies", {1, 3, 5, 7}, rep(4, INT32_MAX - 1000));
  S.compact("f: alternating");
  S.lookup("f: after", seq(NG, 0), rep(NG, 0), {}, {}, NCAP);
  S.set_gc("f: RESET of all", seq(NG, 0), {}, GPX_LI_RESET_);
  S.compact("f: all dead");
  S.compact("f: an empty table");
  S.add("f: add after", {1}, {1}, 2);
  return S.checks;
}

/* more than GPX_BLOCK tiles: tile_offsets goes round twice */
static int case_rounds() {
  const int32_t cap = 70000, n = 66000, groups = 64;
  Sys S(groups, cap, n);
  std::vector<int32_t> g(n), s(n);
  for (int32_t i = 0; i < n; i++) g[i] = (int32_t)((i * 2654435761u) >> 8) % groups, s[i] = 1 + i;
  S.add("g: 66,000 rows", g, s, 3);
  S.add("g: 66,000 more into 4,000 rows of room", g, seq(n, 70001), 4);
  S.set_gc("g: half the groups", seq(groups / 2, 0, 2), rep(groups / 2, 40000));
  S.lookup("g: lookup, cut", seq(groups, 0), rep(groups, 30000), rep(groups, 50000), std::vector<uint8_t>(groups, 1), 5000);
  S.file_rows("g: file 4", 4, cap);
  S.files("g: files", 0, 8);
  S.compact("g: compact");
  S.lookup("g: after", seq(groups, 0), rep(groups, 0), {}, {}, cap);
  return S.checks;
}

int main() {
  int checks = 0;
  checks += case_tile_edges();
  checks += case_gc_reset();
  checks += case_lookup();
  checks += case_relocate();
  checks += case_files();
  checks += case_compact();
  checks += case_rounds();
  printf("checks: %d\n", checks);
  return 0;
}
