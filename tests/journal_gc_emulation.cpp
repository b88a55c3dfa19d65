// Lockstep CPU emulation of the kernels of gigapaxos_amd/csrc/gpx_journal_gc.hip.h (tests/test_journal_gc_abi.py
// compiles and runs this with AddressSanitizer): the real header, unmodified, on top of the real gpx_bytes.hip.h and
// gpx_journal.hip.h.  One std::thread per lane of a workgroup, one workgroup at a time (tests/lockstep_runtime.h).
// Every buffer is a heap block of its exact size - `in` rounded up to 16 bytes, which is the read contract of
// include/gpx_journal_gc.h - the scratch starts as garbage and `out`, the verdicts and the rows carry a sentinel, so an
// index past an end is a sanitizer report and a byte written beyond what is done a failure.  The launches and their
// conditions are those of jg_run (gpx_journal_gc_dev.inc).  The expected answer is a plain loop over the rules of the
// header.  The case list is that of tests/test_journal_gc_gpu.py.  What this cannot show is what only the GPU has: the
// compiler's code and memory ordering between launches.
#include <algorithm>
#include <barrier>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "lockstep_runtime.h"

#define GPX_S_OK 0
#define GPX_R_TOLOG 1
#define GPX_NT_JOURNAL 32
static uint32_t __builtin_amdgcn_alignbyte(uint32_t hi, uint32_t lo, uint32_t s) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (s & 3)));
}
// gpx_kernels.hip.h's aggregates and stream helpers, as plain accesses
struct alignas(16) I4 { int32_t x, y, z, w; };
static I4 mk4(int32_t x, int32_t y, int32_t z, int32_t w) { return I4{x, y, z, w}; }
template <int BIT> static int32_t stream_load4(const int32_t* p) { return *p; }
template <int BIT> static I4 stream_load16(const I4* p) { return *p; }
template <int BIT, class T> static void stream_store4(T* p, T v) { *p = v; }
template <int BIT> static void stream_store16(I4* p, I4 v) { *p = v; }

#include "gpx_bytes.hip.h"
#include "gpx_journal.hip.h"
#include "gpx_journal_gc.hip.h"

template <class T> static T* blk_of(const std::vector<T>& v) {
  T* p = (T*)malloc(std::max<size_t>(v.size(), 1) * sizeof(T));
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}
/* a 16-byte aligned heap block of exactly `bytes` bytes (what `in` and `out` must be) */
static uint8_t* blk16(size_t bytes, int fill) {
  void* p = nullptr;
  if (posix_memalign(&p, 16, std::max<size_t>(bytes, 1))) exit(2);
  memset(p, fill, std::max<size_t>(bytes, 1));
  return (uint8_t*)p;
}

static void fail(const std::string& what, const char* msg, long long a = 0, long long b = 0) {
  printf("%s: %s (%lld, %lld)\n", what.c_str(), msg, a, b);
  exit(1);
}

static uint32_t g_rng = 4711u;
static uint32_t rnd() { return g_rng = g_rng * 1664525u + 1013904223u; }

#define NGROUPS 100
#define GF_STOPPED_BITS 0xFFFFFFF0u /* any bit but the exists bit: a stopped group is judged like any other */

struct Case { /* the inputs of one call and the group state */
  std::vector<uint8_t> in;
  long long in_bytes = 0, in_base = 0;
  std::vector<int32_t> gidx, slot, len, bnum, bcoord, cp;
  std::vector<long long> off;
  bool have_cp = false, have_in = true;
  std::vector<uint32_t> g_flags = std::vector<uint32_t>(NGROUPS, 1u);
  std::vector<int32_t> a_gc = std::vector<int32_t>(NGROUPS, 0);
  int32_t n() const { return (int32_t)len.size(); }
};

/* appends one entry of `len` bytes to the block and a row for it; keep decides the slot against the group's a_gc */
static void add_entry(Case& c, int32_t len, bool keep, bool named = true) {
  const long long at = (long long)c.in.size();
  for (int sft = 24; sft >= 0; sft -= 8) c.in.push_back((uint8_t)((uint32_t)len >> sft));
  for (int32_t q = 0; q < len; q++) c.in.push_back((uint8_t)(1 + (rnd() >> 24) % 250));
  c.in_bytes = (long long)c.in.size();
  if (!named) return;
  const int32_t i = c.n(), g = (int32_t)(rnd() >> 8) % NGROUPS;
  c.gidx.push_back(g), c.slot.push_back((int32_t)((uint32_t)c.a_gc[g] + (keep ? 1u + (rnd() >> 28) : 0u - (rnd() >> 28))));
  c.off.push_back(c.in_base + at), c.len.push_back(len), c.bnum.push_back(i % 7), c.bcoord.push_back(100 + i % 3);
}

static Case fresh(long long in_base = 0) {
  Case c;
  c.in_base = in_base;
  for (int g = 0; g < NGROUPS; g++) c.a_gc[g] = (int32_t)(rnd() >> 4) - (1 << 26), c.g_flags[g] = 1u | (rnd() & 0xFF00u);
  return c;
}

struct Result {
  JgCounts counts;
  std::vector<uint8_t> bytes;
  std::vector<int32_t> src;
};

/* one call: the expected answer by a plain loop, the four launches as jg_run makes them, every output compared */
static Result run(const std::string& what, const Case& c, long long cap_bytes, int32_t cap_entries, long long out_base,
                  int32_t flags, bool null_cols = false, int32_t row_base = 0) {
  const int32_t n = c.n();
  const bool co = flags & GPX_JG_COUNT_ONLY_;
  // ---- expected ----
  struct Ent { int32_t row, len; long long rel, pos; bool head; };
  std::vector<Ent> ents;
  std::vector<uint8_t> ver(n);
  int32_t bad = 0, unj = 0;
  long long total = 0, named = 0, prev_end = -1;
  for (int32_t i = 0; i < n; i++) {
    const long long L = c.len[i];
    bool ok = c.off[i] >= c.in_base && L >= 0 && L <= (long long)INT32_MAX - 4;
    const long long rel = ok ? c.off[i] - c.in_base : 0;
    ok = ok && rel <= c.in_bytes && rel + 4 + L <= c.in_bytes;
    if (ok && c.have_in) {
      const uint32_t u = (uint32_t)c.in[rel] << 24 | (uint32_t)c.in[rel + 1] << 16 | (uint32_t)c.in[rel + 2] << 8 | c.in[rel + 3];
      ok = u == (uint32_t)L;
    }
    if (!ok) { ver[i] = GPX_JG_BAD_, bad++, prev_end = -1; continue; }
    named += 4 + L;
    const int32_t g = c.gidx[i];
    if (g < 0 || g >= NGROUPS || !(c.g_flags[g] & 1u)) {
      ver[i] = GPX_JG_KEEP_UNJUDGED_, unj++;
    } else {
      uint32_t gc = (uint32_t)c.a_gc[g];
      if (c.have_cp && (int32_t)((uint32_t)c.cp[i] - gc) < 0) gc = (uint32_t)c.cp[i];
      ver[i] = (int32_t)((uint32_t)c.slot[i] - gc) > 0 ? GPX_JG_KEEP_ : GPX_JG_DROP_;
    }
    if (ver[i] == GPX_JG_DROP_) { prev_end = -1; continue; }
    ents.push_back(Ent{i, (int32_t)L, rel, total, prev_end != rel});
    total += 4 + L, prev_end = rel + 4 + L;
  }
  int32_t heads = 0;
  for (const Ent& e : ents) heads += e.head;
  const int32_t unchanged = bad == 0 && (int32_t)ents.size() == n && heads == (n ? 1 : 0) && (n == 0 || ents[0].rel == 0) && total == c.in_bytes;
  int32_t n_done = 0, runs_done = 0;
  long long bytes_done = 0;
  if (!co && !((flags & GPX_JG_SKIP_UNCHANGED_) && unchanged))
    for (const Ent& e : ents) {
      if (n_done >= cap_entries || e.pos + 4 + e.len > cap_bytes) break;
      n_done++, runs_done += e.head, bytes_done = e.pos + 4 + e.len;
    }
  std::vector<uint8_t> want;
  for (int32_t e = 0; e < n_done; e++) want.insert(want.end(), c.in.begin() + ents[e].rel, c.in.begin() + ents[e].rel + 4 + ents[e].len);
  if ((long long)want.size() != bytes_done) fail(what, "the test's own expectation", (long long)want.size(), bytes_done);

  // ---- the buffers: exact sizes, garbage in the scratch, sentinels in the outputs ----
  /* `in`: in_bytes rounded up to 16 and not a byte more (the block may hold more than the call is told) */
  const size_t in_sz = ((size_t)c.in_bytes + 15) & ~(size_t)15;
  uint8_t* in = nullptr;
  if (c.have_in) {
    in = blk16(in_sz, 0xEE);
    if (!c.in.empty()) memcpy(in, c.in.data(), std::min<size_t>(c.in.size(), in_sz));
  }
  int32_t *gidx = blk_of(c.gidx), *slot = blk_of(c.slot), *len = blk_of(c.len);
  int32_t *bnum = null_cols ? nullptr : blk_of(c.bnum), *bcoord = null_cols ? nullptr : blk_of(c.bcoord);
  int32_t* cp = c.have_cp ? blk_of(c.cp) : nullptr;
  long long* off = blk_of(c.off);
  uint32_t* gf = blk_of(c.g_flags);
  int32_t* agc = blk_of(c.a_gc);
  const int ntiles = (n + GPX_JR_TILE - 1) / GPX_JR_TILE;
  JgMem M;
  M.tile_cnt = blk<int32_t>(ntiles, 0xEE), M.tile_heads = blk<int32_t>(ntiles, 0xEE), M.tile_bad = blk<int32_t>(ntiles, 0xEE);
  M.tile_unj = blk<int32_t>(ntiles, 0xEE), M.tile_eoff = blk<int32_t>(ntiles, 0xEE), M.tile_hoff = blk<int32_t>(ntiles, 0xEE);
  M.tile_bytes = blk<long long>(ntiles, 0xEE), M.tile_named = blk<long long>(ntiles, 0xEE), M.tile_boff = blk<long long>(ntiles, 0xEE);
  M.d_pos = blk<long long>(n, 0xEE), M.d_src = blk<long long>(n, 0xEE), M.first_ok = blk<int32_t>(1, 0xEE);
  uint8_t* out = co ? nullptr : blk16((size_t)cap_bytes, 0xA5);
  uint8_t* verdict = blk<uint8_t>(n, 0xA5);
  auto rowcol = [&](bool wanted) { return co || !wanted ? nullptr : blk<int32_t>(cap_entries, 0xA5); };
  int32_t *k_src = rowcol(true), *k_gidx = rowcol(true), *k_slot = rowcol(true), *k_bnum = rowcol(!null_cols);
  int32_t *k_bcoord = rowcol(!null_cols), *k_len = rowcol(true);
  long long* k_off = co ? nullptr : blk<long long>(cap_entries, 0xA5);
  JgCounts* counts = blk<JgCounts>(1, 0xA5);
  JgIn I;
  I.in = in, I.win_lo = 0, I.win_hi = c.in_bytes, I.in_base = c.in_base, I.e_gidx = gidx, I.e_slot = slot, I.e_off = off;
  I.e_len = len, I.e_bnum = bnum, I.e_bcoord = bcoord, I.cp_slot = cp, I.force = nullptr, I.g_flags = gf, I.a_gc = agc;
  I.max_groups = NGROUPS, I.n = n, I.row_base = row_base;
  const JgOut O{out, cap_bytes, out_base, cap_entries, k_src, k_gidx, k_slot, k_bnum, k_bcoord, k_off, k_len};

  // ---- jg_run's launches ----
  if (ntiles) launch(ntiles, [&] { k_jg_tile(I, M, verdict); });
  launch(1, [&] { k_jg_offsets(ntiles, I, M, cap_bytes, cap_entries, flags, c.in_bytes, counts); });
  if (ntiles && !co && cap_entries > 0 && cap_bytes >= 4) {
    launch(ntiles, [&] { k_jg_rows(I, M, O, counts); });
    const long long tiles = cap_bytes / GPX_JR_CTILE + 1;
    launch((int)std::min<long long>(tiles, 3), [&] { k_jg_copy(in, M, out, counts); }); /* a small grid: the stride loop */
  }

  // ---- compare ----
  const JgCounts k = *counts;
  if (k.n_usable != n - bad || k.n_keep != (int32_t)ents.size() || k.n_done != n_done || k.n_bad != bad || k.n_unjudged != unj ||
      k.n_runs_done != runs_done || k.unchanged != unchanged || k.reserved != 0 || k.keep_bytes != total ||
      k.bytes_done != bytes_done || k.named_bytes != named || k.reserved2 != 0) {
    printf("%s: counts %d %d %d %d %d %d %d %d %lld %lld %lld, want %d %zu %d %d %d %d %d 0 %lld %lld %lld\n", what.c_str(), k.n_usable,
           k.n_keep, k.n_done, k.n_bad, k.n_unjudged, k.n_runs_done, k.unchanged, k.reserved, k.keep_bytes, k.bytes_done,
           k.named_bytes, n - bad, ents.size(), n_done, bad, unj, runs_done, unchanged, total, bytes_done, named);
    exit(1);
  }
  for (int32_t i = 0; i < n; i++)
    if (verdict[i] != ver[i]) fail(what, "verdict wrong", i, verdict[i]);
  Result R{k, want, {}};
  if (!co) {
    for (long long q = 0; q < cap_bytes; q++)
      if (out[q] != (q < bytes_done ? want[q] : 0xA5)) fail(what, q < bytes_done ? "byte wrong" : "byte written beyond bytes_done", q, out[q]);
    const int32_t s4 = (int32_t)0xA5A5A5A5;
    for (int32_t e = 0; e < cap_entries; e++) {
      if (e < n_done) {
        const Ent& w = ents[e];
        if (k_src[e] != row_base + w.row || k_gidx[e] != c.gidx[w.row] || k_slot[e] != c.slot[w.row] ||
            (k_bnum && k_bnum[e] != c.bnum[w.row]) || (k_bcoord && k_bcoord[e] != c.bcoord[w.row]) ||
            k_off[e] != out_base + w.pos || k_len[e] != w.len)
          fail(what, "row wrong", e, k_src[e]);
        R.src.push_back(k_src[e]);
      } else if (k_src[e] != s4 || k_gidx[e] != s4 || k_slot[e] != s4 || (k_bnum && k_bnum[e] != s4) ||
                 (k_bcoord && k_bcoord[e] != s4) || k_len[e] != s4 || k_off[e] != (long long)0xA5A5A5A5A5A5A5A5ull) {
        fail(what, "row written beyond n_done", e);
      }
    }
  }
  printf("%s: ok, %d kept of %d rows, %d refused, %d unjudged, %lld bytes; done %d in %d runs, %lld; unchanged %d\n", what.c_str(),
         k.n_keep, n, k.n_bad, k.n_unjudged, k.keep_bytes, k.n_done, k.n_runs_done, k.bytes_done, k.unchanged);
  free(in), free(gidx), free(slot), free(len), free(bnum), free(bcoord), free(cp), free(off), free(gf), free(agc);
  free(M.tile_cnt), free(M.tile_heads), free(M.tile_bad), free(M.tile_unj), free(M.tile_eoff), free(M.tile_hoff);
  free(M.tile_bytes), free(M.tile_named), free(M.tile_boff), free(M.d_pos), free(M.d_src), free(M.first_ok);
  free(out), free(verdict), free(k_src), free(k_gidx), free(k_slot), free(k_bnum), free(k_bcoord), free(k_len), free(k_off), free(counts);
  return R;
}

static long long kept_bytes(const Case& c) { /* what the kept rows of a case built by add_entry need */
  long long t = 0;
  for (int32_t i = 0; i < c.n(); i++)
    if ((int32_t)((uint32_t)c.slot[i] - (uint32_t)c.a_gc[c.gidx[i]]) > 0) t += 4 + c.len[i];
  return t;
}

int main() {
  const int32_t CO = GPX_JG_COUNT_ONLY_, SK = GPX_JG_SKIP_UNCHANGED_;
  // 1. verdicts: gc x slot around it and half the ring away, cp_slot absent / above / equal / below / wrapped, a stopped
  //    group, group numbers that cannot be judged
  for (int mode = 0; mode < 5; mode++) { /* cp_slot: none, acc + 3, acc, acc - 3, acc + 2^31 (behind acc on the ring) */
    Case c = fresh(1000);
    const int32_t gcs[] = {-1, 0, 5, INT32_MAX - 1, INT32_MIN};
    for (int q = 0; q < 5; q++) c.a_gc[q] = gcs[q], c.g_flags[q] = 1u;
    c.g_flags[3] |= GF_STOPPED_BITS; /* stopped, and every other bit */
    c.g_flags[7] = GF_STOPPED_BITS;  /* every bit but exists: never created */
    c.have_cp = mode > 0;
    const uint32_t dcp[] = {0u, 3u, 0u, 0u - 3u, 0x80000000u};
    for (int q = 0; q < 5; q++)
      for (uint32_t d : {0u - 1u, 0u, 1u, 0x7fffffffu, 0x80000000u, 0u - 4u, 0u - 3u, 0u - 2u}) {
        add_entry(c, 3 + q, true);
        c.gidx.back() = q, c.slot.back() = (int32_t)((uint32_t)gcs[q] + d), c.cp.push_back((int32_t)((uint32_t)gcs[q] + dcp[mode]));
      }
    for (int32_t g : {-1, NGROUPS, 7, INT32_MIN, INT32_MAX}) add_entry(c, 9, false), c.gidx.back() = g, c.cp.push_back(0);
    const Result r = run("verdicts, cp_slot mode " + std::to_string(mode), c, 1 << 16, c.n(), 7, 0);
    if (r.counts.n_unjudged != 5 || r.counts.n_keep == c.n() || r.counts.n_keep == 5) fail("verdicts", "vacuous", r.counts.n_keep);
  }
  // 2. phases: every source-start phase modulo 16 against every output phase modulo 16 at a run head; entries of 0 .. 40
  //    bytes, kept or dropped at random, so that a dropped entry's length shifts the one against the other
  {
    Case c = fresh();
    for (int i = 0; i < 6000; i++) add_entry(c, i < 410 ? i % 41 : (int32_t)(rnd() >> 8) % 41, (rnd() >> 16) & 1);
    std::set<int> seen;
    long long pos = 0;
    bool prev = false;
    for (int32_t i = 0; i < c.n(); i++) {
      const bool keep = (int32_t)((uint32_t)c.slot[i] - (uint32_t)c.a_gc[c.gidx[i]]) > 0;
      if (keep && !prev) seen.insert((int)(c.off[i] & 15) * 16 + (int)(pos & 15));
      if (keep) pos += 4 + c.len[i];
      prev = keep;
    }
    if (seen.size() != 256) fail("phases", "not every pair of phases is reached", (long long)seen.size());
    run("phases", c, pos, c.n(), 0, 0);
    run("phases, a file offset as base", [&] { Case d = c; d.in_base = 1ll << 40; for (auto& o : d.off) o += 1ll << 40; return d; }(), pos, c.n(), 1ll << 41, 0);
  }
  // 3. runs of kept rows over the row-tile edge; everything kept; nothing kept; adjacency broken
  {
    Case c = fresh();
    for (int32_t rl : {1, 2, 63, 64, 65, 255, 256, 257, 1, 190}) {
      for (int32_t q = 0; q < rl; q++) add_entry(c, (int32_t)(rnd() >> 8) % 50, true);
      for (int32_t q = 0; q < 1 + rl / 2; q++) add_entry(c, (int32_t)(rnd() >> 8) % 50, false);
    }
    const Result r = run("runs of 1 .. 257 kept rows", c, kept_bytes(c), c.n(), 0, 0);
    if (r.counts.n_runs_done != 10 || 3 * r.counts.n_keep < c.n() || 3 * (c.n() - r.counts.n_keep) < c.n()) fail("runs", "vacuous", r.counts.n_keep, c.n());
    Case all = fresh(64);
    for (int i = 0; i < 700; i++) add_entry(all, (int32_t)(rnd() >> 8) % 120, true);
    const Result u = run("everything kept", all, all.in_bytes, all.n(), 64, 0);
    if (!u.counts.unchanged || u.counts.n_runs_done != 1 || u.bytes != all.in) fail("everything kept", "not the input");
    const Result s = run("everything kept, skip unchanged", all, all.in_bytes, all.n(), 64, SK);
    if (!s.counts.unchanged || s.counts.n_done || s.counts.bytes_done) fail("skip unchanged", "something was written");
    Case none = fresh();
    for (int i = 0; i < 700; i++) add_entry(none, (int32_t)(rnd() >> 8) % 120, false);
    const Result z = run("nothing kept", none, none.in_bytes, none.n(), 0, SK);
    if (z.counts.n_keep || z.counts.unchanged) fail("nothing kept", "counts");
    /* everything kept, but: unnamed bytes between rows; a trailing unnamed entry; rows out of offset order */
    Case gaps = fresh();
    for (int i = 0; i < 600; i++) add_entry(gaps, (int32_t)(rnd() >> 8) % 60, true, i % 50 != 49);
    const Result g = run("unnamed bytes between rows", gaps, gaps.in_bytes, gaps.n(), 0, SK);
    if (g.counts.unchanged || g.counts.n_runs_done != 12 || g.counts.n_keep != gaps.n()) fail("gaps", "counts", g.counts.n_runs_done);
    Case tail = all;
    add_entry(tail, 5, true, false);
    if (run("a trailing unnamed entry", tail, tail.in_bytes, tail.n(), 64, SK).counts.unchanged) fail("tail", "unchanged");
    Case swapped = all;
    for (auto* v : {&swapped.gidx, &swapped.slot, &swapped.len, &swapped.bnum, &swapped.bcoord}) std::swap((*v)[300], (*v)[301]);
    std::swap(swapped.off[300], swapped.off[301]);
    const Result w = run("rows out of offset order", swapped, swapped.in_bytes, swapped.n(), 64, SK);
    if (w.counts.unchanged || w.counts.n_runs_done != 4 || w.counts.keep_bytes != swapped.in_bytes) fail("swapped", "counts", w.counts.n_runs_done);
  }
  // 4. copy tiles: kept totals of 16384 k - 5 .. 16384 k + 5; more than 256 runs in a tile; one huge entry
  for (int k = 1; k <= 3; k++)
    for (int d = -5; d <= 5; d++) {
      const long long total = 16384ll * k + d;
      Case c = fresh();
      long long t = 0;
      while (total - t > 400) {
        const int32_t l = 97 + (int32_t)(rnd() >> 8) % 50;
        add_entry(c, l, true), t += 4 + l;
        if ((rnd() >> 20) % 3 == 0) add_entry(c, (int32_t)(rnd() >> 8) % 30, false);
      }
      const long long rest = total - t; /* two entries fill it exactly */
      add_entry(c, (int32_t)(rest / 2) - 4, true), add_entry(c, (int32_t)(rest - rest / 2) - 4, true), add_entry(c, 3, false);
      if (kept_bytes(c) != total) fail("tile edges", "the test's own sizes", kept_bytes(c), total);
      run("tile edge " + std::to_string(k) + (d < 0 ? " - " : " + ") + std::to_string(d < 0 ? -d : d), c, total, c.n(), 77, 0);
    }
  {
    Case c = fresh();
    for (int i = 0; i < 10000; i++) add_entry(c, (rnd() >> 16) & 1, i & 1);
    const Result r = run("10,000 entries of 0 and 1 bytes, alternately kept", c, kept_bytes(c), c.n(), 0, 0);
    if (r.counts.n_runs_done != 5000) fail("alternately kept", "runs", r.counts.n_runs_done);
    Case big = fresh();
    for (int i = 0; i < 2001; i++) add_entry(big, i == 1000 ? (1 << 20) + 13 : (int32_t)(rnd() >> 8) % 60, i == 1000 || (rnd() >> 16) % 3);
    run("one entry of 1 MiB + 13 among 2,000", big, kept_bytes(big), big.n(), 5, 0);
  }
  // 5. refusals
  {
    Case c = fresh(500);
    for (int i = 0; i < 40; i++) add_entry(c, 10 + i, i % 3 != 0);
    Case ok = c;
    c.off[5] = c.in_base - 1;                      /* a negative offset */
    c.off[6] = INT64_MIN;
    c.len[7] = -1;
    c.len[8] = INT32_MAX - 3;                      /* above the largest length */
    c.len[39] += 1;                                /* ends one byte past in_bytes */
    c.in[(size_t)(c.off[20] - c.in_base) + 3] ^= 1; /* a wrong prefix */
    c.off[22] += 1;                                /* a row that points into the middle of an entry */
    c.off[23] = c.in_base + c.in_bytes - 3;        /* a prefix that would straddle the end */
    c.off[24] = INT64_MAX;
    const Result r = run("refusals", c, c.in_bytes, c.n(), 0, 0);
    if (r.counts.n_bad != 9) fail("refusals", "nine rows were to be refused", r.counts.n_bad);
    c.have_in = false; /* without `in` the prefix cannot be tested: rows 20 and 22 pass */
    const Result q = run("refusals, counts only without in", c, 0, 0, 0, CO);
    if (q.counts.n_bad != 7) fail("refusals", "seven rows were to be refused", q.counts.n_bad);
  }
  // 6. caps, the cut call continued, counts only, n = 0, NULL optional columns
  {
    Case c = fresh();
    std::vector<long long> ends(1, 0);
    for (int i = 0; i < 1400; i++) {
      const int32_t l = i == 0 ? 21 : (int32_t)(rnd() >> 8) % 90;
      const bool keep = i == 0 || (i & 1);
      add_entry(c, l, keep);
      if (keep) ends.push_back(ends.back() + 4 + l);
    }
    const long long all = ends.back();
    const int32_t n = c.n(), nk = (int32_t)ends.size() - 1;
    for (long long cb : {0ll, 3ll, 24ll, 25ll, 26ll, ends[300] - 1, ends[300], ends[300] + 1, ends[300] + 2, ends[300] + 3, ends[300] + 4,
                         ends[128], ends[256] - 1, all - 1, all, all + 100})
      run("cap_bytes " + std::to_string(cb), c, cb, n, 9, 0);
    for (int32_t ce : {0, 1, 127, 128, 129, nk - 1, nk, nk + 10}) run("cap_entries " + std::to_string(ce), c, all, ce, 9, 0);
    run("both caps", c, ends[400] + 2, 300, 0, 0);
    {
      std::vector<uint8_t> got;
      long long base = 500;
      int32_t first = 0, calls = 0;
      while (first < n) {
        Case part = c;
        auto cut = [&](auto& v) { v.erase(v.begin(), v.begin() + first); };
        cut(part.gidx), cut(part.slot), cut(part.len), cut(part.bnum), cut(part.bcoord), cut(part.off);
        const Result r = run("continued, from row " + std::to_string(first), part, 5000, 64, base, 0, false, first);
        if (r.counts.n_done == 0) fail("continued", "no progress", first);
        got.insert(got.end(), r.bytes.begin(), r.bytes.end());
        base += r.counts.bytes_done;
        first = r.src.back() + 1;
        calls++;
        if (r.counts.n_done == r.counts.n_keep) break;
      }
      const Result whole = run("continued: the uncut call", c, all, n, 500, 0);
      if (got != whole.bytes || base != 500 + all) fail("continued", "the pieces are not the whole", (long long)got.size(), calls);
    }
    run("counts only", c, 0, 0, 0, CO);
    c.have_in = false;
    run("counts only, no in", c, 0, 0, 0, CO);
    c.have_in = true;
    run("NULL optional columns", c, all, n, 3, 0, true);
    run("n = 0", fresh(), 64, 4, 0, 0);
    run("n = 0, counts only", fresh(), 0, 0, 0, CO | SK);
  }
  // 7. more tiles of rows than one round of k_jg_offsets holds, a cut in its second round
  {
    Case c = fresh();
    for (int i = 0; i < 70000; i++) add_entry(c, i % 3 ? 0 : 2, (i >> 1) & 1);
    run("70,000 rows", c, kept_bytes(c), c.n(), 0, 0);
    run("70,000 rows, cut in tile 256", c, 1 << 20, 32800, 0, 0);
  }
  return 0;
}
