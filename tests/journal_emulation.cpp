// Lockstep CPU emulation of the kernels of gigapaxos_amd/csrc/gpx_journal.hip.h (tests/test_journal_abi.py compiles and
// runs this with AddressSanitizer): the real header, unmodified, on top of the real gpx_bytes.hip.h.  One std::thread
// per lane of a workgroup, barriers for __syncthreads and for the wave collectives, one workgroup at a time.  Every
// buffer is a heap block of its exact size (`frames` rounded up to 4 bytes: load4_unaligned reads whole aligned words),
// the scratch starts as garbage and `out` and the rows carry a sentinel, so an index past an end is a sanitizer report
// and a byte written beyond what is done a failure.  The launches and their conditions are those of jr_run (gpx_journal_dev.inc).  The expected answer is a plain
// loop over the rules of include/gpx_journal.h.  What this cannot show is what only the GPU has: the compiler's code and
// memory ordering between launches (tests/test_journal_gpu.py).
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

#define GPX_S_OK 0
#define GPX_S_NOGROUP 1
#define GPX_S_WINDOW 3
#define GPX_R_TOLOG 1
#define GPX_R_STORED 2
#define GPX_NT_JOURNAL 32
static uint32_t __builtin_amdgcn_alignbyte(uint32_t hi, uint32_t lo, uint32_t s) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (s & 3)));
}
// gpx_kernels.hip.h's aggregates and stream helpers, as plain accesses
struct alignas(16) I4 { int32_t x, y, z, w; };
static I4 mk4(int32_t x, int32_t y, int32_t z, int32_t w) { return I4{x, y, z, w}; }
template <int BIT> static int32_t stream_load4(const int32_t* p) { return *p; }
template <int BIT, class T> static void stream_store4(T* p, T v) { *p = v; }
template <int BIT> static void stream_store16(I4* p, I4 v) { *p = v; }

#include "gpx_bytes.hip.h"
#include "gpx_journal.hip.h"

template <class T> static T* blk_of(const std::vector<T>& v) {
  T* p = (T*)malloc(std::max<size_t>(v.size(), 1) * sizeof(T));
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

static void fail(const std::string& what, const char* msg, long long a = 0, long long b = 0) {
  printf("%s: %s (%lld, %lld)\n", what.c_str(), msg, a, b);
  exit(1);
}

struct Case { /* the inputs of one call */
  std::vector<uint8_t> frames;
  std::vector<long long> off; /* n_frames + 1 entries, or n_frames with len */
  std::vector<int32_t> len;   /* empty: the decode form */
  std::vector<int32_t> rec_frame; /* empty: identity */
  std::vector<int32_t> gidx, slot, bnum, bcoord;
  std::vector<uint8_t> r_flags, status;
  int32_t n_frames = 0;
  long long frames_bytes = 0; /* what the call is told; the block holds as much */
  int32_t n() const { return (int32_t)status.size(); }
};

static uint32_t g_rng = 12345u;
static uint32_t rnd() { return g_rng = g_rng * 1664525u + 1013904223u; }

/* frames of the given lengths, every record to log, record i -> frame i.  padded: the pack calls' form (frame_len,
 * starts at multiples of 4, pad bytes that must never show up); else contiguous (frame_off alone) */
static Case make(const std::vector<int32_t>& lens, bool padded) {
  Case c;
  long long pos = 0;
  for (size_t f = 0; f < lens.size(); f++) {
    c.off.push_back(pos);
    if (padded) c.len.push_back(lens[f]);
    for (int32_t q = 0; q < lens[f]; q++) c.frames.push_back((uint8_t)(1 + (rnd() >> 24) % 250));
    pos += lens[f];
    if (padded)
      while (pos & 3) c.frames.push_back(0xFF), pos++;
    c.gidx.push_back((int32_t)f * 3 + 1), c.slot.push_back((int32_t)f - 7), c.bnum.push_back((int32_t)f % 5);
    c.bcoord.push_back(100 + (int32_t)f % 3), c.r_flags.push_back(GPX_R_TOLOG | (f % 2 ? GPX_R_STORED : 0)), c.status.push_back(GPX_S_OK);
  }
  if (!padded) c.off.push_back(pos);
  c.n_frames = (int32_t)lens.size();
  c.frames_bytes = pos;
  return c;
}

struct Result {
  JrCounts counts;
  std::vector<uint8_t> bytes;
  std::vector<int32_t> rec;
};

/* one call: the expected answer by a plain loop, the four launches as jr_run makes them, every output compared */
static Result run(const std::string& what, const Case& c, long long cap_bytes, int32_t cap_entries, long long base_offset,
                  int32_t flags, int32_t rec_base = 0, long long win_lo = 0, long long win_hi = -1) {
  const int32_t n = c.n();
  if (win_hi < 0) win_hi = c.frames_bytes;
  // ---- expected ----
  struct Ent { int32_t rec, len; long long src, pos; };
  std::vector<Ent> ents;
  int32_t bad = 0;
  long long total = 0;
  for (int32_t i = 0; i < n; i++) {
    if (c.status[i] != GPX_S_OK || !(c.r_flags[i] & GPX_R_TOLOG)) continue;
    const long long f = c.rec_frame.empty() ? (long long)rec_base + i : c.rec_frame[i];
    bool ok = f >= 0 && f < c.n_frames;
    long long s = 0, L = 0;
    if (ok) {
      s = c.off[f];
      L = c.len.empty() ? c.off[f + 1] - s : c.len[f];
      ok = s >= 0 && L >= 0 && L <= (long long)INT32_MAX - 4 && s >= win_lo && s + L <= win_hi;
    }
    if (!ok) { bad++; continue; }
    ents.push_back(Ent{i, (int32_t)L, s, total});
    total += 4 + L;
  }
  int32_t n_done = 0;
  long long bytes_done = 0;
  if (!(flags & GPX_JR_COUNT_ONLY_))
    for (const Ent& e : ents) {
      if (n_done >= cap_entries || e.pos + 4 + e.len > cap_bytes) break;
      n_done++, bytes_done = e.pos + 4 + e.len;
    }
  std::vector<uint8_t> want;
  for (int32_t e = 0; e < n_done; e++) {
    for (int sft = 24; sft >= 0; sft -= 8) want.push_back((uint8_t)((uint32_t)ents[e].len >> sft));
    want.insert(want.end(), c.frames.begin() + ents[e].src, c.frames.begin() + ents[e].src + ents[e].len);
  }
  if ((long long)want.size() != bytes_done) fail(what, "the test's own expectation", (long long)want.size(), bytes_done);

  // ---- the buffers: exact sizes, garbage in the scratch, sentinels in the outputs ----
  std::vector<uint8_t> win(c.frames.begin() + win_lo, c.frames.begin() + std::min<long long>(win_hi, (long long)c.frames.size()));
  while (win.size() & 3) win.push_back(0xEE); /* rounded up to 4 bytes */
  uint8_t* frames = blk_of(win);
  long long* foff = blk_of(c.off);
  int32_t* flen = c.len.empty() ? nullptr : blk_of(c.len);
  int32_t* rf = c.rec_frame.empty() ? nullptr : blk_of(c.rec_frame);
  int32_t *gidx = blk_of(c.gidx), *slot = blk_of(c.slot), *bnum = blk_of(c.bnum), *bcoord = blk_of(c.bcoord);
  uint8_t *rfl = blk_of(c.r_flags), *st = blk_of(c.status);
  const int ntiles = (n + GPX_JR_TILE - 1) / GPX_JR_TILE;
  JrMem M;
  M.tile_cnt = blk<int32_t>(ntiles, 0xEE), M.tile_bad = blk<int32_t>(ntiles, 0xEE), M.tile_eoff = blk<int32_t>(ntiles, 0xEE);
  M.tile_bytes = blk<long long>(ntiles, 0xEE), M.tile_boff = blk<long long>(ntiles, 0xEE);
  M.d_pos = blk<long long>(n, 0xEE), M.d_src = blk<long long>(n, 0xEE), M.d_len = blk<int32_t>(n, 0xEE);
  const bool co = flags & GPX_JR_COUNT_ONLY_;
  uint8_t* out = co ? nullptr : blk<uint8_t>((size_t)cap_bytes, 0xA5);
  int32_t *e_rec = co ? nullptr : blk<int32_t>(cap_entries, 0xA5), *e_gidx = co ? nullptr : blk<int32_t>(cap_entries, 0xA5);
  int32_t *e_slot = co ? nullptr : blk<int32_t>(cap_entries, 0xA5), *e_bnum = co ? nullptr : blk<int32_t>(cap_entries, 0xA5);
  int32_t *e_bcoord = co ? nullptr : blk<int32_t>(cap_entries, 0xA5), *e_len = co ? nullptr : blk<int32_t>(cap_entries, 0xA5);
  long long* e_off = co ? nullptr : blk<long long>(cap_entries, 0xA5);
  JrCounts* counts = blk<JrCounts>(1, 0xA5);
  JrIn I;
  I.frames = frames, I.win_lo = win_lo, I.win_hi = win_hi, I.n_frames = c.n_frames, I.frame_off = foff, I.frame_len = flen;
  I.rec_frame = rf, I.gidx = gidx, I.slot = slot, I.bnum = bnum, I.bcoord = bcoord, I.r_flags = rfl, I.status = st;
  I.n = n, I.rec_base = rec_base;
  const JrOut O{out, cap_bytes, base_offset, cap_entries, e_rec, e_gidx, e_slot, e_bnum, e_bcoord, e_off, e_len};

  // ---- jr_run's launches ----
  if (ntiles) launch(ntiles, [&] { k_jr_tile(I, M); });
  launch(1, [&] { k_jr_offsets(ntiles, I, M, cap_bytes, cap_entries, flags, counts); });
  if (ntiles && !co && cap_entries > 0 && cap_bytes >= 4) {
    launch(ntiles, [&] { k_jr_rows(I, M, O, counts); });
    const long long tiles = cap_bytes / GPX_JR_CTILE + 1;
    launch((int)std::min<long long>(tiles, 3), [&] { k_jr_copy(frames, M, out, counts); }); /* a small grid: the stride loop */
  }

  // ---- compare ----
  const JrCounts k = *counts;
  if (k.n_entries != (int32_t)ents.size() || k.n_done != n_done || k.n_bad != bad || k.reserved != 0 || k.n_bytes != total ||
      k.bytes_done != bytes_done) {
    printf("%s: counts %d %d %d %d %lld %lld, want %zu %d %d 0 %lld %lld\n", what.c_str(), k.n_entries, k.n_done, k.n_bad,
           k.reserved, k.n_bytes, k.bytes_done, ents.size(), n_done, bad, total, bytes_done);
    exit(1);
  }
  Result R{k, want, {}};
  if (!co) {
    for (long long q = 0; q < cap_bytes; q++)
      if (out[q] != (q < bytes_done ? want[q] : 0xA5)) fail(what, q < bytes_done ? "byte wrong" : "byte written beyond bytes_done", q, out[q]);
    const int32_t s4 = (int32_t)0xA5A5A5A5;
    for (int32_t e = 0; e < cap_entries; e++) {
      if (e < n_done) {
        const Ent& w = ents[e];
        if (e_rec[e] != rec_base + w.rec || e_gidx[e] != c.gidx[w.rec] || e_slot[e] != c.slot[w.rec] || e_bnum[e] != c.bnum[w.rec] ||
            e_bcoord[e] != c.bcoord[w.rec] || e_off[e] != base_offset + w.pos || e_len[e] != w.len)
          fail(what, "row wrong", e, e_rec[e]);
        R.rec.push_back(e_rec[e]);
      } else if (e_rec[e] != s4 || e_gidx[e] != s4 || e_slot[e] != s4 || e_bnum[e] != s4 || e_bcoord[e] != s4 || e_len[e] != s4 ||
                 e_off[e] != (long long)0xA5A5A5A5A5A5A5A5ull) {
        fail(what, "row written beyond n_done", e);
      }
    }
  }
  printf("%s: ok, %d entries of %d records, %d refused, %lld bytes; done %d, %lld\n", what.c_str(), k.n_entries, n, k.n_bad,
         k.n_bytes, k.n_done, k.bytes_done);
  free(frames), free(foff), free(flen), free(rf), free(gidx), free(slot), free(bnum), free(bcoord), free(rfl), free(st);
  free(M.tile_cnt), free(M.tile_bad), free(M.tile_eoff), free(M.tile_bytes), free(M.tile_boff), free(M.d_pos), free(M.d_src), free(M.d_len);
  free(out), free(e_rec), free(e_gidx), free(e_slot), free(e_bnum), free(e_bcoord), free(e_len), free(e_off), free(counts);
  return R;
}

static long long need(const std::vector<int32_t>& lens) {
  long long t = 0;
  for (int32_t l : lens) t += 4 + l;
  return t;
}

int main() {
  const int32_t CO = GPX_JR_COUNT_ONLY_;
  // 1. every phase of a boundary: lengths 0 .. 40 in turn, then random in [0, 300]; both frame forms; the buffers exact
  {
    std::vector<int32_t> lens;
    for (int i = 0; i < 2000; i++) lens.push_back(i < 410 ? i % 41 : (int32_t)(rnd() >> 8) % 301);
    run("phases, contiguous frames", make(lens, false), need(lens), 2000, 0, 0);
    run("phases, padded frames", make(lens, true), need(lens), 2000, 1ll << 40, 0);
  }
  // 2. tile edges: totals of 16384 k - 5 .. 16384 k + 5 whose last entry is a bare prefix: it ends at, straddles (at
  //    each of its bytes) or starts at the tile boundary
  for (int k = 1; k <= 3; k++)
    for (int d = -5; d <= 5; d++) {
      const long long total = 16384ll * k + d;
      std::vector<int32_t> lens;
      long long t = 0;
      while (total - t - 4 > 400) lens.push_back(97 + (int32_t)(rnd() >> 8) % 50), t += 4 + lens.back();
      const long long rest = total - t - 4; /* two entries fill it exactly, then the bare prefix */
      lens.push_back((int32_t)(rest / 2) - 4), lens.push_back((int32_t)(rest - rest / 2) - 4), lens.push_back(0);
      if (need(lens) != total) fail("tile edges", "the test's own sizes", need(lens), total);
      run("tile edge " + std::to_string(k) + (d < 0 ? " - " : " + ") + std::to_string(d < 0 ? -d : d), make(lens, false), total,
          (int32_t)lens.size(), 77, 0);
    }
  // 3. many entries per tile (more than 4,096 descriptors in 16 KB: rounds), one entry over 64 tiles
  {
    std::vector<int32_t> lens;
    for (int i = 0; i < 10000; i++) lens.push_back((rnd() >> 16) & 1);
    run("10,000 entries of 0 and 1 bytes", make(lens, false), need(lens), 10000, 0, 0);
    std::vector<int32_t> zeros(5000, 0);
    run("5,000 empty frames", make(zeros, true), need(zeros), 5000, 0, 0);
    lens.clear();
    for (int i = 0; i < 2001; i++) lens.push_back(i == 1000 ? (1 << 20) + 13 : (int32_t)(rnd() >> 8) % 60);
    run("one entry of 1 MiB + 13 among 2,000", make(lens, false), need(lens), 2001, 5, 0);
  }
  // 4. selection: every status x flag bits x frame validity
  {
    std::vector<int32_t> lens;
    for (int i = 0; i < 40; i++) lens.push_back(10 + i);
    Case c = make(lens, true);
    const Case base = c;
    c.gidx.clear(), c.slot.clear(), c.bnum.clear(), c.bcoord.clear(), c.r_flags.clear(), c.status.clear();
    /* frames 30 .. 33 are spoilt: a negative start, a negative length, a range one byte past the end, a huge length */
    c.off[30] = -4, c.len[31] = -1, c.len[39] = (int32_t)(c.frames_bytes - c.off[39]) + 1, c.len[33] = INT32_MAX - 3;
    const int32_t fr[] = {3, -1, c.n_frames, 30, 31, 39, 33, 7, 3, INT32_MIN, INT32_MAX};
    for (uint8_t stv : {GPX_S_OK, GPX_S_WINDOW, GPX_S_NOGROUP})
      for (uint8_t fl : {0, GPX_R_TOLOG, GPX_R_STORED, GPX_R_TOLOG | GPX_R_STORED, 0xFD, 0xFE})
        for (int32_t f : fr) {
          const int32_t i = c.n();
          c.rec_frame.push_back(f), c.status.push_back(stv), c.r_flags.push_back(fl);
          c.gidx.push_back(i), c.slot.push_back(2 * i), c.bnum.push_back(3 * i), c.bcoord.push_back(-i);
        }
    const Result r = run("selection", c, 1 << 20, c.n(), 1000, 0);
    if (r.counts.n_entries != 3 * 3 || r.counts.n_bad != 3 * 8) fail("selection", "counts", r.counts.n_entries, r.counts.n_bad);
    run("selection, counts only", c, 0, 0, 0, CO);
    /* the decode form: an offset that runs backwards is a negative length */
    Case d = make(lens, false);
    d.off[20] = d.off[21] + 5;
    const Result q = run("selection, offsets running backwards", d, 1 << 20, d.n(), 0, 0);
    if (q.counts.n_bad != 1) fail("selection", "one frame was to be refused", q.counts.n_bad);
    /* a window, as the host twin stages it: frames outside are refused, the others are found inside it */
    const Result w = run("a window of the block", base, 1 << 20, base.n(), 0, 0, 0, base.off[5], base.off[30]);
    if (w.counts.n_entries != 25 || w.counts.n_bad != 15) fail("window", "counts", w.counts.n_entries, w.counts.n_bad);
  }
  // 5. caps, the cut call continued, counts only, n = 0
  {
    std::vector<int32_t> lens;
    for (int i = 0; i < 700; i++) lens.push_back(i == 0 ? 21 : (int32_t)(rnd() >> 8) % 90);
    const Case c = make(lens, false);
    const long long all = need(lens);
    const int32_t n = c.n();
    std::vector<long long> ends(1, 0);
    for (int32_t l : lens) ends.push_back(ends.back() + 4 + l);
    for (long long cb : {0ll, 3ll, 24ll, 25ll, 26ll, ends[300] - 1, ends[300], ends[300] + 1, ends[300] + 2, ends[300] + 3, ends[300] + 4,
                         ends[256], ends[512] - 1, all - 1, all, all + 100})
      run("cap_bytes " + std::to_string(cb), c, cb, n, 9, 0);
    for (int32_t ce : {0, 1, 255, 256, 257, n - 1, n, n + 10}) run("cap_entries " + std::to_string(ce), c, all, ce, 9, 0);
    run("both caps", c, ends[400] + 2, 300, 0, 0);
    /* a cut call continued with the columns advanced past the last done record */
    {
      std::vector<uint8_t> got;
      Case rest = c;
      rest.rec_frame.resize(n);
      for (int32_t i = 0; i < n; i++) rest.rec_frame[i] = i;
      long long base = 500;
      int32_t first = 0, calls = 0;
      while (first < n) {
        Case part = rest;
        auto cut = [&](auto& v) { v.erase(v.begin(), v.begin() + first); };
        cut(part.rec_frame), cut(part.gidx), cut(part.slot), cut(part.bnum), cut(part.bcoord), cut(part.r_flags), cut(part.status);
        const Result r = run("continued, from record " + std::to_string(first), part, 5000, 64, base, 0, first);
        if (r.counts.n_done == 0) fail("continued", "no progress", first);
        got.insert(got.end(), r.bytes.begin(), r.bytes.end());
        base += r.counts.bytes_done;
        first = r.rec.back() + 1;
        calls++;
        if (r.counts.n_done == r.counts.n_entries) break;
      }
      const Result whole = run("continued: the uncut call", c, all, n, 500, 0);
      if (got != whole.bytes || base != 500 + all) fail("continued", "the pieces are not the whole", (long long)got.size(), calls);
    }
    run("counts only", c, 0, 0, 0, CO);
    run("n = 0", make({}, false), 64, 4, 0, 0);
    run("n = 0, counts only", make({}, true), 0, 0, 0, CO);
  }
  // 6. more tiles of records than one round of k_jr_offsets holds, a cut in a late tile
  {
    std::vector<int32_t> lens(257 * GPX_JR_TILE + 1, 0);
    for (size_t i = 0; i < lens.size(); i += 3) lens[i] = 2;
    Case c = make(lens, false);
    for (int32_t i = 0; i < c.n(); i += 2) c.r_flags[i] = GPX_R_STORED; /* every other one is not logged */
    run("258 tiles of records", c, need(lens), c.n(), 0, 0);
    run("258 tiles of records, cut in tile 256", c, 1 << 20, 32800, 0, 0);
  }
  return 0;
}
