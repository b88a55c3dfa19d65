// Lockstep CPU emulation of the byte-run core, gigapaxos_amd/csrc/gpx_bytes.hip.h (tests/test_journal_abi.py compiles
// and runs this with AddressSanitizer and UBSan): the real header, unmodified, over tests/lockstep_runtime.h, each piece
// against a plain loop.  Every buffer is a heap block of its exact size and every output carries a sentinel behind it,
// so an index past an end is a sanitizer report and a byte written beyond the end a failure.  What the families build
// from these pieces is in their own emulations (tests/journal_emulation.cpp, tests/journal_gc_emulation.cpp).
#include <climits>
#include <cstdio>
#include <string>

#include "lockstep_runtime.h"

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

static void fail(const std::string& what, long long a = 0, long long b = 0, long long c = 0) {
  printf("%s: (%lld, %lld, %lld)\n", what.c_str(), a, b, c);
  exit(1);
}
static uint32_t g_rng = 88172645u;
static uint32_t rnd() { return (g_rng = g_rng * 1664525u + 1013904223u) >> 8; }

/* the plain loop both searches are held against */
static int32_t last_le(const long long* a, int32_t n, long long key) {
  int32_t r = -1;
  for (int32_t i = 0; i < n; i++)
    if (a[i] <= key) r = i;
  return r;
}
/* n strictly ascending positions, neighbours at least 2 apart, and the keys: below the first, equal to each sampled
 * element, between it and its neighbour, above the last */
static long long* ascending(int32_t n, std::vector<long long>& keys, bool below_first) {
  long long* a = blk<long long>(n, 0);
  for (int32_t i = 0; i < n; i++) a[i] = 10 + 3ll * i + rnd() % 2;
  keys.clear();
  if (below_first) keys.push_back(n ? a[0] - 1 : 5);
  for (int32_t i = 0; i < n; i += (n > 65 && i > 1 && i < n - 62 ? 61 : 1)) keys.push_back(a[i]), keys.push_back(a[i] + 1);
  keys.push_back(n ? a[n - 1] + 100 : LLONG_MAX);
  return a;
}

// ---- wave_search: key q is searched by wave q % 4, all of its lanes ----
static void wave_search_case(int32_t n) {
  std::vector<long long> keys;
  long long* a = ascending(n, keys, true);
  int32_t* got = blk<int32_t>(keys.size(), 0xA5);
  launch(1, [&] {
    for (size_t q = threadIdx.x >> 6; q < keys.size(); q += GPX_BLOCK / 64) {
      const int32_t r = wave_search(a, n, keys[q]);
      if (r != last_le(a, n, keys[q])) fail("wave_search", n, keys[q], r); /* every lane has the answer */
      if ((threadIdx.x & 63) == 0) got[q] = r;
    }
  });
  for (size_t q = 0; q < keys.size(); q++)
    if (got[q] != last_le(a, n, keys[q])) fail("wave_search: stored", n, keys[q], got[q]);
  free(a), free(got);
}

// ---- lds_search: one lane per key; s[0] <= key is the caller's duty ----
static void lds_search_case(int32_t n) {
  std::vector<long long> keys;
  long long* s = ascending(n, keys, false);
  launch(1, [&] {
    for (size_t q = threadIdx.x; q < keys.size(); q += GPX_BLOCK) {
      const int32_t r = lds_search(s, n, keys[q]);
      if (r != last_le(s, n, keys[q])) fail("lds_search", n, keys[q], r);
    }
  });
  free(s);
}

// ---- load4_unaligned<0>: the last bytes of a block that ends where the last needed word ends ----
static void load4_case(size_t bytes, uint32_t align) {
  uint8_t* b = blk<uint8_t>(bytes, 0);
  for (size_t q = 0; q < bytes; q++) b[q] = (uint8_t)(1 + rnd() % 250);
  const uint8_t* p = b + bytes - (align ? 8 - align : 4); /* align 0 needs one word, any other the last two */
  if (((uintptr_t)p & 3) != align) fail("load4_unaligned: the test's own address", (long long)bytes, align);
  const uint32_t want = p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
  if (load4_unaligned<0>(p) != want || load4_unaligned<GPX_NT_JOURNAL>(p) != want) fail("load4_unaligned", (long long)bytes, align);
  free(b);
}

// ---- copy_runs: the smallest family there is - runs concatenated as they are, the chunk built byte by byte ----
struct RawTile {
  long long pos[GPX_BYTES_SPAN], src[GPX_BYTES_SPAN];
};
struct RawCopy {
  typedef RawTile Tile;
  const uint8_t* in;
  const long long* d_src;
  void stage(RawTile& T, int32_t e, int32_t s) const { T.src[s] = d_src[e]; }
  void chunk(const RawTile& T, long long P, long long Pe, int32_t k, int32_t ns, uint32_t (&w)[4]) const {
    /* what the skeleton promises: k is the last staged descriptor at or below P */
    if (k < 0 || k >= ns || T.pos[k] > P || (k + 1 < ns && T.pos[k + 1] <= P) || Pe <= P || Pe > P + 16) fail("copy_runs: chunk's arguments", P, k, ns);
    for (int d = 0; d < 4; d++) w[d] = 0x5A5A5A5Au; /* not the sentinel: what is at or beyond Pe must never be stored */
    for (int c = 0; P + c < Pe; c++) {
      while (k + 1 < ns && T.pos[k + 1] <= P + c) k++;
      w[c >> 2] = (w[c >> 2] & ~(0xFFu << (8 * (c & 3)))) | (uint32_t)in[T.src[k] + (P + c - T.pos[k])] << (8 * (c & 3));
    }
  }
};
static void k_raw_copy(const uint8_t* in, const long long* d_pos, const long long* d_src, int32_t nD, uint8_t* out, long long lim) {
  copy_runs(RawCopy{in, d_src}, d_pos, nD, out, lim);
}
/* runs of the given lengths, scattered over a source block with gaps of 0 .. 6 bytes, copied on a grid of `grid` */
static void copy_case(const std::string& what, const std::vector<long long>& lens, int grid) {
  const int32_t nD = (int32_t)lens.size();
  long long *d_pos = blk<long long>(nD, 0), *d_src = blk<long long>(nD, 0), total = 0, src = 0;
  for (int32_t r = 0; r < nD; r++) {
    if (lens[r] < 4) fail(what + ": the test's own runs", r, lens[r]);
    src += rnd() % 7;
    d_pos[r] = total, d_src[r] = src;
    total += lens[r], src += lens[r];
  }
  uint8_t* in = blk<uint8_t>((size_t)src, 0);
  for (long long q = 0; q < src; q++) in[q] = (uint8_t)(1 + rnd() % 250);
  uint8_t* out = blk<uint8_t>((size_t)total + 64, 0xA5); /* malloc: 16-byte aligned, as `out` has to be */
  launch(grid, [&] { k_raw_copy(in, d_pos, d_src, nD, out, total); });
  for (int32_t r = 0; r < nD; r++)
    for (long long q = 0; q < lens[r]; q++)
      if (out[d_pos[r] + q] != in[d_src[r] + q]) fail(what + ": byte wrong", r, q, out[d_pos[r] + q]);
  for (long long q = total; q < total + 64; q++)
    if (out[q] != 0xA5) fail(what + ": byte written beyond the end", q, out[q]);
  free(d_pos), free(d_src), free(in), free(out);
}
/* random runs of 4 .. 300 bytes that add up to `total` (0 or >= 4) */
static std::vector<long long> runs_of(long long total) {
  std::vector<long long> lens;
  while (total >= 8) {
    const long long l = std::min<long long>(4 + rnd() % 297, total - 4);
    lens.push_back(l), total -= l;
  }
  if (total) lens.push_back(total);
  return lens;
}

// ---- the caps helpers, in the loop the two offsets kernels run them in, with two handed-over words ----
struct CapsOut {
  int32_t first, n_done, heads;
  long long bytes_done;
};
static void k_caps(int32_t ntiles, const int32_t* tile_cnt, const int32_t* tile_heads, const long long* tile_bytes, const int32_t* len,
                   int32_t cap_entries, long long cap_bytes, CapsOut* res) {
  int32_t run_c = 0, run_h = 0, cut = INT32_MAX, cut_x[2] = {0, 0};
  long long run_v = 0, cut_b = 0;
  for (int32_t t0 = 0; t0 < ntiles; t0 += GPX_BLOCK) {
    const int32_t t = t0 + (int32_t)threadIdx.x;
    const int32_t c = t < ntiles ? tile_cnt[t] : 0, h = t < ntiles ? tile_heads[t] : 0;
    const long long v = t < ntiles ? tile_bytes[t] : 0;
    const Scan64 S = block_scan64(c, h, v), H = block_scan64(h, 0, 0);
    const int32_t eo = run_c + S.ex_c, ho = run_h + H.ex_c;
    const long long bo = run_v + S.ex_v;
    if (t < ntiles && cut == INT32_MAX && caps_cut(c, v, eo, bo, cap_entries, cap_bytes)) cut = t, cut_x[0] = eo, cut_b = bo, cut_x[1] = ho;
    run_c += S.tot_c, run_h += S.tot_b, run_v += S.tot_v;
  }
  const int32_t first = caps_first_cut(cut, cut_b, cut_x);
  CapsOut r{first, run_c, run_h, run_v};
  if (first != INT32_MAX) {
    const int32_t l = len[(size_t)first * GPX_BLOCK + threadIdx.x]; /* -1: not an entry */
    const long long v = l >= 0 ? 4ll + l : 0ll;
    const bool done = caps_done(l >= 0, v, cut_x[0], cut_b, cap_entries, cap_bytes);
    const Scan64 D = block_scan64(done, 0, done ? v : 0ll);
    r = CapsOut{first, cut_x[0] + D.tot_c, cut_x[1], cut_b + D.tot_v};
  }
  res[threadIdx.x] = r; /* every lane reports: the answers are the same in all of them */
}
struct CapsTable { /* 258 tiles of records, about half of them entries; tile 3 has none */
  int32_t ntiles = 258, n_entries = 0;
  int32_t *len, *tile_cnt, *tile_heads;
  long long* tile_bytes;
  std::vector<long long> start; /* per entry, and the total behind the last */
  std::vector<int32_t> tile_of, eoff, hoff;
  CapsTable() {
    len = blk<int32_t>((size_t)ntiles * GPX_BLOCK, 0), tile_cnt = blk<int32_t>(ntiles, 0), tile_heads = blk<int32_t>(ntiles, 0);
    tile_bytes = blk<long long>(ntiles, 0);
    long long pos = 0;
    int32_t heads = 0;
    for (int32_t t = 0; t < ntiles; t++) {
      eoff.push_back(n_entries), hoff.push_back(heads);
      heads += tile_heads[t] = (int32_t)(rnd() % 9);
      for (int32_t q = 0; q < GPX_BLOCK; q++) {
        const bool sel = t != 3 && (q == 0 || q == GPX_BLOCK - 1 || rnd() % 2);
        const int32_t l = len[(size_t)t * GPX_BLOCK + q] = sel ? (int32_t)(rnd() % 40) : -1;
        if (!sel) continue;
        start.push_back(pos), tile_of.push_back(t);
        pos += 4 + l, n_entries++, tile_cnt[t]++, tile_bytes[t] += 4 + l;
      }
    }
    start.push_back(pos);
  }
  /* the caps as given; want: the entries done, by the plain rule */
  void run(const std::string& what, int32_t cap_entries, long long cap_bytes, int32_t want) const {
    int32_t done = 0;
    while (done < n_entries && done < cap_entries && start[done + 1] <= cap_bytes) done++;
    if (done != want) fail(what + ": the test's own caps", done, want);
    CapsOut* res = blk<CapsOut>(GPX_BLOCK, 0xA5);
    launch(1, [&] { k_caps(ntiles, tile_cnt, tile_heads, tile_bytes, len, cap_entries, cap_bytes, res); });
    const bool cutting = done < n_entries;
    const int32_t first = cutting ? tile_of[done] : INT32_MAX;
    for (int32_t l = 0; l < GPX_BLOCK; l++) {
      const CapsOut& r = res[l];
      if (r.first != first || r.n_done != done || r.bytes_done != start[done]) fail(what, l, r.first, r.n_done);
      if (r.heads != (cutting ? hoff[first] : hoff.back() + tile_heads[ntiles - 1])) fail(what + ": the second handed-over word", l, r.heads);
    }
    free(res);
  }
  /* a cut by entries and a cut by bytes in front of entry e */
  void cut_at(const std::string& what, int32_t e) const {
    run(what + ", by entries", e, LLONG_MAX, e);
    run(what + ", by bytes", INT32_MAX, start[e + 1] - 1, e); /* one byte short of entry e's end */
    run(what + ", by both", e, start[e + 1] - 1, e);
  }
  ~CapsTable() { free(len), free(tile_cnt), free(tile_heads), free(tile_bytes); }
};

int main() {
  for (int32_t n : {0, 1, 63, 64, 65, 4096, 4097}) wave_search_case(n);
  printf("wave_search: ok\n");
  for (int32_t n : {1, 2, 255, 256}) lds_search_case(n);
  printf("lds_search: ok\n");
  for (uint32_t align = 0; align < 4; align++) load4_case(8, align), load4_case(align ? 12 : 4, align);
  printf("load4_unaligned: ok\n");

  for (int k = 1; k <= 2; k++)
    for (int d = -5; d <= 5; d++) copy_case("copy_runs: total 16384 * " + std::to_string(k) + " + " + std::to_string(d), runs_of(16384ll * k + d), 3);
  {
    /* several rounds, each cut by the `hi` rule: 4,097 runs of 4 bytes from byte 0, and behind a run that puts them at
     * 2 mod 4 and into the second tile, which then overlaps 4,097 descriptors */
    std::vector<long long> lens(4097, 4);
    copy_case("copy_runs: 4,097 runs of 4 bytes", lens, 3);
    lens.insert(lens.begin(), 16382);
    copy_case("copy_runs: 4,097 descriptors in a tile", lens, 3);
  }
  copy_case("copy_runs: one run over three tiles", {5, 3 * 16384 + 100, 7}, 3);
  for (int m = 1; m <= 15; m++) {
    copy_case("copy_runs: tail of " + std::to_string(m), {7, 13, 28 + m}, 1);
    if (m >= 4) copy_case("copy_runs: a call of " + std::to_string(m) + " bytes", {m}, 1);
  }
  copy_case("copy_runs: 5 tiles on a grid of 2", runs_of(5 * 16384 - 3), 2);
  copy_case("copy_runs: total 0", {}, 2);
  printf("copy_runs: ok\n");

  {
    const CapsTable T;
    for (int32_t t : {0, 257}) {
      const int32_t e0 = T.eoff[t], c = T.tile_cnt[t];
      T.cut_at("caps: the first entry of tile " + std::to_string(t), e0);
      T.cut_at("caps: a middle entry of tile " + std::to_string(t), e0 + c / 2);
      T.cut_at("caps: the last entry of tile " + std::to_string(t), e0 + c - 1);
    }
    T.cut_at("caps: behind a tile without entries", T.eoff[4]);
    T.run("caps: nothing cut, exact", T.n_entries, T.start.back(), T.n_entries);
    T.run("caps: nothing cut, wide", INT32_MAX, LLONG_MAX, T.n_entries);
    T.run("caps: nothing fits", 0, 0, 0);
  }
  printf("caps: ok\n");
  return 0;
}
