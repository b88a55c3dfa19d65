// What a host does today to keep the log index, for scripts/bench_logindex.py: paxosutil/LogIndex.java restated over
// per-group vectors, one thread - add (LogIndex.java:192-204), setGCSlot / GC (:128-152), getLoggedAccepts (:213-237)
// and the walk over every group that getLogfiles / getMinLogfile / FileIDMap.isRemovable need.  The Java keeps a map by
// name, boxed Integers and a String per entry; this loop is handed group numbers and file ids and so is the faster of
// the two.
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {
struct Entry {
  int32_t slot, bnum, bcoord, file;
  long long off;
  int32_t len;
};
struct Index {
  int32_t gc = -1, min_file = -1;
  std::vector<Entry> log;
};
struct Map {
  std::vector<Index> of;
};
inline int32_t diff(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
}  // namespace

extern "C" {

void* li_new(int32_t groups) {
  Map* m = new Map;
  m->of.resize(groups);
  return m;
}
void li_free(void* h) { delete (Map*)h; }

long long li_add(void* h, int32_t n, const int32_t* g, const int32_t* slot, const int32_t* bnum, const int32_t* bcoord,
                 const long long* off, const int32_t* len, int32_t file) {
  Map& m = *(Map*)h;
  long long added = 0;
  for (int32_t i = 0; i < n; i++) {
    Index& x = m.of[g[i]];
    if (diff(slot[i], x.gc) <= 0) continue;
    if (x.min_file == -1) x.min_file = file;
    x.log.push_back(Entry{slot[i], bnum[i], bcoord[i], file, off[i], len[i]});
    added++;
  }
  return added;
}

long long li_set_gc(void* h, int32_t n, const int32_t* g, const int32_t* gc) {
  Map& m = *(Map*)h;
  long long died = 0;
  for (int32_t i = 0; i < n; i++) {
    Index& x = m.of[g[i]];
    x.gc = gc[i];
    size_t w = 0;
    for (size_t r = 0; r < x.log.size(); r++)
      if (diff(x.log[r].slot, x.gc) > 0) x.log[w++] = x.log[r];
    died += (long long)(x.log.size() - w);
    x.log.resize(w);
    x.min_file = w ? x.log[0].file : -1;
  }
  return died;
}

/* getLoggedAccepts for a batch; the hits' offsets go to o_off (cap entries), a checksum of the rest to *sum */
long long li_lookup(void* h, int32_t n, const int32_t* g, const int32_t* lo, const int32_t* hi, const uint8_t* has_max,
                    long long cap, long long* o_off, int32_t* o_len, unsigned long long* sum) {
  Map& m = *(Map*)h;
  long long hits = 0;
  unsigned long long s = 0;
  for (int32_t i = 0; i < n; i++) {
    const Index& x = m.of[g[i]];
    for (const Entry& e : x.log)
      if (diff(e.slot, lo[i]) >= 0 && (!has_max || !has_max[i] || diff(e.slot, hi[i]) <= 0)) {
        if (hits < cap) o_off[hits] = e.off, o_len[hits] = e.len;
        s += (unsigned long long)e.file + (unsigned long long)e.bnum;
        hits++;
      }
  }
  *sum = s;
  return hits;
}

/* alive rows per file, groups per min file, the smallest min file: a walk over every group */
long long li_files(void* h, int32_t base, int32_t n_files, int32_t* o_rows, int32_t* o_groups, int32_t* o_min) {
  Map& m = *(Map*)h;
  long long outside = 0;
  int32_t lo = INT32_MAX;
  for (int32_t f = 0; f < n_files; f++) o_rows[f] = 0, o_groups[f] = 0;
  for (const Index& x : m.of) {
    for (const Entry& e : x.log) {
      const long long d = (long long)e.file - base;
      if (d >= 0 && d < n_files) o_rows[d]++;
      else outside++;
    }
    if (x.log.empty() || x.min_file == -1) continue;
    if (x.min_file < lo) lo = x.min_file;
    const long long d = (long long)x.min_file - base;
    if (d >= 0 && d < n_files) o_groups[d]++;
    else outside++;
  }
  *o_min = lo == INT32_MAX ? -1 : lo;
  return outside;
}

long long li_rows(void* h) {
  long long r = 0;
  for (const Index& x : ((Map*)h)->of) r += (long long)x.log.size();
  return r;
}

} /* extern "C" */
