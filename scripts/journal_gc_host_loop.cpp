// What a host does today to compact a log file, for scripts/bench_journal_gc.py: compactLogfile's loop
// (SQLPaxosLogger.java:3375-3408) on one thread - walk the file entry by entry (readInt, readFully into a fresh array),
// look the entry's threshold up, and write the needed ones, prefix and bytes, to the new file (here: one growing
// std::vector).  The Java also parses every entry back into a packet to learn its group and slot; this loop is handed
// both (the rows, in file order) and so is the faster of the two.  Returns the bytes kept; *sum is a checksum so that
// nothing is elided.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

extern "C" long long journal_gc_host_loop(const uint8_t* file, long long bytes, const int32_t* e_gidx, const int32_t* e_slot,
                                          const int32_t* gc_slot, unsigned long long* sum) {
  std::vector<uint8_t> tmp;
  long long pos = 0;
  int i = 0;
  while (pos < bytes) {
    const uint32_t len = (uint32_t)file[pos] << 24 | (uint32_t)file[pos + 1] << 16 | (uint32_t)file[pos + 2] << 8 | file[pos + 3];
    std::vector<uint8_t> msg(file + pos + 4, file + pos + 4 + len); /* byte[] msg = new byte[length]; raf.readFully(msg) */
    if ((int32_t)((uint32_t)e_slot[i] - (uint32_t)gc_slot[e_gidx[i]]) > 0) {
      for (int sft = 24; sft >= 0; sft -= 8) tmp.push_back((uint8_t)(len >> sft));
      tmp.insert(tmp.end(), msg.begin(), msg.end());
    }
    pos += 4 + (long long)len;
    i++;
  }
  unsigned long long s = 0;
  for (size_t q = 0; q < tmp.size(); q += 4096) s += tmp[q];
  *sum = s + (tmp.empty() ? 0 : tmp.back());
  return (long long)tmp.size();
}
