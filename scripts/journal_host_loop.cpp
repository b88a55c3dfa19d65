// What a host does today for a log batch, for scripts/bench_journal_pack.py: FileLogger::logBatch's loop
// (gigapaxos_amd/host/gpx_host.cpp) - per record four push_backs of the length and one insert of the frame into one
// std::vector - over host-resident frames, for the records whose status and r_flags (copied back from the device by the
// caller) say they must be logged.  One thread.  Returns the bytes built; *sum is a checksum so that nothing is elided.
#include <cstddef>
#include <cstdint>
#include <vector>

extern "C" long long journal_host_loop(int n, const uint8_t* frames, const long long* frame_off, const uint8_t* r_flags,
                                       const uint8_t* status, unsigned long long* sum) {
  std::vector<uint8_t> bytes;
  for (int i = 0; i < n; i++) {
    if (status[i] != 0 || !(r_flags[i] & 1)) continue;
    const uint8_t* f = frames + frame_off[i];
    const uint32_t len = (uint32_t)(frame_off[i + 1] - frame_off[i]);
    for (int sft = 24; sft >= 0; sft -= 8) bytes.push_back((uint8_t)(len >> sft));
    bytes.insert(bytes.end(), f, f + len);
  }
  unsigned long long s = 0;
  for (size_t q = 0; q < bytes.size(); q += 4096) s += bytes[q];
  *sum = s + (bytes.empty() ? 0 : bytes.back());
  return (long long)bytes.size();
}
