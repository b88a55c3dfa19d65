// What the project's own logger writes for a handful of frames: gpx::FileLogger (gigapaxos_amd/host/gpx_host.cpp) logs
// frames of 0, 1, 3, 4, 5 and 70,000 bytes to the file named on the command line and waits until they are durable.
// tests/test_journal_abi.py compares the file with tests/journal_model.py: the model is pinned to FileLogger::logBatch.
// Frame f holds the bytes (f * 31 + q * 7 + 1) mod 251, q = 0, 1, ...
#include <chrono>
#include <cstdio>
#include <thread>
#include <vector>

#include "../gigapaxos_amd/host/gpx_host.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const int lens[] = {0, 1, 3, 4, 5, 70000};
  std::vector<gpx::Frame> frames;
  for (int f = 0; f < 6; f++) {
    gpx::Frame fr((size_t)lens[f]);
    for (int q = 0; q < lens[f]; q++) fr[(size_t)q] = (uint8_t)((f * 31 + q * 7 + 1) % 251);
    frames.push_back(fr);
  }
  std::vector<const gpx::Frame*> recs;
  for (const gpx::Frame& fr : frames) recs.push_back(&fr);
  {
    gpx::FileLogger log(argv[1]);
    const uint64_t t = log.logBatch(recs);
    for (int spin = 0; log.durable() < t && !log.failed() && spin < 20000; spin++)
      std::this_thread::sleep_for(std::chrono::milliseconds(1));
    if (log.failed() || log.durable() < t) return 1;
  }
  printf("logged %zu frames\n", frames.size());
  return 0;
}
