// maxmatches_plan.hpp -- the plain-C++ decisions of the MaxMatches replay stage: which shapes the device
// stage takes, and where k_mm_replay keeps a block's heap.  No HIP in here: included by muscato_maxmatches.hpp and by
// host/maxmatches_plan_check.cpp, the stand-alone program that runs it under the sanitizers.
#pragma once

#include <cstdint>

namespace musc_mm {

constexpr uint32_t MAX_READ_LEN = 1024;      // = MUSC_MM_MAX_READ_LEN of the header: longest loaded read the stage takes
constexpr uint32_t HEAP_LDS_ENTRIES = 4096;  // (mm, pair) entries of 8 bytes: 32 KiB of a workgroup's LDS
constexpr uint64_t MAX_TUPLES = 0xFFFFFFF0ull;  // a pair names its tuple in 32 bits
constexpr uint64_t MAX_BLOCKS = 0x3FFFFFFEull;  // a (tuple, window) word names its block in 30 bits

// The shape of a call.  Everything the refusal looks at, and nothing else.
struct Shape {
  uint32_t max_len;       // longest loaded read
  int32_t window_width;
  int32_t max_matches;
  uint64_t ntuples;
};

// nullptr: the stage takes the shape; else why not (code 12)
inline const char* refusal(const Shape& s) {
  if (s.max_len > MAX_READ_LEN) return "a loaded read is longer than MUSC_MM_MAX_READ_LEN bases";
  if (s.window_width < 1 || (uint32_t)s.window_width > MAX_READ_LEN) return "WindowWidth is outside 1..MUSC_MM_MAX_READ_LEN";
  if (s.max_matches < 0) return "MaxMatches is negative";
  if (s.ntuples >= MAX_TUPLES) return "too many tuples for 32-bit pair entries";
  return nullptr;
}

// LDS entries the replay may use: MUSC_DEBUG_MM_HEAP_LDS (tests) lowers the compiled capacity, never raises it
inline uint32_t heap_lds_entries(long knob) {
  if (knob <= 0) return HEAP_LDS_ENTRIES;
  return knob < (long)HEAP_LDS_ENTRIES ? (uint32_t)knob : HEAP_LDS_ENTRIES;
}

// the heap of a truncated block holds at most MaxMatches + 1 entries (the append before the cut)
inline bool heap_in_lds(int32_t max_matches, uint32_t lds_entries) {
  return (uint64_t)max_matches + 1 <= (uint64_t)lds_entries;
}

}  // namespace musc_mm
