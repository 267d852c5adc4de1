// launch_plan.hpp -- what the host drivers decide about a launch before they make it: the grid of a
// persistent stage kernel under its cap or under MUSC_DEBUG_STAGE_GRID, and the scratch plan of the scans' host
// recursion.  Plain C++, no HIP, no context: included by muscato_hip.hip and by host/launch_plan_check.cpp, the
// stand-alone program that holds it under the sanitizers.
#pragma once

#include <cstdint>

namespace musc_launch {

// The caps of the stage grids, in blocks.  A grid-stride kernel of 256 lanes takes CAP_GRID; the text tiles, k_fq_gather,
// the partition kernels and the renders four times that; the snappy chunk kernels eight times; k_mm_replay one
// workgroup per suspect block up to CAP_REPLAY; the index builds one block per 256 bases up to CAP_INDEX.
constexpr uint64_t CAP_GRID = 4096;  // MAX_GRID of kernels_common.hpp (muscato_hip.hip holds the two equal)
constexpr uint64_t CAP_TILES = 4 * CAP_GRID;
constexpr uint64_t CAP_CHUNKS = 8 * CAP_GRID;
constexpr uint64_t CAP_REPLAY = 65536;
constexpr uint64_t CAP_INDEX = 1ull << 22;

// the largest knob: what is read from the environment is clamped to it, so that a grid always fits a dispatch's 32 bits
constexpr uint64_t KNOB_MAX = 0x7FFFFFFFull;

// Blocks of a stage launch that wants `wanted` (one per 256 items, per tile, per chunk): at most `cap`, never none.
// knob = MUSC_DEBUG_STAGE_GRID (0: not set) takes the cap's place, so that a test crosses the kernel's loop on a small
// input; it never raises a grid above what the launch wants, and a knob above KNOB_MAX counts as KNOB_MAX.
inline unsigned stage_blocks(uint64_t wanted, uint64_t cap, uint64_t knob) {
  const uint64_t lim = knob ? (knob < KNOB_MAX ? knob : KNOB_MAX) : cap;
  const uint64_t b = wanted < lim ? wanted : lim;
  return (unsigned)(b ? b : 1);
}

// ---- the scans (scan_levels of muscato_hip.hip).  A level scans its n elements tile by tile; with more than one tile
// the tiles' sums go to the front of the scratch, are scanned in turn by the next level, whose scratch starts
// scan_next_level(nb) elements further on, and are added back.  A level of one tile takes no scratch.
constexpr uint64_t SCAN_TILE_ELEMS = 2048;  // SCAN_TILE of kernels_common.hpp (held equal there too)

inline uint64_t scan_tiles(uint64_t n) { return (n + SCAN_TILE_ELEMS - 1) / SCAN_TILE_ELEMS; }

// where the next level's scratch starts behind a level's nb sums: a multiple of four elements (16 bytes of u32, what
// scan_load8 and scan_store8 move at once)
inline uint64_t scan_next_level(uint64_t nb) { return (nb + 8 + 3) & ~3ull; }

// elements of scratch a scan of n elements takes, u32 or u64 alike
inline uint64_t scan_tmp_elems(uint64_t n) {
  uint64_t t = 0;
  while (n > SCAN_TILE_ELEMS) {
    n = scan_tiles(n);
    t += scan_next_level(n);
  }
  return t + 8;
}

}  // namespace musc_launch
