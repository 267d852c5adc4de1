// text_stage.hpp -- how a range of rendered records is cut into pieces that pass through the bounded device staging
// buffer on their way to a host destination.  Plain C++, no HIP: included by muscato_text.hpp and by
// host/text_stage_check.cpp, the stand-alone program that runs it under the sanitizers.
#pragma once

#include <algorithm>
#include <cstdint>

namespace musc_text {

// off[0 .. n] are the byte offsets of the n records of a window (they do not decrease; record i = bytes [off[i],
// off[i + 1])), p < n the first record of a piece.  Returns the piece's end: the most records whose bytes fit `stage`,
// at least one (a record larger than the stage goes alone: the caller grows the buffer), never past the window.
inline uint64_t stage_piece_end(const uint64_t* off, uint64_t n, uint64_t p, uint64_t stage) {
  const uint64_t fit = (uint64_t)(std::upper_bound(off + p, off + n + 1, off[p] + stage) - off) - 1;
  return std::min(std::max(fit, p + 1), n);
}

}  // namespace musc_text
