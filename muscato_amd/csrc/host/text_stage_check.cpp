// text_stage_check.cpp -- the staging plan of the text calls (csrc/text_stage.hpp: how a window of records is cut into
// pieces that fit the staging buffer) against a brute-force model, as a program of its own so that it runs under the
// sanitizers.
// It needs no GPU and is not part of the library; muscato_amd/build.py (CHECKS) builds it, plain and sanitized.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../text_stage.hpp"
#include "check.hpp"

namespace {

// the model: the first record whatever its size, then records one by one while the sum still fits (after an oversize
// record nothing does, not even an empty one)
uint64_t model_end(const std::vector<uint64_t>& len, uint64_t p, uint64_t stage) {
  uint64_t q = p + 1, sum = len[p];
  while (q < len.size() && sum + len[q] <= stage) sum += len[q++];
  return q;
}

// One window of records with these lengths, starting at byte `first` of the text.  The offsets live in a heap block of
// exactly n + 1 words: a read past either end is an error under the address sanitizer.
void check(const std::vector<uint64_t>& len, uint64_t first, uint64_t stage) {
  const uint64_t n = len.size();
  std::vector<uint64_t> off(n + 1);
  off[0] = first;
  for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + len[i];
  uint64_t p = 0, pieces = 0;
  while (p < n) {
    const uint64_t q = musc_text::stage_piece_end(off.data(), n, p, stage);
    EXPECT(q > p);   // at least one record
    EXPECT(q <= n);  // never past the window
    if (q <= p || q > n) return;
    const uint64_t bytes = off[q] - off[p];
    EXPECT(bytes <= stage || q == p + 1);  // fits, or is a single oversize record
    EXPECT(q == model_end(len, p, stage));
    p = q;  // (the next piece starts where this one ends: the pieces tile the window when the loop ends at n)
    pieces++;
  }
  EXPECT(p == n);
  EXPECT(pieces <= n);
}

}  // namespace

int main() {
  // by hand: empty records around an oversize one, an exact fit, a stage of one byte
  check({0}, 0, 1);
  check({5}, 7, 1);
  check({0, 0, 0}, 3, 1);
  check({0, 5, 0, 0, 1, 1, 0}, 0, 1);
  check({4, 4, 4, 4}, 100, 8);
  check({4, 4, 1, 4}, 100, 8);
  check({9, 0, 9, 0}, 0, 8);
  std::mt19937_64 rng(29);
  for (int round = 0; round < 20000; round++) {
    const int kind = round % 4;
    const uint64_t n = kind == 0 ? 1 : kind == 1 ? 2 : 3 + rng() % (kind == 2 ? 12 : 300);
    const uint64_t stage = round % 7 == 0 ? 1 : 1 + rng() % (round % 3 ? 64 : 4096);
    std::vector<uint64_t> len(n);
    for (auto& l : len) {
      const unsigned k = (unsigned)(rng() % 8);
      l = k < 2 ? 0 : k < 6 ? rng() % (stage + 1) : k == 6 ? stage + 1 + rng() % (3 * stage) : rng() % 5;
    }
    check(len, rng() % 3 ? rng() % (1ull << 40) : 0, stage);
  }
  return check_done("text_stage_check");
}
