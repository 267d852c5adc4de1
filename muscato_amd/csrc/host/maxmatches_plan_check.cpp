// maxmatches_plan_check.cpp -- the decisions of the MaxMatches replay stage that need no device
// (csrc/maxmatches_plan.hpp: the refusal bound, the heap's place) and the literal qinsert the kernel runs, stand-alone
// and under the sanitizers: muscato_amd/build.py (CHECKS) builds it, plain and sanitized.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "../maxmatches_plan.hpp"
#include "check.hpp"

// k_mm_replay's insertion (the new entry travels up in a register, parents move down) on a host array of exactly
// MaxMatches + 1 entries: the sanitizer sees every index
static uint32_t qinsert_hole(std::vector<std::pair<uint32_t, uint32_t>>& heap, uint32_t size, uint32_t max_matches, uint32_t mm, uint32_t idx) {
  uint32_t ii = size;
  while (ii > 0) {
    const uint32_t jj = (ii - 1) >> 1;
    if (heap.at(jj).first <= mm) break;
    heap.at(ii) = heap.at(jj);
    ii = jj;
  }
  heap.at(ii) = {mm, idx};
  return size + 1 > max_matches ? max_matches : size + 1;
}

// cmd/muscato_confirm/main.go:424-448 as apply_maxmatches of cli_maxmatches_host.hpp writes it: append, swap up, cut
static void qinsert_literal(std::vector<std::pair<uint32_t, uint32_t>>& q, uint32_t max_matches, uint32_t mm, uint32_t idx) {
  q.push_back({mm, idx});
  size_t ii = q.size() - 1;
  while (ii > 0) {
    const size_t jj = (ii - 1) / 2;
    if (q[jj].first > q[ii].first) { std::swap(q[jj], q[ii]); ii = jj; } else break;
  }
  if (q.size() > max_matches) q.resize(max_matches);
}

int main() {
  using namespace musc_mm;
  // the refusal bound: reads of 255 bases and up to the bound are taken, one base more is not
  EXPECT(refusal(Shape{255, 20, 1000, 10}) == nullptr);
  EXPECT(refusal(Shape{MAX_READ_LEN, 20, 0, 0}) == nullptr);
  EXPECT(refusal(Shape{MAX_READ_LEN + 1, 20, 1000, 10}) != nullptr);
  EXPECT(refusal(Shape{100, 0, 1000, 10}) != nullptr);
  EXPECT(refusal(Shape{100, (int32_t)MAX_READ_LEN, 1000, 10}) == nullptr);
  EXPECT(refusal(Shape{100, (int32_t)MAX_READ_LEN + 1, 1000, 10}) != nullptr);
  EXPECT(refusal(Shape{100, 20, -1, 10}) != nullptr);
  EXPECT(refusal(Shape{100, 20, 0x7FFFFFFF, MAX_TUPLES - 1}) == nullptr);
  EXPECT(refusal(Shape{100, 20, 1000, MAX_TUPLES}) != nullptr);
  static_assert(MAX_READ_LEN >= 255, "the bound may not lie below reads of 255 bases");
  // the LDS knob only lowers the capacity
  EXPECT(heap_lds_entries(0) == HEAP_LDS_ENTRIES && heap_lds_entries(-5) == HEAP_LDS_ENTRIES);
  EXPECT(heap_lds_entries(1) == 1 && heap_lds_entries(4095) == 4095 && heap_lds_entries(1L << 40) == HEAP_LDS_ENTRIES);
  // MaxMatches + 1 entries must fit
  EXPECT(heap_in_lds(0, 1) && !heap_in_lds(1, 1) && heap_in_lds(4095, 4096) && !heap_in_lds(4096, 4096));
  EXPECT(!heap_in_lds(0x7FFFFFFF, HEAP_LDS_ENTRIES));
  // the two insertions keep the same array, entry for entry
  std::mt19937 rng(7);
  for (uint32_t mm : {0u, 1u, 2u, 3u, 6u, 63u, 64u, 65u}) {
    for (int trial = 0; trial < 20; trial++) {
      std::vector<std::pair<uint32_t, uint32_t>> hole(mm + 1), lit;
      uint32_t size = 0;
      const uint32_t n = mm + 1 + rng() % 200;
      for (uint32_t i = 0; i < n; i++) {
        const uint32_t v = rng() % 5;
        size = qinsert_hole(hole, size, mm, v, i);
        qinsert_literal(lit, mm, v, i);
        EXPECT(size == lit.size());
        for (uint32_t j = 0; j < size; j++) EXPECT(hole[j] == lit[j]);
      }
    }
  }
  return check_done("maxmatches_plan_check");
}
