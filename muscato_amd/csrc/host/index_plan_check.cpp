// index_plan_check.cpp -- the decisions of the index layer (csrc/index_plan.hpp: table shapes, memory estimates, the
// cascade context -> line -> 64-byte buckets, the partition cuts) against their properties and a recorded decision
// table, as a program of its own so that it runs under the sanitizers.
// It needs no GPU and is not part of the library; muscato_amd/build.py (CHECKS) builds it, plain and sanitized.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../index_plan.hpp"
#include "check.hpp"

namespace {

namespace mi = musc_index;

// ---- the partition cuts

std::vector<uint64_t> offsets_of(const std::vector<uint64_t>& len) {
  std::vector<uint64_t> off(len.size() + 1, 0);  // (exactly nseq + 1 words: a read past either end is an error under the address sanitizer)
  for (size_t i = 0; i < len.size(); i++) off[i + 1] = off[i] + len[i];
  return off;
}

// the ranges tile [0, nseq]; `largest` is the largest; a range of several targets holds at most `limit` bases; and the
// cut is greedy: a range could not have taken the next target too
void check_cut(const std::vector<uint64_t>& off, uint64_t limit) {
  const uint32_t nseq = (uint32_t)off.size() - 1;
  std::vector<uint32_t> first;
  uint64_t largest = 0;
  const bool ok = mi::cut_targets(off, limit, &first, &largest);
  EXPECT(!first.empty() && first[0] == 0);
  uint64_t seen = 0;
  for (size_t p = 0; p + 1 < first.size(); p++) {
    const uint32_t g0 = first[p], g1 = first[p + 1];
    EXPECT(g0 < g1 && g1 <= nseq);  // no gap, no empty range, never past the last target
    if (g0 >= g1 || g1 > nseq) return;
    const uint64_t bases = off[g1] - off[g0];
    seen = std::max(seen, bases);
    EXPECT(bases <= limit || g1 == g0 + 1);
    if (g1 < nseq) EXPECT(off[g1 + 1] - off[g0] > std::min(limit, off[nseq]));  // the next target did not fit
  }
  if (ok) {
    EXPECT(first.back() == nseq);
    EXPECT(first.size() - 1 <= mi::MAX_PARTITIONS);
    EXPECT(largest == seen);
  } else {
    EXPECT(first.size() - 1 > mi::MAX_PARTITIONS);  // refused, and only then
  }
}

void check_fewest(const std::vector<uint64_t>& off, uint64_t room, bool monotone) {
  auto fits = [&](uint64_t bases) { return bases <= room; };
  std::vector<uint32_t> first;
  uint64_t largest = 0;
  const uint32_t n = mi::fewest_partitions(off, fits, &first, &largest);
  if (n) {  // the plan fits and covers
    EXPECT(n >= 2 && n <= mi::MAX_PARTITIONS);
    EXPECT(fits(largest));
    EXPECT(first.size() >= 2 && first[0] == 0 && first.back() == off.size() - 1);
    uint64_t seen = 0;
    for (size_t p = 0; p + 1 < first.size(); p++) {
      EXPECT(first[p] < first[p + 1]);
      seen = std::max(seen, off[first[p + 1]] - off[first[p]]);
    }
    EXPECT(seen == largest);
  }
  if (!monotone) return;
  uint32_t lin = 0;  // equal targets: the fit is monotone in the share count, so the search finds what a scan from 2 finds
  for (uint32_t k = 2; k <= mi::MAX_PARTITIONS && !lin; k++) {
    std::vector<uint32_t> f;
    uint64_t lg = 0;
    if (mi::cut_targets(off, (off.back() + k - 1) / k, &f, &lg) && fits(lg)) lin = k;
  }
  EXPECT(n == lin);
}

// ---- the decisions

// One row: the knobs (MUSC_INDEX as 0 auto, 1 classic, 2 lines, 3 classic64; MUSC_DEBUG_INDEX_BITS; MUSC_DEBUG_CTX_DIRECT;
// MUSC_DEBUG_INDEX_BUDGET_MB), the request, the memory, and what the cascade answers.  Where nothing fits (fits = 0) the
// kind is the window-start kind that was tried last.
struct Row {
  int index, index_bits, ctx_direct;
  long budget_mb;
  int ww, ctx_ok, wide;
  uint64_t bases, avail, extra;
  int need_fit;
  uint32_t kind;
  int bits, direct, fits;
};

// Recorded from the functions this header replaced (the two table-shape functions, the three memory estimates and the
// planner's copy of the cascade in muscato_hip.hip), before they went: their behaviour, which the cascade must
// reproduce row for row.
const Row RECORDED[] = {
    // window-start table: 4^ww against 32 * max(bases, 2^19); 2 * ww of 30 and 32; the 31-bit cap
    {0, 0, 0, 0, 12, 0, 0, 1000ull, 274877906944ull, 0ull, 1, /* -> */ 0, 24, 1, 1},
    {0, 0, 0, 0, 13, 0, 0, 1000ull, 274877906944ull, 0ull, 1, /* -> */ 0, 10, 0, 1},
    {0, 0, 0, 0, 12, 0, 0, 524288ull, 274877906944ull, 0ull, 1, /* -> */ 0, 24, 1, 1},
    {0, 0, 0, 0, 13, 0, 0, 524288ull, 274877906944ull, 0ull, 1, /* -> */ 0, 19, 0, 1},
    {0, 0, 0, 0, 13, 0, 0, 2097151ull, 274877906944ull, 0ull, 1, /* -> */ 0, 21, 0, 1},
    {0, 0, 0, 0, 13, 0, 0, 2097152ull, 274877906944ull, 0ull, 1, /* -> */ 0, 26, 1, 1},
    {0, 0, 0, 0, 15, 0, 0, 33554431ull, 274877906944ull, 0ull, 1, /* -> */ 0, 25, 0, 1},
    {0, 0, 0, 0, 15, 0, 0, 33554432ull, 274877906944ull, 0ull, 1, /* -> */ 0, 30, 1, 1},
    {0, 0, 0, 0, 16, 0, 0, 33554432ull, 274877906944ull, 0ull, 1, /* -> */ 0, 25, 0, 1},
    {0, 0, 0, 0, 16, 0, 0, 17179869184ull, 274877906944ull, 0ull, 1, /* -> */ 0, 31, 0, 0},
    {0, 0, 0, 0, 16, 0, 0, 2147483653ull, 274877906944ull, 0ull, 1, /* -> */ 0, 31, 0, 1},
    {0, 0, 0, 0, 16, 0, 0, 2147483648ull, 274877906944ull, 0ull, 1, /* -> */ 0, 31, 0, 1},
    {0, 0, 0, 0, 16, 0, 0, 1073741825ull, 274877906944ull, 0ull, 1, /* -> */ 0, 31, 0, 1},
    // context table: 4^ww against 2 * max(bases, 2^9); 2 * ww of 30 and 32; the 30-bit cap; wide buckets
    {0, 0, 0, 0, 5, 1, 0, 100ull, 274877906944ull, 0ull, 1, /* -> */ 1, 10, 1, 1},
    {0, 0, 0, 0, 6, 1, 0, 100ull, 274877906944ull, 0ull, 1, /* -> */ 1, 10, 0, 1},
    {0, 0, 0, 0, 6, 1, 0, 2047ull, 274877906944ull, 0ull, 1, /* -> */ 1, 11, 0, 1},
    {0, 0, 0, 0, 6, 1, 0, 2048ull, 274877906944ull, 0ull, 1, /* -> */ 1, 12, 1, 1},
    {0, 0, 0, 0, 15, 1, 0, 536870911ull, 274877906944ull, 0ull, 1, /* -> */ 1, 29, 0, 1},
    {0, 0, 0, 0, 15, 1, 0, 536870912ull, 274877906944ull, 0ull, 1, /* -> */ 1, 30, 1, 1},
    {0, 0, 0, 0, 15, 1, 1, 536870912ull, 274877906944ull, 0ull, 1, /* -> */ 2, 30, 1, 1},
    {0, 0, 0, 0, 16, 1, 0, 536870912ull, 274877906944ull, 0ull, 1, /* -> */ 1, 29, 0, 1},
    {0, 0, 0, 0, 16, 1, 0, 2147483653ull, 274877906944ull, 0ull, 1, /* -> */ 1, 30, 0, 1},
    {0, 0, 0, 0, 16, 1, 1, 1073741825ull, 274877906944ull, 0ull, 1, /* -> */ 2, 30, 0, 1},
    {0, 0, 0, 0, 16, 1, 0, 1073741824ull, 274877906944ull, 0ull, 1, /* -> */ 1, 30, 0, 1},
    // MUSC_DEBUG_INDEX_BITS of 7, 8, 30, 31 and 32, on both tables; MUSC_DEBUG_CTX_DIRECT
    {0, 7, 0, 0, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 3, 20, 1, 1},
    {0, 7, 0, 0, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 1, 20, 1, 1},
    {0, 7, 0, 0, 10, 1, 1, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 2, 20, 1, 1},
    {0, 8, 0, 0, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 8, 0, 1},
    {0, 8, 0, 0, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 1, 8, 0, 1},
    {0, 8, 0, 0, 10, 1, 1, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 2, 8, 0, 1},
    {0, 30, 0, 0, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 30, 0, 1},
    {0, 30, 0, 0, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 1, 30, 0, 1},
    {0, 30, 0, 0, 10, 1, 1, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 2, 30, 0, 1},
    {0, 31, 0, 0, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 31, 0, 1},
    {0, 31, 0, 0, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 1, 20, 1, 1},
    {0, 31, 0, 0, 10, 1, 1, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 2, 20, 1, 1},
    {0, 32, 0, 0, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 3, 20, 1, 1},
    {0, 32, 0, 0, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 1, 20, 1, 1},
    {0, 32, 0, 0, 10, 1, 1, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 2, 20, 1, 1},
    {0, 0, 0, 0, 10, 1, 0, 1000ull, 274877906944ull, 0ull, 1, /* -> */ 1, 10, 0, 1},
    {0, 0, 1, 0, 10, 1, 0, 1000ull, 274877906944ull, 0ull, 1, /* -> */ 1, 20, 1, 1},
    {0, 0, 1, 0, 16, 1, 0, 1000ull, 274877906944ull, 0ull, 1, /* -> */ 1, 10, 0, 1},
    {0, 8, 1, 0, 10, 1, 0, 1000ull, 274877906944ull, 0ull, 1, /* -> */ 1, 8, 0, 1},
    {0, 0, 1, 0, 10, 0, 0, 1000ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 1},
    // line buckets: bases just below and at 4 * nb; a hashed table; bits 30 against 31; memory for the 2^30-line table or not
    {0, 0, 0, 0, 10, 0, 0, 4194303ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 0, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 3, 20, 1, 1},
    {0, 20, 0, 0, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 0, 1},
    {0, 0, 0, 0, 15, 0, 0, 4294967296ull, 274877906944ull, 0ull, 1, /* -> */ 3, 30, 1, 1},
    {0, 0, 0, 0, 15, 0, 0, 4294967296ull, 214748364800ull, 0ull, 1, /* -> */ 0, 30, 1, 1},
    {0, 0, 0, 0, 15, 0, 0, 4294967295ull, 274877906944ull, 0ull, 1, /* -> */ 0, 30, 1, 1},
    {0, 0, 0, 0, 13, 0, 0, 1073741824ull, 274877906944ull, 0ull, 1, /* -> */ 3, 26, 1, 1},
    {0, 0, 0, 0, 13, 0, 0, 1073741824ull, 13958643712ull, 0ull, 1, /* -> */ 0, 26, 1, 0},
    {0, 0, 0, 0, 13, 0, 0, 1073741824ull, 32212254720ull, 0ull, 1, /* -> */ 0, 26, 1, 1},
    {2, 30, 0, 0, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 3, 30, 0, 1},
    {2, 31, 0, 0, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 31, 0, 1},
    {2, 0, 0, 0, 16, 0, 0, 8589934592ull, 274877906944ull, 0ull, 1, /* -> */ 0, 31, 0, 0},
    // each forced MUSC_INDEX (classic, lines, classic64), on a database the automatic choice gives lines and one it does not
    {0, 0, 0, 0, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 3, 20, 1, 1},
    {0, 0, 0, 0, 10, 0, 0, 1000ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 0, 16, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 22, 0, 1},
    {1, 0, 0, 0, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 3, 20, 1, 1},
    {1, 0, 0, 0, 10, 0, 0, 1000ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 1},
    {1, 0, 0, 0, 16, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 22, 0, 1},
    {2, 0, 0, 0, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 3, 20, 1, 1},
    {2, 0, 0, 0, 10, 0, 0, 1000ull, 274877906944ull, 0ull, 1, /* -> */ 3, 20, 1, 1},
    {2, 0, 0, 0, 16, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 3, 22, 0, 1},
    {3, 0, 0, 0, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 1},
    {3, 0, 0, 0, 10, 0, 0, 1000ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 1},
    {3, 0, 0, 0, 16, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 22, 0, 1},
    {2, 0, 0, 100, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 3, 20, 1, 0},
    {2, 0, 0, 100, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 0, /* -> */ 3, 20, 1, 1},
    {3, 0, 0, 100, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 0},
    // a budget that admits each kind in turn and none (ww 10, 2^22 bases: context 193.3 MiB, lines 200.0004 MiB,
    // 64-byte buckets 144.0001 MiB), context eligible or not, wide or not; then the same with fit = false
    {0, 0, 0, 1, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 0},
    {0, 0, 0, 1, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 0},
    {0, 0, 0, 144, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 0},
    {0, 0, 0, 144, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 0},
    {0, 0, 0, 145, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 145, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 193, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 193, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 194, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 194, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 1, 20, 1, 1},
    {0, 0, 0, 200, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 200, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 1, 20, 1, 1},
    {0, 0, 0, 201, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 3, 20, 1, 1},
    {0, 0, 0, 201, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 1, 20, 1, 1},
    {0, 0, 0, 220, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 3, 20, 1, 1},
    {0, 0, 0, 220, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 1, 20, 1, 1},
    {0, 0, 0, 300, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 3, 20, 1, 1},
    {0, 0, 0, 300, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 1, 20, 1, 1},
    {0, 0, 0, 194, 10, 1, 1, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 219, 10, 1, 1, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 3, 20, 1, 1},
    {0, 0, 0, 220, 10, 1, 1, 4194304ull, 274877906944ull, 0ull, 1, /* -> */ 3, 20, 1, 1},
    {0, 0, 0, 1, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 0, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 1, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 0, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 144, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 0, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 144, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 0, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 194, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 0, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 194, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 0, /* -> */ 1, 20, 1, 1},
    {0, 0, 0, 201, 10, 0, 0, 4194304ull, 274877906944ull, 0ull, 0, /* -> */ 3, 20, 1, 1},
    {0, 0, 0, 201, 10, 1, 0, 4194304ull, 274877906944ull, 0ull, 0, /* -> */ 1, 20, 1, 1},
    // the reserves (context 4 GiB, lines 12 GiB, 64-byte buckets 4 GiB) and a non-zero extra reserve, no budget
    {0, 0, 0, 0, 10, 1, 0, 4194304ull, 4557111296ull, 0ull, 1, /* -> */ 1, 20, 1, 1},
    {0, 0, 0, 0, 10, 1, 0, 4194304ull, 4557111296ull, 58720256ull, 1, /* -> */ 1, 20, 1, 1},
    {0, 0, 0, 0, 10, 1, 0, 4194304ull, 4557111296ull, 59768832ull, 1, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 0, 10, 1, 0, 4194304ull, 4557111296ull, 104857600ull, 1, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 0, 10, 1, 0, 4194304ull, 4557111296ull, 111149056ull, 1, /* -> */ 0, 20, 1, 0},
    {0, 0, 0, 0, 10, 1, 0, 4194304ull, 4557111296ull, 112197632ull, 1, /* -> */ 0, 20, 1, 0},
    {0, 0, 0, 0, 10, 0, 0, 4194304ull, 13147045888ull, 0ull, 1, /* -> */ 3, 20, 1, 1},
    {0, 0, 0, 0, 10, 0, 0, 4194304ull, 13147045888ull, 52428800ull, 1, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 0, 10, 0, 0, 4194304ull, 13147045888ull, 53477376ull, 1, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 0, 10, 0, 0, 4194304ull, 13147045888ull, 8701083648ull, 1, /* -> */ 0, 20, 1, 0},
    {0, 0, 0, 0, 10, 0, 0, 4194304ull, 13147045888ull, 8702132224ull, 1, /* -> */ 0, 20, 1, 0},
    {0, 0, 0, 0, 10, 0, 0, 4194304ull, 13147045888ull, 8702132224ull, 0, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 0, 10, 1, 0, 4194304ull, 0ull, 0ull, 1, /* -> */ 0, 20, 1, 0},
    {0, 0, 0, 0, 10, 1, 0, 4194304ull, 0ull, 5ull, 0, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 300, 10, 1, 0, 4194304ull, 4557111296ull, 104857600ull, 1, /* -> */ 0, 20, 1, 1},
    {0, 0, 0, 100, 10, 1, 0, 4194304ull, 274877906944ull, 8589934592ull, 1, /* -> */ 0, 20, 1, 0},
};

// Computed by hand from the formulas: ww 15, 116 182 bases, context eligible and narrow, 15 MiB (15 728 640 B).  The
// context table is hashed with 2^17 buckets and needs 131 073 * 140 + 38 727 * 40 = 19 899 300 B: it does not fit.
// The window-start table is hashed too, so lines are out.  64-byte buckets need 131 073 * 80 + 116 182 * 16 =
// 12 344 752 B and fit.
const Row BY_HAND = {0, 0, 0, 15, 15, 1, 0, 116182ull, 274877906944ull, 0ull, 1, /* -> */ 0, 17, 0, 1};

void check_row(const Row& r) {
  mi::Knobs k;
  k.index = r.index;
  k.index_bits = r.index_bits;
  k.ctx_direct = r.ctx_direct != 0;
  k.index_budget_mb = r.budget_mb;
  const mi::Plan p = mi::cascade(k, r.ww, r.ctx_ok != 0, r.wide != 0, r.bases, r.avail, r.extra, r.need_fit != 0);
  const bool same = p.kind == r.kind && p.bits == r.bits && p.direct == r.direct && p.fits == (r.fits != 0);
  if (!same)
    fprintf(stderr, "row {%d, %d, %d, %ld, %d, %d, %d, %llu, %llu, %llu, %d}: got %u %d %d %d, recorded %u %d %d %d\n", r.index,
            r.index_bits, r.ctx_direct, r.budget_mb, r.ww, r.ctx_ok, r.wide, (unsigned long long)r.bases, (unsigned long long)r.avail,
            (unsigned long long)r.extra, r.need_fit, p.kind, p.bits, p.direct, (int)p.fits, r.kind, r.bits, r.direct, r.fits);
  EXPECT(same);
  // the table of the plan is the one table_for names, and a plan that says it fits does by the estimate
  const mi::Table t = mi::table_for(k, mi::is_ctx(p.kind), r.ww, r.bases);
  EXPECT(t.bits == p.bits && t.direct == p.direct);
  if (r.need_fit || mi::is_ctx(p.kind)) EXPECT(p.fits == mi::index_fits(k, p.kind, p.bits, r.bases, r.avail, r.extra));
}

}  // namespace

int main() {
  // cuts by hand: empty targets, one target longer than the limit, limit 1, a limit beyond the database
  for (uint64_t limit : {1ull, 2ull, 5ull, 9ull, 10ull, 1000ull}) {
    check_cut(offsets_of({0}), limit);
    check_cut(offsets_of({7}), limit);
    check_cut(offsets_of({0, 0, 0}), limit);
    check_cut(offsets_of({3, 0, 0, 9, 0, 1, 1, 5, 0}), limit);
    check_cut(offsets_of({5, 5, 5, 5}), limit);
  }
  check_cut(offsets_of(std::vector<uint64_t>(mi::MAX_PARTITIONS, 3)), 3);      // exactly MAX_PARTITIONS ranges
  check_cut(offsets_of(std::vector<uint64_t>(mi::MAX_PARTITIONS + 1, 3)), 3);  // one more: refused
  check_cut(offsets_of(std::vector<uint64_t>(3 * mi::MAX_PARTITIONS, 1)), 1);
  std::mt19937_64 rng(31);
  for (int round = 0; round < 4000; round++) {
    const size_t n = round % 5 == 0 ? 1 + rng() % 3 : 1 + rng() % 200;
    const uint64_t limit = round % 7 == 0 ? 1 : 1 + rng() % (round % 3 ? 64 : 4096);
    std::vector<uint64_t> len(n);
    for (auto& l : len) {
      const unsigned k = (unsigned)(rng() % 8);
      l = k < 2 ? 0 : k < 6 ? rng() % (limit + 1) : k == 6 ? limit + 1 + rng() % (3 * limit) : rng() % 5;
    }
    check_cut(offsets_of(len), limit);
  }
  // the fewest partitions: equal targets (monotone) against the linear scan, ragged ones for fit and cover, a room
  // that nothing fits (one long target) and one that needs more than MAX_PARTITIONS shares
  for (int round = 0; round < 60; round++) {
    const size_t n = 2 + rng() % (round % 2 ? 40 : 1500);
    const uint64_t each = 1 + rng() % 50;
    const std::vector<uint64_t> off = offsets_of(std::vector<uint64_t>(n, each));
    check_fewest(off, each * (1 + rng() % n), true);
    check_fewest(off, each, true);
    if (round % 10 == 0) check_fewest(off, each - 1, true);  // (nothing fits: 0)
    std::vector<uint64_t> len(n);
    for (auto& l : len) l = rng() % 4 ? rng() % 100 : rng() % 3000;
    check_fewest(offsets_of(len), 1 + rng() % 5000, false);
  }
  for (const Row& r : RECORDED) check_row(r);
  check_row(BY_HAND);
  EXPECT(mi::index_need(mi::K_CTX, 17, 116182) == 19899300ull);
  EXPECT(mi::index_need(mi::K_CLASSIC64, 17, 116182) == 12344752ull);
  EXPECT(BY_HAND.kind == mi::K_CLASSIC64 && BY_HAND.bits == 17 && BY_HAND.direct == 0 && BY_HAND.fits == 1);
  return check_done("index_plan_check");
}
