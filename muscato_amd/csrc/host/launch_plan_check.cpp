// launch_plan_check.cpp -- csrc/launch_plan.hpp as a program of its own, so that it runs under the sanitizers: the grid
// of a stage launch under its cap and under MUSC_DEBUG_STAGE_GRID, held to the expressions the drivers used before
// they shared one function; the scratch plan of the scans' host recursion, walked level by level for sizes up to 2^40;
// and the recursion itself replayed on the host into a scratch of exactly scan_tmp_elems(n) elements, held to a
// running sum.
// It needs no GPU and is not part of the library; muscato_amd/build.py (CHECKS) builds it, plain and sanitized.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../launch_plan.hpp"
#include "check.hpp"

using namespace musc_launch;

namespace {

// ---------------------------------------------------------------- stage_blocks

// what each family of launches computed before stage_blocks, written out again (MAX_GRID was 4096u).  The forms
// without a max(1, ..) were launched with wanted > 0 only.
constexpr unsigned OLD_MAX_GRID = 4096u;
unsigned old_nblk(uint64_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }
unsigned old_grid(uint64_t k) { return std::max(1u, std::min(old_nblk(k, 256), OLD_MAX_GRID)); }              // grid(k)
unsigned old_tiles(uint64_t w) { return (unsigned)std::min<uint64_t>(w, 4 * OLD_MAX_GRID); }                   // L->tgrid, the renders
unsigned old_part(uint64_t items) { return std::min(old_nblk(items, 256), 4u * OLD_MAX_GRID); }                // the partition kernels
unsigned old_chunks(uint64_t w) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(w, 8 * OLD_MAX_GRID)); }  // k_sz_frame (k_sz_decode: no max)
unsigned old_replay(uint32_t nb) { return std::min<uint32_t>(nb, 65536u); }                                    // k_mm_replay
unsigned old_index(uint64_t bases) { return (unsigned)std::min<uint64_t>((bases + 255) / 256, 1u << 22); }     // k_index

void check_stage_blocks() {
  const uint64_t caps[] = {CAP_GRID, CAP_TILES, CAP_CHUNKS, CAP_REPLAY, CAP_INDEX};
  for (const uint64_t cap : caps) {
    const uint64_t wanted[] = {0, 1, cap - 1, cap, cap + 1, 0xFFFFFFFFull};
    const uint64_t knobs[] = {0, 1, 3, cap + 1};
    for (const uint64_t w : wanted)
      for (const uint64_t k : knobs) {
        const unsigned b = stage_blocks(w, cap, k);
        EXPECT_MSG(b >= 1, "wanted %llu cap %llu knob %llu", (unsigned long long)w, (unsigned long long)cap, (unsigned long long)k);
        if (w) EXPECT_MSG(b <= w, "wanted %llu cap %llu knob %llu -> %u", (unsigned long long)w, (unsigned long long)cap, (unsigned long long)k, b);
        if (k) EXPECT_MSG(b <= k, "wanted %llu cap %llu knob %llu -> %u", (unsigned long long)w, (unsigned long long)cap, (unsigned long long)k, b);
        else EXPECT_MSG(b == std::max<uint64_t>(1, std::min<uint64_t>(w, cap)), "wanted %llu cap %llu -> %u", (unsigned long long)w, (unsigned long long)cap, b);
        // (a knob is the whole grid where the launch wants at least that much: the loop is crossed as the test means it to be)
        if (k && w >= k) EXPECT(b == k);
      }
  }
  // a knob beyond a dispatch's 32 bits counts as KNOB_MAX: the grid never wraps, and never to 0
  const uint64_t big_knobs[] = {KNOB_MAX, KNOB_MAX + 1, 1ull << 32, (1ull << 32) + 3, ~0ull};
  const uint64_t big_wanted[] = {1, KNOB_MAX, KNOB_MAX + 1, 1ull << 32, ~0ull};
  for (const uint64_t k : big_knobs)
    for (const uint64_t w : big_wanted) {
      const unsigned b = stage_blocks(w, CAP_GRID, k);
      EXPECT_MSG(b == (w < KNOB_MAX ? w : KNOB_MAX), "wanted %llu knob %llu -> %u", (unsigned long long)w, (unsigned long long)k, b);
    }
  // the same wanted values as the drivers form them, against each family's own expression of before
  auto wanted_of = [](uint64_t cap, int i) -> uint64_t {
    const uint64_t w[] = {0, 1, cap - 1, cap, cap + 1, 0xFFFFFFFFull};
    return w[i];
  };
  for (int i = 0; i < 6; i++) {
    // grid(k): k items, one block per 256; every k that rounds up to the wanted count
    const uint64_t wg = wanted_of(CAP_GRID, i);
    for (const uint64_t k : {wg * 256, wg ? wg * 256 - 255 : 0, wg ? wg * 256 - 1 : 0})
      EXPECT_MSG(stage_blocks((k + 255) / 256, CAP_GRID, 0) == old_grid(k), "grid(%llu)", (unsigned long long)k);
    const uint64_t wt = wanted_of(CAP_TILES, i);
    if (wt) {
      EXPECT(stage_blocks(wt, CAP_TILES, 0) == old_tiles(wt));
      EXPECT(stage_blocks(old_nblk(wt * 256, 256), CAP_TILES, 0) == old_part(wt * 256));
      EXPECT(stage_blocks(old_nblk(wt * 256 - 255, 256), CAP_TILES, 0) == old_part(wt * 256 - 255));
      EXPECT(stage_blocks(old_nblk(wt * 16, 16), CAP_TILES, 0) == std::min(old_nblk(wt * 16, 16), 4 * OLD_MAX_GRID));  // k_fq_gather
    }
    // (the renders: bytes / 256 + 1 blocks, never 0)
    EXPECT(stage_blocks((wt * 256) / 256 + 1, CAP_TILES, 0) == old_tiles((wt * 256) / 256 + 1));
    const uint64_t wc = wanted_of(CAP_CHUNKS, i);
    EXPECT(stage_blocks(wc, CAP_CHUNKS, 0) == old_chunks(wc));
    const uint64_t wr = wanted_of(CAP_REPLAY, i);
    if (wr) EXPECT(stage_blocks(wr, CAP_REPLAY, 0) == old_replay((uint32_t)wr));
    const uint64_t wi = wanted_of(CAP_INDEX, i);
    if (wi) {
      EXPECT(stage_blocks((wi * 256 + 255) / 256, CAP_INDEX, 0) == old_index(wi * 256));
      EXPECT(stage_blocks((wi * 256 - 255 + 255) / 256, CAP_INDEX, 0) == old_index(wi * 256 - 255));
    }
  }
}

// ---------------------------------------------------------------- the scan plan

// scan_tmp_elems as the library had it before it moved
uint64_t old_scan_tmp_elems(uint64_t n) {
  uint64_t t = 0;
  while (n > 2048) {
    n = (n + 2048 - 1) / 2048;
    t += (n + 8 + 3) & ~3ull;
  }
  return t + 8;
}

struct Level {
  uint64_t off, nb;  // the level's sums: nb elements at `off` elements into the scratch
};

// the carve of scan_levels, without the kernels: a level of more than one tile puts its sums at the front of what it
// was given and hands the rest, from scan_next_level(nb) on, to the level that scans them
std::vector<Level> walk(uint64_t n) {
  std::vector<Level> L;
  uint64_t off = 0;
  for (;;) {
    const uint64_t nb = scan_tiles(n);
    if (nb <= 1) return L;
    L.push_back(Level{off, nb});
    off += scan_next_level(nb);
    n = nb;
  }
}

const uint64_t T1 = SCAN_TILE_ELEMS, T2 = T1 * T1, T3 = T2 * T1;
const uint64_t PLAN_N[] = {0, 1, T1 - 1, T1, T1 + 1, T2 - 1, T2, T2 + 1, T3 - 1, T3 + 1, 1ull << 40};

void check_scan_plan() {
  EXPECT(SCAN_TILE_ELEMS == 2048);
  for (const uint64_t n : PLAN_N) {
    const uint64_t total = scan_tmp_elems(n);
    EXPECT_MSG(total == old_scan_tmp_elems(n), "n %llu", (unsigned long long)n);
    EXPECT(scan_tiles(n) == (n + 2047) / 2048);
    const std::vector<Level> L = walk(n);
    // the number of levels with sums: one per factor of 2048 above the first
    const size_t want_levels = n <= T1 ? 0 : n <= T2 ? 1 : n <= T3 ? 2 : 3;
    EXPECT_MSG(L.size() == want_levels, "n %llu: %zu levels", (unsigned long long)n, L.size());
    for (const uint64_t es : {(uint64_t)4, (uint64_t)8}) {
      uint64_t prev_end = 0;
      for (size_t k = 0; k < L.size(); k++) {
        const uint64_t b0 = L[k].off * es, b1 = (L[k].off + L[k].nb) * es;
        EXPECT_MSG(b1 <= total * es, "n %llu level %zu: [%llu, %llu) of %llu bytes", (unsigned long long)n, k, (unsigned long long)b0,
                   (unsigned long long)b1, (unsigned long long)(total * es));
        EXPECT_MSG(b0 >= prev_end, "n %llu level %zu overlaps the one before", (unsigned long long)n, k);
        // (scan_load8 / scan_store8 move a uint4 of u32; the u64 kernels move single elements)
        EXPECT_MSG(b0 % (es == 4 ? 16 : 8) == 0, "n %llu level %zu starts at byte %llu", (unsigned long long)n, k, (unsigned long long)b0);
        EXPECT(k == 0 ? L[k].nb == scan_tiles(n) : L[k].nb == scan_tiles(L[k - 1].nb));
        prev_end = b1;
      }
    }
    if (!L.empty()) EXPECT(scan_tiles(L.back().nb) == 1);  // the last level's sums fit one tile: the recursion ends
  }
}

// ---------------------------------------------------------------- the recursion, replayed

// scan_levels with the kernels' work done by loops: the tile-wise scan of the level (`inclusive` at the top level of a
// u32 scan, exclusive below and for u64), the tiles' sums into tmp, the next level over them in place, the add-back.
// in may equal out: an element is read before its place is written, as a lane does.
template <class T>
void replay(const T* in, T* out, uint64_t n, T* tmp, bool inclusive) {
  const uint64_t nb = scan_tiles(n);
  T* const sums = nb <= 1 ? nullptr : tmp;
  for (uint64_t b = 0; b < (nb ? nb : 1); b++) {
    T run = 0;
    const uint64_t e = std::min(n, (b + 1) * SCAN_TILE_ELEMS);
    for (uint64_t i = b * SCAN_TILE_ELEMS; i < e; i++) {
      const T x = in[i];
      out[i] = inclusive ? (T)(run + x) : run;
      run = (T)(run + x);
    }
    if (sums) sums[b] = run;
  }
  if (!sums) return;
  replay<T>(sums, sums, nb, tmp + scan_next_level(nb), false);
  for (uint64_t i = 0; i < n; i++) out[i] = (T)(out[i] + sums[i / SCAN_TILE_ELEMS]);
}

constexpr uint64_t GUARD = 16;

template <class T>
void check_replay(uint64_t n, bool inclusive, bool in_place, T value_mask, uint64_t seed) {
  const uint64_t elems = scan_tmp_elems(n);
  // heap blocks of exactly the sizes the library allocates (a step past one is the address sanitizer's to report), the
  // scratch with GUARD marked elements behind it (a step past it is reported in a plain run too)
  T* const in = (T*)malloc((n ? n : 1) * sizeof(T));
  T* const out = in_place ? in : (T*)malloc((n ? n : 1) * sizeof(T));
  T* const tmp = (T*)malloc((elems + GUARD) * sizeof(T));
  std::vector<T> src(n);
  std::mt19937_64 rng(seed);
  for (uint64_t i = 0; i < n; i++) in[i] = src[i] = (T)(rng() & value_mask);
  const T mark = (T)0xA5A5A5A5A5A5A5A5ull;
  for (uint64_t i = 0; i < elems + GUARD; i++) tmp[i] = mark;
  replay<T>(in, out, n, tmp, inclusive);
  uint64_t run = 0;  // the model: one running sum, wider than any total here
  for (uint64_t i = 0; i < n; i++) {
    if (inclusive) run += src[i];
    EXPECT_MSG((uint64_t)out[i] == run, "n %llu%s%s element %llu", (unsigned long long)n, inclusive ? " inclusive" : "", in_place ? " in place" : "",
               (unsigned long long)i);
    if (!inclusive) run += src[i];
  }
  if (!in_place)
    for (uint64_t i = 0; i < n; i++) EXPECT_MSG(in[i] == src[i], "n %llu: input element %llu changed", (unsigned long long)n, (unsigned long long)i);
  for (uint64_t i = 0; i < GUARD; i++) EXPECT_MSG(tmp[elems + i] == mark, "n %llu: guard element %llu written", (unsigned long long)n, (unsigned long long)i);
  // every level's sums were written, and nothing between the levels was
  const std::vector<Level> L = walk(n);
  std::vector<char> used(elems, 0);
  for (const Level& l : L)
    for (uint64_t i = 0; i < l.nb; i++) used[l.off + i] = 1;
  uint64_t stray = 0;
  for (uint64_t i = 0; i < elems; i++) stray += !used[i] && tmp[i] != mark;
  EXPECT_MSG(stray == 0, "n %llu: %llu scratch elements outside the levels written", (unsigned long long)n, (unsigned long long)stray);
  free(tmp);
  if (!in_place) free(out);
  free(in);
}

void check_replays() {
  uint64_t seed = 1;
  for (const uint64_t n : PLAN_N) {
    if (n > T2 + 1) continue;
    for (const bool in_place : {false, true}) {
      // u32: values of two bits, so that no total here passes 2^32 (the model's sum is compared whole)
      check_replay<uint32_t>(n, false, in_place, 3u, seed++);
      check_replay<uint32_t>(n, true, in_place, 3u, seed++);
      // u64: values of 30 bits, totals far beyond 2^32
      check_replay<uint64_t>(n, false, in_place, (1ull << 30) - 1, seed++);
    }
  }
}

}  // namespace

int main() {
  check_stage_blocks();
  check_scan_plan();
  check_replays();
  return check_done("launch_plan_check");
}
