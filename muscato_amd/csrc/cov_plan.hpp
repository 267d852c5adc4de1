// cov_plan.hpp -- the size rules of the coverage stage: the weight of a line from its read's tail, the
// interval a line covers on the forward strand, the key of an event and the end bit of the event sort, the byte counts
// of a bedGraph record and of a summary record, and the refusal bounds.  Plain C++, usable on the host and on the
// device: included by kernels_cov.hpp, by host/cli_text.hpp (coverage_text, the host copy of the stage) and by
// host/cli_plan_check.cpp.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COV_HD __host__ __device__ inline
#else
#define COV_HD inline
#endif

/* the flags of musc_cov_prepare (include/muscato_cov.h states them for callers) */
#ifndef MUSC_COV_REV_PAIRS
#define MUSC_COV_REV_PAIRS 1u
#define MUSC_COV_WEIGHTED 2u
#define MUSC_COV_UNIQUE 4u
#endif

namespace musc_cov {

constexpr uint32_t ALL_FLAGS = MUSC_COV_REV_PAIRS | MUSC_COV_WEIGHTED | MUSC_COV_UNIQUE;
constexpr uint64_t WEIGHT_LIMIT = 1ull << 32;  // a weight saturates here; a total weight of this much or more is refused
constexpr uint64_t LINES_LIMIT = 1ull << 31;   // a list of this many lines or more is refused

COV_HD bool total_refused(uint64_t total_weight) { return total_weight >= WEIGHT_LIMIT; }
COV_HD bool lines_refused(uint64_t lines) { return lines >= LINES_LIMIT; }

COV_HD uint32_t ndigits(uint64_t v) {
  uint32_t n = 1;
  while (v >= 10u) {
    v /= 10u;
    n++;
  }
  return n;
}

// The weight of a line under MUSC_COV_WEIGHTED, from its read's tail (count \t names): the bytes before the first tab
// (the whole tail when it has none) as a decimal number when they are a non-empty string of digits, saturated at
// WEIGHT_LIMIT; 1 otherwise.  (Without a read text, and without the flag, the weight is 1: the caller's rule.)
COV_HD uint64_t weight(const unsigned char* p, uint64_t T) {
  uint64_t v = 0, i = 0;
  for (; i < T && p[i] != '\t'; i++) {
    const uint32_t d = (uint32_t)p[i] - (uint32_t)'0';
    if (d > 9u) return 1;
    v = v * 10u + d;  // (v <= 2^32 before the step: no overflow)
    if (v > WEIGHT_LIMIT) v = WEIGHT_LIMIT;
  }
  return i == 0 ? 1 : v;
}

// The interval [a, a + S) a line covers on the forward strand of target f: the tuple's (g, pos), len = bases of g (and
// of its partner: a pair of unequal lengths is refused), L = bases of the read.
struct Interval {
  uint32_t f;
  uint64_t a, S;
};
COV_HD Interval interval(bool rev_pairs, uint32_t g, uint64_t pos, uint64_t len, uint64_t L) {
  const uint64_t left = len - pos, S = L < left ? L : left;  // pos <= len: musc_results_order refuses the rest
  const bool rev = rev_pairs && (g & 1u);
  return Interval{rev ? g - 1u : g, rev ? len - pos - S : pos, S};
}

// The key of an event at base x of target f, 0 <= x <= len(f): every target owns len + 1 slots, so that the end of one
// target never meets base 0 of the next.
COV_HD uint64_t slot(uint64_t seq_off_f, uint32_t f, uint64_t x) { return seq_off_f + f + x; }

// The end bit of the event sort: the bit width of nbases + nseq, which is above every slot (at least one bit)
COV_HD unsigned sort_end_bit(uint64_t nbases, uint64_t nseq) {
  uint64_t v = nbases + nseq;
  unsigned b = 0;
  while (v) {
    v >>= 1;
    b++;
  }
  return b ? b : 1u;
}

// rname \t start \t end \t depth \n
COV_HD uint64_t run_bytes(uint32_t rname, uint64_t start, uint64_t end, uint32_t depth) {
  return (uint64_t)rname + 1 + ndigits(start) + 1 + ndigits(end) + 1 + ndigits(depth) + 1;
}

// rname \t len \t numreads \t covbases \t sumdepth \t maxdepth \n
COV_HD uint64_t summary_bytes(uint32_t rname, uint64_t len, uint32_t numreads, uint64_t covbases, uint64_t sumdepth, uint32_t maxdepth) {
  return (uint64_t)rname + 1 + ndigits(len) + 1 + ndigits(numreads) + 1 + ndigits(covbases) + 1 + ndigits(sumdepth) + 1 + ndigits(maxdepth) + 1;
}

}  // namespace musc_cov
