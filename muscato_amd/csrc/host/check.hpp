// check.hpp -- what the stand-alone check programs (host/*_check.cpp) share: the two counters, EXPECT, its form with a
// message, and the one way a main ends.  Plain C++17, nothing but <cstdio>.  A failed check prints where it stands, is
// counted, and the program goes on: one run shows every rule that broke.
// muscato_amd/build.py (CHECKS) builds the programs, plain with the tools and with AddressSanitizer and UBSan for the
// suite (tests/test_check_programs.py).
#pragma once

#include <cstdio>

inline long long failures = 0;    // checks that did not hold
inline long long checks_run = 0;  // checks evaluated
constexpr long long CHECK_PRINT_CAP = 20;  // EXPECT_MSG prints while fewer than this many checks have failed

#define EXPECT(cond)                                              \
  do {                                                            \
    checks_run++;                                                 \
    if (!(cond)) {                                                \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      failures++;                                                 \
    }                                                             \
  } while (0)

// ... with a printf-style message that says which case it was (its arguments are evaluated on failure only).  For the
// checks inside long loops: every failure is counted, the first CHECK_PRINT_CAP are printed.
#define EXPECT_MSG(cond, ...)                                            \
  do {                                                                   \
    checks_run++;                                                        \
    if (!(cond)) {                                                       \
      if (failures < CHECK_PRINT_CAP) {                                  \
        fprintf(stderr, "%s:%d: %s -- ", __FILE__, __LINE__, #cond);     \
        fprintf(stderr, __VA_ARGS__);                                    \
        fputc('\n', stderr);                                             \
      }                                                                  \
      failures++;                                                        \
    }                                                                    \
  } while (0)

// the end of every main: "NAME: F of N checks failed" on stderr and 1, or the one stdout line "NAME: N checks passed"
// (with " (extra)" behind it: the census of what the program went through) and 0
inline int check_done(const char* name, const char* extra = nullptr) {
  if (failures) {
    fprintf(stderr, "%s: %lld of %lld checks failed\n", name, failures, checks_run);
    return 1;
  }
  if (extra) printf("%s: %lld checks passed (%s)\n", name, checks_run, extra);
  else printf("%s: %lld checks passed\n", name, checks_run);
  return 0;
}
