// read_names_keys.hpp -- the order of the members of the larger groups (above WAVE_GROUP_MAX) as integer keys, for a
// stable LSD radix sort of plain uint64_t keys.  Plain C++ that g++ compiles without HIP and hipcc
// compiles for the device (RN_HD), as read_names_lanes.hpp, whose name_word it calls.  No function here talks to another
// lane, and the one loop has a constant bound (GROUP_STEPS).
//
// The order is PairLess's (read_names_lanes.hpp): group, then the clipped name bytewise with a proper prefix first,
// then the kept-read number.  As keys, from the least significant pass to the most:
//
//   1. sortkey_tail   clipped_len << 32 | kept read                                   (42 bits)
//   2. sortkey_word   name_word(w) for w = W - 1 ... 0, W = key_words(max clipped_len of the pairs) (64 bits each)
//   3. sortkey_group  the group number                                                (32 bits)
//
// W + 2 stable passes leave the pairs ordered by (group, word 0, ..., word W - 1, clipped_len, kept read).  Why that is
// PairLess's order: a name's words past its clipped end are 0 (and load nothing), and W covers the longest name, so the
// W words are every byte of both names, zero-padded.  If a word differs, take the first: when it lies inside the shorter
// name's words, the bytewise compare finds the same first difference (a 0x00 of the padding against a byte of the
// longer name is the prefix rule, or loses to any non-zero byte as it must); when it lies behind them, the longer name
// holds a non-zero byte there against padding and stands behind, which is what its length says too.  If all W words are
// equal, the names agree over the shorter one's length and the longer one holds only 0x00 bytes behind it -- the
// shorter is a prefix, or the names are equal -- so clipped_len decides, and between equal names the kept-read number,
// which is file order.  The kept-read number is part of the last key, so no two pairs have all keys equal: the result
// is a function of the set of pairs and does not depend on the order in which they enter the first pass.
//
// W = 0 (every name of the larger groups is empty) is sortkey_tail and sortkey_group alone.  The caller clamps what it
// read back with key_words before it loops: at most CMP_WORDS + 2 passes whatever the device said.
#pragma once

#include <cstdint>

#include "read_names_lanes.hpp"

namespace musc_rn {

// the compare words that the longest clipped name among the pairs has, never more than CMP_WORDS
RN_HD uint32_t key_words(uint64_t max_clipped_len) {
  const uint64_t w = (max_clipped_len + 7) / 8;
  return w < CMP_WORDS ? (uint32_t)w : CMP_WORDS;
}
RN_HD uint32_t key_passes(uint64_t max_clipped_len) { return key_words(max_clipped_len) + 2; }

constexpr uint32_t TAIL_BITS = 42, GROUP_BITS = 32;  // the bits of sortkey_tail (1000 < 2^10) and sortkey_group that can be set

template <class Pair>
RN_HD uint64_t sortkey_tail(const Names& N, const Pair& p) {
  return (uint64_t)clipped_len(N.name_len[p.y]) << 32 | p.y;
}
template <class R, class Pair>
RN_HD uint64_t sortkey_word(const R& rd, const Names& N, const Pair& p, uint32_t w) {
  return name_word(rd, N.name_off[p.y], N.name_len[p.y], w);
}
template <class Pair>
RN_HD uint64_t sortkey_group(const Pair& p) {
  return p.x;
}

// The key of pair perm[k] for pass `pass` of key_passes: 0 = the tail, 1 ... W = word W - pass, W + 1 = the group.
template <class R, class Pair>
RN_HD uint64_t sortkey(const R& rd, const Names& N, const Pair* pairs, const uint32_t* perm, uint64_t k, uint32_t pass, uint32_t W) {
  const Pair p = pairs[perm[k]];
  if (pass == 0) return sortkey_tail(N, p);
  if (pass > W) return sortkey_group(p);
  return sortkey_word(rd, N, p, W - pass);
}

// After the last pass perm[k] = the pair that stands at place k of the order; the pairs were made in group order and the
// order keeps the groups apart, so it belongs where pair k of the unsorted list came from (unpairs_item, through perm).
template <class Pair>
RN_HD void unpairs_by_perm(const Pair* pairs, const uint32_t* perm, const uint32_t* place, uint64_t k, uint32_t* ranked) {
  ranked[place[k]] = pairs[perm[k]].y;
}

// The group of place i: the g with ustart[g] <= i < ustart[g + 1], for i < ustart[nu] and ustart[0] = 0 (nu >= 1).
constexpr uint32_t GROUP_STEPS = 32;
RN_HD uint32_t place_group(const uint32_t* ustart, uint32_t nu, uint64_t i) {
  uint32_t lo = 0, hi = nu;  // ustart[lo] <= i < ustart[hi]
  for (uint32_t it = 0; it < GROUP_STEPS; it++) {
    if (hi - lo <= 1) break;
    const uint32_t mid = lo + (hi - lo) / 2;
    if (ustart[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace musc_rn
