// read_names_lanes.hpp -- everything a lane of the read-name stage computes, in plain C++ that g++ compiles
// without HIP and hipcc compiles for the device (RN_HD): the compare word of a clipped name, the three-way compare of
// two names, the first-tab search, the rank of a member by counting, the token starts and sizes of a group, the byte at
// a place of a record and of a line, and the store shape of the render.  A kernel of the stage
// (kernels_read_names.hpp) is nothing but the index arithmetic that hands a lane its item and a call of one `*_item`
// function below, or of a function of read_names_keys.hpp, which orders the larger groups by integer keys in place of
// the comparison sort under PairLess (PairLess is the specification, run under std::sort in the check
// program only).  host/read_names_plan_check.cpp runs the functions item by item in grid order over seeded
// texts, through a reader that reports every load outside the text, and holds what they leave to the reference's
// string code byte for byte.
//
// No function here talks to another lane: no shuffle, no ballot, no shared memory, no barrier, no atomic.  Every loop
// has a bound that is a constant of the plan (CMP_WORDS, NAME_KEEP, WAVE_GROUP_MAX, JOIN_SCAN_MAX, SEARCH_STEPS, 10
// digits); the data only ends a loop sooner.  Every index product is 64-bit.
#pragma once

#include <cstdint>

#include "read_names_plan.hpp"

namespace musc_rn {

constexpr uint32_t CMP_WORDS = (NAME_KEEP + DOTS + 7) / 8;  // 125: the most 8-byte words a compare looks at
// The members of a group whose token starts can lie in front of the join's cut: every token adds at least its ';', so
// after JOIN_LIMIT + 2 of them the sum is above JOIN_LIMIT whatever they hold.
constexpr uint32_t JOIN_SCAN_MAX = JOIN_LIMIT + 2;
constexpr uint32_t START_SAT = JOIN_LIMIT + 1;  // a token start or a sum of this much or more is stored as this
constexpr uint32_t SEARCH_STEPS = 11;           // 2^10 < JOIN_SCAN_MAX <= 2^11: halvings of the token search

// The text as a device kernel reads it.  The check program has a reader of its own that counts a load with p >= nbytes.
struct TextBytes {
  const unsigned char* text;
  uint64_t nbytes;
  RN_HD uint32_t byte(uint64_t p) const { return text[p]; }
};

// what the stage reads of the kept reads (numbered in file order) and of the groups
struct Names {
  const uint64_t* name_off;  // [n] first byte of the name in the text
  const uint32_t* name_len;  // [n] its bytes after the \r rule, before the 1000-byte rule
  uint64_t n;                // the kept reads
};

// Bytes [8 w, 8 w + 8) of the clipped name, the first most significant: '.' for the virtual bytes, 0 past the clipped
// end.  Loads bytes [off, off + text_len) only.
template <class R>
RN_HD uint64_t name_word(const R& rd, uint64_t off, uint32_t name_len, uint32_t w) {
  const uint32_t tl = text_len(name_len), cl = clipped_len(name_len);
  uint64_t v = 0;
  for (uint32_t k = 0; k < 8; k++) {
    const uint32_t i = 8 * w + k;
    const uint32_t b = i < tl ? rd.byte(off + i) : i < cl ? (uint32_t)'.' : 0u;
    v = v << 8 | b;
  }
  return v;
}

// -1, 0, 1: the bytewise order of two clipped names, unsigned bytes, a proper prefix first.  A word can differ behind
// the shorter name's end only where the longer one holds a non-zero byte, which puts the longer one behind.
template <class R>
RN_HD int name_compare(const R& rd, uint64_t off_a, uint32_t len_a, uint64_t off_b, uint32_t len_b) {
  const uint32_t ca = clipped_len(len_a), cb = clipped_len(len_b);
  const uint32_t nw = ((ca < cb ? ca : cb) + 7) / 8;
  for (uint32_t w = 0; w < CMP_WORDS; w++) {
    if (w >= nw) break;
    const uint64_t x = name_word(rd, off_a, len_a, w), y = name_word(rd, off_b, len_b, w);
    if (x != y) return x < y ? -1 : 1;
  }
  return ca < cb ? -1 : ca > cb ? 1 : 0;
}

// kept read a stands in front of kept read b (a != b) within their group: by name, equal names in file order
template <class R>
RN_HD bool member_before(const R& rd, const Names& N, uint32_t a, uint32_t b) {
  const int d = name_compare(rd, N.name_off[a], N.name_len[a], N.name_off[b], N.name_len[b]);
  return d < 0 || (d == 0 && a < b);
}

// the place of the first tab among the bytes of the name that come from the text, or text_len when there is none
template <class R>
RN_HD uint32_t first_tab(const R& rd, uint64_t off, uint32_t name_len) {
  const uint32_t tl = text_len(name_len);
  for (uint32_t i = 0; i < NAME_LIMIT; i++) {
    if (i >= tl) break;
    if (rd.byte(off + i) == 9u) return i;
  }
  return tl;
}

// ---- measure: one item per kept read
template <class R>
RN_HD uint32_t measure_item(const R& rd, const Names& N, uint64_t i) {
  const uint32_t n = N.name_len[i];
  return meta_pack(clipped_len(n), token_len(n, first_tab(rd, N.name_off[i], n)));
}

// ---- rank: one item per place of the sorted order.  members = the count kept reads of the group in file order.
// The members in front of `me`, by counting (count <= WAVE_GROUP_MAX).
template <class R>
RN_HD uint32_t rank_by_count(const R& rd, const Names& N, const uint32_t* members, uint32_t count, uint32_t me) {
  uint32_t r = 0;
  for (uint32_t o = 0; o < WAVE_GROUP_MAX; o++) {
    if (o >= count) break;
    const uint32_t other = members[o];
    if (other != me && member_before(rd, N, other, me)) r++;
  }
  return r;
}

// Place i of the order belongs to group g = places [ustart[g], ustart[g + 1]).  Writes the member into its ranked place
// of `ranked` (a permutation within the group, so no two items write one place) and returns 0; a member of a group
// above WAVE_GROUP_MAX is left for the sort: it stays in its place and the item returns 1.
template <class R>
RN_HD uint32_t rank_item(const R& rd, const Names& N, const uint32_t* order, const uint32_t* ustart, uint32_t g, uint64_t i,
                         uint32_t* ranked) {
  const uint64_t s = ustart[g];
  const uint32_t count = ustart[g + 1] - ustart[g], me = order[i];
  const Path p = group_path(count);
  if (p == PATH_WAVE) {
    ranked[s + rank_by_count(rd, N, order + s, count, me)] = me;
    return 0;
  }
  ranked[i] = me;
  return p == PATH_SORTED ? 1u : 0u;
}

// The order of the (group, kept read) pairs of the larger groups, for a comparison sort over uint2-like pairs: group,
// name, kept-read number -- a strict total order.
template <class R, class Pair>
struct PairLess {
  R rd;
  Names N;
  RN_HD bool operator()(const Pair& a, const Pair& b) const {
    if (a.x != b.x) return a.x < b.x;
    // (a pair that is none of the stage's -- padding inside a sort -- loads nothing: by number)
    if (a.y == b.y || a.y >= N.n || b.y >= N.n) return a.y < b.y;
    return member_before(rd, N, a.y, b.y);
  }
};

// ---- the larger groups: one item per place.  flag[i] = what rank_item returned, excl = its exclusive scan: the k-th
// flagged place gives pair k = (group, kept read) and remembers where it stands ...
template <class Pair>
RN_HD void pairs_item(const uint32_t* flag, const uint32_t* excl, const uint32_t* order, uint32_t g, uint64_t i, Pair* pairs, uint32_t* place) {
  if (!flag[i]) return;
  Pair p;
  p.x = g;
  p.y = order[i];
  pairs[excl[i]] = p;
  place[excl[i]] = (uint32_t)i;
}
// ... and one item per sorted pair: the pairs were made in group order and the sort keeps the groups apart, so pair k
// of the sorted list belongs where pair k of the unsorted one came from
template <class Pair>
RN_HD void unpairs_item(const Pair* sorted, const uint32_t* place, uint64_t k, uint32_t* ranked) {
  ranked[place[k]] = sorted[k].y;
}

// ---- sizes: one item per group
struct GroupSizes {
  uint64_t record, line;  // bytes of count \t J and of seq \t count \t J \n
  uint32_t count, clipped;
};
// tstart[s + j] = where token j of the ranked group starts in the join, for j < min(count, JOIN_SCAN_MAX), saturated;
// gsum[g] = the join's length before the cut, saturated.
RN_HD GroupSizes sizes_item(const uint32_t* ranked, const uint32_t* ustart, const uint32_t* meta, const uint32_t* seq_len, uint64_t g,
                            uint32_t* tstart, uint32_t* gsum) {
  const uint64_t s = ustart[g];
  const uint32_t count = ustart[g + 1] - ustart[g];
  uint32_t sum = 0;  // (at most JOIN_SCAN_MAX * (NAME_LIMIT + 1))
  for (uint32_t j = 0; j < JOIN_SCAN_MAX; j++) {
    if (j >= count) break;
    tstart[s + j] = sum < START_SAT ? sum : START_SAT;
    sum += meta_tok(meta[ranked[s + j]]) + 1;
  }
  // (a group has a member; one with more than JOIN_SCAN_MAX has a sum above the limit already)
  const uint32_t total = sum - 1 < START_SAT ? sum - 1 : START_SAT;
  gsum[g] = total;
  GroupSizes z;
  z.count = count;
  z.clipped = join_clipped(total);
  z.record = record_len(count, total);
  z.line = line_len(seq_len[ranked[s]], count, total);
  return z;
}

// ---- the bytes
RN_HD uint32_t digit_char(uint32_t v, uint32_t width, uint32_t j) {  // digit j of v, the first the most significant
  uint32_t p = 1;
  for (uint32_t k = 0; k < 10; k++) {
    if (k + j + 1 >= width) break;
    p *= 10;
  }
  return (uint32_t)'0' + (v / p) % 10u;
}

struct Groups {
  const uint32_t* ranked;  // [n] the kept reads, group by group, in name order
  const uint32_t* ustart;  // [nu + 1]
  const uint32_t* meta;    // [n] by kept read
  const uint32_t* tstart;  // [n] by place
  const uint32_t* gsum;    // [nu]
};

// byte p of the record count \t J of group g, p < record_len
template <class R>
RN_HD uint32_t record_byte(const R& rd, const Names& N, const Groups& G, uint64_t g, uint64_t p) {
  const uint64_t s = G.ustart[g];
  const uint32_t count = G.ustart[g + 1] - G.ustart[g], sum = G.gsum[g];
  const uint32_t w = dec_width(count);
  if (p < w) return digit_char(count, w, (uint32_t)p);
  if (p == w) return 9u;
  const uint32_t q = (uint32_t)(p - w - 1);
  if (q >= join_text_len(sum)) return (uint32_t)'.';
  // the last token that starts at or in front of q: starts below the cut are not saturated and grow strictly
  uint32_t lo = 0, hi = count < JOIN_SCAN_MAX ? count : JOIN_SCAN_MAX;
  for (uint32_t it = 0; it < SEARCH_STEPS; it++) {
    if (hi - lo <= 1) break;
    const uint32_t mid = lo + (hi - lo) / 2;
    if (G.tstart[s + mid] <= q) lo = mid; else hi = mid;
  }
  const uint32_t r = G.ranked[s + lo], d = q - G.tstart[s + lo];
  if (d >= meta_tok(G.meta[r])) return (uint32_t)';';
  return virtual_byte(N.name_len[r], d) ? (uint32_t)'.' : rd.byte(N.name_off[r] + d);
}

// The loaded reads as the library keeps them: rw words a read, 16 bases a word at 2 bits (A C G T = 0 1 2 3), the last
// word = the length in its low 16 bits; rdm (null: no read holds an X) marks the bases that are none of the four.
struct Reads {
  const uint32_t* rd;
  const uint32_t* rdm;
  int rw;
};
RN_HD uint32_t read_len(const Reads& S, uint64_t g) { return S.rd[g * (uint64_t)S.rw + (uint64_t)(S.rw - 1)] & 0xFFFFu; }

// byte k of the line seq \t record \n of group g, k < line_len; the record is read from the rendered read text
RN_HD uint32_t line_byte(const Reads& S, const char* ttext, const uint64_t* toff, uint64_t g, uint64_t k) {
  const uint32_t L = read_len(S, g);
  const uint64_t t0 = toff[g], T = toff[g + 1] - t0;
  if (k < L) {
    const uint64_t b = g * (uint64_t)S.rw * 16ull + k;
    const uint32_t sh = 2u * ((uint32_t)b & 15u);
    if (S.rdm && ((S.rdm[b >> 4] >> sh) & 1u)) return (uint32_t)'X';
    return (0x54474341u >> (8u * ((S.rd[b >> 4] >> sh) & 3u))) & 0xFFu;  // "ACGT"
  }
  if (k == L) return 9u;
  if (k - L - 1 < T) return (unsigned char)ttext[t0 + (k - L - 1)];
  return 10u;
}

// `total` bytes at p, byte k = at(k), by the 64 lanes of one wave, each on its own: whole dwords at the alignment the
// destination ADDRESS has, the bytes in front of the first (lanes 0..2) and behind the last (lanes 8..10) one by one.
// Nothing outside [p, p + total) is written.  (The shape of wave_store, kernels_results.hpp.)
template <class F>
RN_HD void lane_store(unsigned char* p, uint64_t total, uint32_t lane, F at) {
  const uint64_t mis = (uint64_t)(4u - ((uint32_t)(uintptr_t)p & 3u)) & 3u;
  const uint64_t head = mis < total ? mis : total;
  const uint64_t nd = (total - head) >> 2;
  for (uint64_t d = lane; d < nd; d += 64) {
    const uint64_t k = head + 4 * d;
    *reinterpret_cast<uint32_t*>(p + k) = at(k) | (at(k + 1) << 8) | (at(k + 2) << 16) | (at(k + 3) << 24);
  }
  const uint64_t tail0 = head + 4 * nd;
  if (lane < head) p[lane] = (unsigned char)at(lane);
  else if (lane >= 8 && tail0 + (lane - 8) < total) p[tail0 + (lane - 8)] = (unsigned char)at(tail0 + (lane - 8));
}

// ---- render: one item per (record, lane).  Records [r0, r1) into out, record i at off[i] - off[r0].
template <class R>
RN_HD void record_item(const R& rd, const Names& N, const Groups& G, const uint64_t* off, uint64_t r0, uint64_t g, uint32_t lane,
                       unsigned char* out) {
  lane_store(out + (off[g] - off[r0]), off[g + 1] - off[g], lane, [&](uint64_t k) { return record_byte(rd, N, G, g, k); });
}
// (the records as they stand in the read text: a range of them to another place, whatever its alignment)
RN_HD void copy_item(const char* ttext, const uint64_t* toff, uint64_t r0, uint64_t g, uint32_t lane, unsigned char* out) {
  lane_store(out + (toff[g] - toff[r0]), toff[g + 1] - toff[g], lane, [&](uint64_t k) { return (uint32_t)(unsigned char)ttext[toff[g] + k]; });
}
RN_HD void line_item(const Reads& S, const char* ttext, const uint64_t* toff, const uint64_t* off, uint64_t r0, uint64_t g, uint32_t lane,
                     unsigned char* out) {
  lane_store(out + (off[g] - off[r0]), off[g + 1] - off[g], lane, [&](uint64_t k) { return line_byte(S, ttext, toff, g, k); });
}

}  // namespace musc_rn
