// side_names.hpp -- host work on the gene text for the side outputs: the form the device path
// requires, and the rank of every gene's NAME among all names.  Plain C++, no HIP: included by muscato_hip.hip and by
// host/side_names_check.cpp, the stand-alone program that runs it under the sanitizers.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace musc_side {

static const uint32_t ABSENT = 0xFFFFFFFFu;

// Every present gene's text is `name \t len`: exactly one tab, both sides non-empty, every other byte above 0x20.
// Then a results line has the name as field 5 and the read's first name as field 8, and bytewise name order is the
// `sort -k5` run order (cmd/muscato/main.go:94-150).  Returns the first gene whose text is not so, or nseq.
inline uint32_t first_bad_form(const char* text, const uint64_t* offsets, const uint8_t* absent, uint32_t nseq) {
  for (uint32_t g = 0; g < nseq; g++) {
    if (absent && absent[g]) continue;
    const unsigned char* const p = reinterpret_cast<const unsigned char*>(text) + offsets[g];
    const uint64_t n = offsets[g + 1] - offsets[g];
    uint64_t tabs = 0, tab_at = 0;
    bool ok = true;
    for (uint64_t i = 0; i < n && ok; i++) {
      if (p[i] == '\t') {
        tabs++;
        tab_at = i;
      } else if (p[i] <= 0x20) {
        ok = false;
      }
    }
    if (!ok || tabs != 1 || tab_at == 0 || tab_at + 1 == n) return g;
  }
  return nseq;
}

struct NameRanks {
  std::vector<uint32_t> rank;      // per gene: rank of its name, bytewise; equal names share one; ABSENT without an id line
  std::vector<uint32_t> rep, len;  // per rank: a gene that has the name (the lowest such gene), the name's bytes
};

// The name of gene g is its text up to the first tab (all of it without one).
inline NameRanks name_ranks(const char* text, const uint64_t* offsets, const uint8_t* absent, uint32_t nseq) {
  NameRanks R;
  R.rank.assign(nseq, ABSENT);
  std::vector<uint32_t> order, nlen(nseq, 0);
  for (uint32_t g = 0; g < nseq; g++) {
    if (absent && absent[g]) continue;
    const uint64_t n = offsets[g + 1] - offsets[g];
    const void* const t = n ? memchr(text + offsets[g], '\t', (size_t)n) : nullptr;
    const uint64_t l = t ? (uint64_t)(static_cast<const char*>(t) - (text + offsets[g])) : n;
    nlen[g] = (uint32_t)std::min<uint64_t>(l, 0xFFFFFFFFull);
    order.push_back(g);
  }
  auto cmp = [&](uint32_t a, uint32_t b) {
    const uint32_t m = std::min(nlen[a], nlen[b]);
    const int d = m ? memcmp(text + offsets[a], text + offsets[b], m) : 0;
    return d ? d : nlen[a] < nlen[b] ? -1 : nlen[a] > nlen[b] ? 1 : 0;
  };
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const int d = cmp(a, b);
    return d ? d < 0 : a < b;
  });
  for (size_t i = 0; i < order.size(); i++) {
    if (i == 0 || cmp(order[i - 1], order[i]) != 0) {
      R.rep.push_back(order[i]);
      R.len.push_back(nlen[order[i]]);
    }
    R.rank[order[i]] = (uint32_t)R.rep.size() - 1u;
  }
  return R;
}

}  // namespace musc_side
