// cov_host_driver.cpp -- a stand-alone program around musc::coverage_text (muscato_amd/csrc/host/cli_text.hpp), the host
// copy of the coverage stage: tests/test_cov_cases.py compiles it, feeds it a case and holds its output to the Python
// model byte for byte.  No GPU and no library.
//
// Input (stdin), every string as one line of hex digits behind an `h`, `-` for a gene without an id line:
//   flags have_tails nreads ntargets nhits
//   nreads read lines, [nreads tail lines], ntargets target lines, ntargets gene text lines, nhits lines `r g pos nmiss`
// Output: the bedGraph, a line `#summary`, the summary on stdout; exit status 12 and the reason on stderr when
// coverage_text refuses.
#include <cstdio>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "../muscato_amd/csrc/host/cli_text.hpp"

static bool line(std::string* s) {
  std::string l;
  if (!std::getline(std::cin, l)) return false;
  if (l == "-") return s->clear(), false;
  s->clear();
  for (size_t i = 1; i + 1 < l.size(); i += 2) s->push_back((char)std::stoi(l.substr(i, 2), nullptr, 16));
  return true;
}

int main() {
  unsigned flags = 0;
  int have_tails = 0;
  size_t nreads = 0, ntargets = 0, nhits = 0;
  std::cin >> flags >> have_tails >> nreads >> ntargets >> nhits;
  std::string skip;
  std::getline(std::cin, skip);
  std::vector<std::string> reads(nreads), tails(have_tails ? nreads : 0), targets(ntargets);
  std::map<uint64_t, std::string> id_rest;
  for (auto& r : reads) line(&r);
  for (auto& t : tails) line(&t);
  for (auto& t : targets) line(&t);
  for (size_t g = 0; g < ntargets; g++) {
    std::string s;
    if (line(&s)) id_rest[g] = s;
  }
  std::vector<musc_hit> hits(nhits);
  for (auto& h : hits) std::cin >> h.read_idx >> h.gene_idx >> h.pos >> h.nmiss;
  std::string bed, summary, why;
  if (!musc::coverage_text(hits.data(), hits.size(), reads, targets, id_rest, have_tails ? &tails : nullptr, flags, &bed, &summary, &why)) {
    fprintf(stderr, "%s\n", why.c_str());
    return 12;
  }
  fwrite(bed.data(), 1, bed.size(), stdout);
  fputs("#summary\n", stdout);
  fwrite(summary.data(), 1, summary.size(), stdout);
  return 0;
}
