// cli_names.hpp -- the name rules of read preparation, once, for the host parse and the device parse alike.  Plain
// C++17, included by muscato_host.hpp and by cli_plan_check.cpp, which holds both to the two loops they replaced.
#pragma once

#include <algorithm>
#include <string>

namespace musc {

// cmd/muscato_prep_reads/main.go:76-79: a name longer than 1000 bytes becomes its first 995 and "..."
inline std::string clip_name(std::string rn) {
  if (rn.size() > 1000) rn.replace(995, std::string::npos, "...");
  return rn;
}

// cmd/muscato_uniqify/main.go:83-135 after the `sort` of the `seq\tname` lines: the (clipped) names [b, e) of one
// sequence in bytewise order of the whole name, each cut at its first tab (toks[1]: what follows a second tab of the
// line is dropped), joined with ';', the join clipped to its first 996 bytes and "..." when longer than 1000.
// Sorts the range in place.
inline std::string join_group_names(std::string* b, std::string* e) {
  std::sort(b, e);
  std::string na;
  for (const std::string* s = b; s != e; ++s) {
    if (s != b) na += ';';
    na.append(*s, 0, s->find('\t'));
  }
  if (na.size() > 1000) na.replace(996, std::string::npos, "...");
  return na;
}

}  // namespace musc
