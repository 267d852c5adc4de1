// read_names_plan_check.cpp -- read_names_plan.hpp against a literal restatement of the reference's string code
// (cmd/muscato_prep_reads/main.go:76-79, cmd/muscato_uniqify/main.go:83-135), byte loop by byte loop: every name length
// 0..1100 with a tab at every place that matters and without one, joins of every length around the bounds, the decimal
// widths, the lengths of a record and a line, and the path of a group.  Stand-alone, no GPU: muscato_amd/build.py
// (CHECKS) builds it, plain and under the sanitizers.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../read_names_plan.hpp"
#include "check.hpp"

using namespace musc_rn;

// ---- the reference, as strings
static std::string ref_clip(const std::string& name) { return name.size() > 1000 ? name.substr(0, 995) + "..." : name; }
static std::string ref_token(const std::string& clipped) {
  std::string t;
  for (char ch : clipped) {
    if (ch == '\t') break;
    t.push_back(ch);
  }
  return t;
}
static std::string ref_join(const std::vector<std::string>& tokens) {
  std::string j;
  for (size_t i = 0; i < tokens.size(); i++) {
    if (i) j.push_back(';');
    j += tokens[i];
  }
  return j.size() > 1000 ? j.substr(0, 996) + "..." : j;
}

// a name of n bytes without a tab; every byte differs from its neighbours so that a shifted copy would show
static std::string make_name(uint32_t n) {
  std::string s(n, 'a');
  for (uint32_t i = 0; i < n; i++) s[i] = (char)('a' + i % 23);
  return s;
}

static void check_name(const std::string& name) {
  const uint32_t n = (uint32_t)name.size();
  const std::string c = ref_clip(name), t = ref_token(c);
  EXPECT_MSG(clipped_len(n) == c.size(), "name of %u bytes", n);
  EXPECT_MSG(text_len(n) <= n && text_len(n) <= clipped_len(n), "name of %u bytes", n);
  if (clipped_len(n) != c.size() || text_len(n) > n) return;  // (a failed check goes on: the loops below index by these)
  for (uint32_t i = 0; i < clipped_len(n); i++) {  // the clipped name by position
    const char b = virtual_byte(n, i) ? '.' : name[i];
    EXPECT_MSG(b == c[i], "name of %u bytes, byte %u", n, i);
    EXPECT_MSG(virtual_byte(n, i) == (i >= text_len(n)), "name of %u bytes, byte %u", n, i);
  }
  uint32_t tab = text_len(n);  // the search the kernel makes: over the bytes that come from the text only
  for (uint32_t i = 0; i < text_len(n); i++)
    if (name[i] == '\t') {
      tab = i;
      break;
    }
  EXPECT_MSG(token_len(n, tab) == t.size(), "name of %u bytes, first tab %u", n, tab);
  EXPECT_MSG(token_len(n, tab == text_len(n) ? 0xFFFFFFFFu : tab) == t.size(), "name of %u bytes: any value past the text says no tab", n);
  const uint32_t m = meta_pack(clipped_len(n), token_len(n, tab));
  EXPECT_MSG(meta_clip(m) == c.size() && meta_tok(m) == t.size(), "meta of a name of %u bytes", n);
}

int main() {
  // ---- names
  for (uint32_t n = 0; n <= 1100; n++) {
    const std::string base = make_name(n);
    check_name(base);
    std::vector<uint32_t> at = {0, 1, 7, 8, 9, n / 2, 993, 994, 995, 996, 997, 998, 999, 1000, n - 2, n - 1};
    for (uint32_t p : at) {
      if (p >= n) continue;
      std::string s = base;
      s[p] = '\t';
      check_name(s);
      if (p + 3 < n) {  // a second tab behind the first
        s[p + 3] = '\t';
        check_name(s);
      }
    }
  }
  // ---- decimal widths
  for (uint64_t v : {0ull, 1ull, 9ull, 10ull, 99ull, 100ull, 999ull, 1000ull, 9999ull, 10000ull, 99999ull, 100000ull, 4294967279ull,
                     4294967295ull, 9999999999ull, 10000000000ull})
    EXPECT_MSG(dec_width(v) == std::to_string(v).size(), "width of %llu", (unsigned long long)v);
  for (uint64_t v = 0; v < 200000; v++) EXPECT_MSG(dec_width(v) == std::to_string(v).size(), "width of %llu", (unsigned long long)v);

  // ---- joins: k tokens of equal length and one that sets the total, for every total around the bounds
  for (uint32_t k : {1u, 2u, 3u, 64u, 65u, 500u}) {
    for (uint32_t total = (k > 990 ? k : 990); total <= 1012; total++) {
      if (total < k - 1) continue;  // (the separators alone are longer)
      const uint32_t body = total - (k - 1), each = body / k;
      std::vector<std::string> tokens(k, make_name(each));
      tokens[k - 1] = make_name(body - each * (k - 1));
      uint64_t sum = 0;
      for (const std::string& t : tokens) sum += t.size() + 1;
      sum -= 1;
      EXPECT_MSG(sum == total, "a join of %u tokens", k);
      const std::string j = ref_join(tokens);
      for (uint64_t s : {sum, sum > JOIN_LIMIT ? (uint64_t)JOIN_LIMIT + 1 : sum, sum > JOIN_LIMIT ? sum + 100000 : sum}) {  // saturated sums say the same
        EXPECT_MSG(join_len(s) == j.size(), "join of %u bytes", total);
        EXPECT_MSG(join_clipped(s) == (total > 1000), "join of %u bytes", total);
        EXPECT_MSG(join_text_len(s) + (join_clipped(s) ? DOTS : 0) == j.size(), "join of %u bytes", total);
        for (uint64_t count : {1ull, 9ull, 10ull, 5000ull, 4294967279ull}) {
          const std::string rec = std::to_string(count) + "\t" + j;
          EXPECT_MSG(record_len(count, s) == rec.size(), "record of %llu reads, join of %u bytes", (unsigned long long)count, total);
          for (uint64_t L : {0ull, 1ull, 100ull, 65535ull}) {
            const std::string line = std::string(L, 'A') + "\t" + rec + "\n";
            EXPECT_MSG(line_len(L, count, s) == line.size(), "line of a read of %llu bases", (unsigned long long)L);
          }
        }
      }
      // the bytes of the join by position: token m starts at the scan of token + 1, nothing is written at or past the cut
      std::string byp(join_len(sum), '?');
      uint64_t start = 0;
      const uint32_t limit = join_text_len(sum);
      for (uint32_t m = 0; m < k && start < limit; m++) {
        for (uint64_t p = 0; p < tokens[m].size() && start + p < limit; p++) byp[start + p] = tokens[m][p];
        if (m + 1 < k && start + tokens[m].size() < limit) byp[start + tokens[m].size()] = ';';
        start += tokens[m].size() + 1;
      }
      if (join_clipped(sum))
        for (uint32_t d = 0; d < DOTS; d++) byp[limit + d] = '.';
      EXPECT_MSG(byp == j, "join of %u tokens, %u bytes, by position", k, total);
    }
  }
  // ---- paths and the refusal bound
  for (uint64_t c = 0; c < 10000; c++) {
    const Path p = group_path(c);
    EXPECT_MSG(p == (c < 2 ? PATH_SINGLE : c <= 64 ? PATH_WAVE : PATH_SORTED), "group of %llu", (unsigned long long)c);
  }
  EXPECT_MSG(group_path(0xFFFFFFFFull) == PATH_SORTED, "the largest group");
  EXPECT_MSG(!refused(0) && !refused(0xFFFFFFEFull) && refused(0xFFFFFFF0ull) && refused(0xFFFFFFFFull) && refused(1ull << 40), "refusal bound");
  return check_done("read_names_plan_check");
}
