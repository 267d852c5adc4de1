// side_names_check.cpp -- the host work of the side outputs (csrc/side_names.hpp: the form check of the gene text and
// the name ranks) against a plain model, as a program of its own so that it runs under the sanitizers.
// It needs no GPU and is not part of the library; muscato_amd/build.py (CHECKS) builds it, plain and sanitized.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>

#include "../side_names.hpp"
#include "check.hpp"

namespace {

struct Text {
  std::string text;
  std::vector<uint64_t> off{0};
  std::vector<uint8_t> absent;
  void add(const std::string& s, bool gone = false) {
    text += s;
    off.push_back(text.size());
    absent.push_back(gone);
  }
  uint32_t n() const { return (uint32_t)absent.size(); }
  // (a copy of exactly the text's size on the heap: a read past its end is an error under the address sanitizer)
  std::vector<char> exact() const { return std::vector<char>(text.begin(), text.end()); }
};

bool model_ok(const std::string& s) {
  size_t tabs = 0;
  for (unsigned char b : s) {
    if (b == '\t') tabs++;
    else if (b <= 0x20) return false;
  }
  return tabs == 1 && s.front() != '\t' && s.back() != '\t';
}

void check(const Text& T) {
  const std::vector<char> buf = T.exact();
  const uint32_t bad = musc_side::first_bad_form(buf.data(), T.off.data(), T.absent.data(), T.n());
  uint32_t want = T.n();
  std::vector<std::string> name(T.n());
  for (uint32_t g = 0; g < T.n(); g++) {
    const std::string s = T.text.substr(T.off[g], T.off[g + 1] - T.off[g]);
    name[g] = s.substr(0, s.find('\t'));
    if (!T.absent[g] && want == T.n() && (s.empty() || !model_ok(s))) want = g;
  }
  EXPECT(bad == want);
  const musc_side::NameRanks R = musc_side::name_ranks(buf.data(), T.off.data(), T.absent.data(), T.n());
  std::map<std::string, uint32_t> first;  // (std::string compares as unsigned bytes: bytewise order)
  for (uint32_t g = 0; g < T.n(); g++)
    if (!T.absent[g]) first.emplace(name[g], g);
  EXPECT(R.rank.size() == T.n() && R.rep.size() == first.size() && R.len.size() == first.size());
  uint32_t k = 0;
  for (auto& kv : first) {
    if (k < R.rep.size()) {
      EXPECT(R.rep[k] == kv.second);
      EXPECT(R.len[k] == kv.first.size());
    }
    k++;
  }
  for (uint32_t g = 0; g < T.n(); g++) {
    if (T.absent[g]) {
      EXPECT(R.rank[g] == musc_side::ABSENT);
    } else {
      EXPECT(R.rank[g] < R.rep.size() && name[R.rep[R.rank[g]]] == name[g]);
    }
  }
}

}  // namespace

int main() {
  {  // the cases of the issue: prefixes, one name with two lengths, identical texts, an absent gene, a high byte
    Text T;
    for (const char* s : {"g9\t5", "g10\t7", "g1\t7", "g\t10", "g\t12", "g1\t7", "\xC3\xA9\t1", "zz\t3"}) T.add(s);
    T.add("gone with blanks\t1", true);
    check(T);
    const std::vector<char> buf = T.exact();
    EXPECT(musc_side::first_bad_form(buf.data(), T.off.data(), T.absent.data(), T.n()) == T.n());
    const musc_side::NameRanks R = musc_side::name_ranks(buf.data(), T.off.data(), T.absent.data(), T.n());
    EXPECT(R.rep.size() == 6 && R.rank[3] == R.rank[4] && R.rank[2] == R.rank[5]);
    EXPECT(R.rank[3] < R.rank[2] && R.rank[2] < R.rank[1] && R.rank[1] < R.rank[0] && R.rank[0] < R.rank[7] && R.rank[7] < R.rank[6]);
  }
  // every way a text can miss the form, as the only text, the first, the last, and hidden by `absent`
  for (const char* bad : {"", "\t", "g\t", "\t5", "g", "g 1\t5", "g\t5\t", "g\t\t5", "g\t5 ", " g\t5", "g\n\t5", "g\t5\r", "a\tb\tc"}) {
    for (int where = 0; where < 4; where++) {
      Text T;
      if (where == 1 || where == 3) T.add("a\t1");
      T.add(bad, where == 3);
      if (where == 2 || where == 3) T.add("b\t2");
      check(T);
      const std::vector<char> buf = T.exact();
      const uint32_t got = musc_side::first_bad_form(buf.data(), T.off.data(), T.absent.data(), T.n());
      EXPECT((got == T.n()) == (where == 3));
    }
  }
  {  // no gene at all, and only absent ones
    Text T;
    check(T);
    T.add("", true);
    T.add("x y", true);
    check(T);
  }
  // random texts over a small alphabet with tabs and blanks: many equal names, prefixes, bad forms
  std::mt19937 rng(17);
  for (int round = 0; round < 2000; round++) {
    Text T;
    const int n = 1 + (int)(rng() % 40);
    for (int g = 0; g < n; g++) {
      std::string s;
      const int len = (int)(rng() % 6);
      for (int i = 0; i < len; i++) s += "ab\xFF"[rng() % 3];
      s += '\t';
      s += std::to_string(rng() % 3);
      if (rng() % 50 == 0) s[rng() % s.size()] = " \t\n\x01"[rng() % 4];
      T.add(s, rng() % 10 == 0);
    }
    check(T);
  }
  return check_done("side_names_check");
}
