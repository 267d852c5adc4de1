// cli_text.hpp -- the text post-chain on the host (cmd/muscato/main.go:422-676 and the side-output tools): results.txt,
// the nonmatch FASTQ, genestats and readstats from the tuples and the unique reads, and the line and field rules they
// share.  The device renders the same bytes (muscato_host.hpp: results_text_device, side_texts_device).
#pragma once

#include <algorithm>
#include <cctype>
#include <cstdint>
#include <map>
#include <set>
#include <string>
#include <string_view>
#include <unordered_set>
#include <vector>

#include "../../../include/muscato_hip.h"

namespace musc {

// Views into a text: the same line and field rules as split_lines / fields, without copies (the
// side outputs walk results.txt three times; at a million lines the copies were most of a run).
template <class F>
inline void for_each_line(const std::string& s, F f) {
  size_t pos = 0;
  while (pos < s.size()) {
    const size_t e = s.find('\n', pos);
    const size_t end = e == std::string::npos ? s.size() : e;
    size_t len = end - pos;
    if (len && s[pos + len - 1] == '\r') len--;
    f(std::string_view(s.data() + pos, len));
    if (e == std::string::npos) break;
    pos = e + 1;
  }
}

inline int fields_sv(std::string_view s, std::string_view* out, int maxf) {  // bytes.Fields, first maxf
  int n = 0;
  size_t i = 0;
  while (i < s.size() && n < maxf) {
    while (i < s.size() && isspace((unsigned char)s[i])) i++;
    const size_t b = i;
    while (i < s.size() && !isspace((unsigned char)s[i])) i++;
    if (i > b) out[n++] = s.substr(b, i - b);
  }
  return n;
}

// a line of reads_sorted.txt: what read preparation (utils/fastq.go, cmd/muscato_prep_reads, `sort`,
// cmd/muscato_uniqify) leaves of the read file
struct UniqueRead {
  std::string seq;
  size_t count;
  std::string names;
};

// Go's strings.Fields / bytes.Fields on ASCII whitespace
inline std::vector<std::string> fields(const std::string& s) {
  std::vector<std::string> f;
  size_t i = 0;
  while (i < s.size()) {
    while (i < s.size() && isspace((unsigned char)s[i])) i++;
    size_t b = i;
    while (i < s.size() && !isspace((unsigned char)s[i])) i++;
    if (i > b) f.emplace_back(s, b, i - b);
  }
  return f;
}

// hits must already be the per-read best+MMTol selection (matches.txt).  Produces the bytes
// of ResultsFileName: sort -k5 + join with the id file + cut (:524-611) turns the gene number
// into "name\tlen" (hits whose number is absent from the id file are unpairable and vanish);
// sort -k1 (:657) orders the six-column lines bytewise; join (:659) appends count and names.
inline std::string results_text(const musc_hit* hits, size_t nhits, const std::vector<UniqueRead>& reads,
                                const std::vector<std::string>& targets,
                                const std::map<uint64_t, std::string>& id_rest) {
  struct Line { std::string six; uint32_t read; };
  std::vector<Line> lines;
  lines.reserve(nhits);
  for (size_t i = 0; i < nhits; i++) {
    const musc_hit& h = hits[i];
    auto it = id_rest.find(h.gene_idx);
    if (it == id_rest.end()) continue;
    const std::string& r = reads[h.read_idx].seq;
    std::string six = r;
    six += '\t';
    six.append(targets[h.gene_idx], h.pos, r.size());
    six += '\t';
    six += std::to_string(h.pos);
    six += '\t';
    six += std::to_string(h.nmiss);
    six += '\t';
    six += it->second;
    lines.push_back(Line{std::move(six), h.read_idx});
  }
  std::sort(lines.begin(), lines.end(), [](const Line& a, const Line& b) { return a.six < b.six; });
  std::string out;
  for (auto& l : lines) {
    out += l.six;
    out += '\t';
    out += std::to_string(reads[l.read].count);
    out += '\t';
    out += reads[l.read].names;
    out += '\n';
  }
  return out;
}

inline std::string nonmatch_name(const std::string& results) {  // cmd/muscato_nonmatch/main.go:67-73
  size_t slash = results.rfind('/');
  std::string a = slash == std::string::npos ? "" : results.substr(0, slash + 1);
  std::string b = slash == std::string::npos ? results : results.substr(slash + 1);
  std::vector<std::string> c;
  size_t p = 0;
  for (;;) {
    size_t e = b.find('.', p);
    c.push_back(b.substr(p, e == std::string::npos ? std::string::npos : e - p));
    if (e == std::string::npos) break;
    p = e + 1;
  }
  std::string d = c.back();
  c.back() = "nonmatch";
  c.push_back(d + ".fastq");
  std::string j;
  for (size_t i = 0; i < c.size(); i++) { if (i) j += '.'; j += c[i]; }
  return a + j;
}

// cmd/muscato_nonmatch/main.go:95-114 with an exact set in place of the Bloom filter
inline std::string nonmatch_text(const std::string& results, const std::vector<UniqueRead>& reads) {
  std::unordered_set<std::string_view> matched;
  for_each_line(results, [&](std::string_view line) {
    std::string_view f[1];
    if (fields_sv(line, f, 1)) matched.insert(f[0]);
  });
  std::string out;
  for (auto& u : reads) {
    if (matched.count(std::string_view(u.seq))) continue;
    auto f = fields(u.seq + "\t" + std::to_string(u.count) + "\t" + u.names);
    if (f.size() < 3) continue;  // the reference would panic on an empty name
    out += f[2] + "#" + f[1] + "\n" + f[0] + "\n+\n" + std::string(f[0].size(), '!') + "\n";
  }
  return out;
}

inline std::string stats_name(const std::string& results, const char* tag) {  // path.Ext handling, :113-120
  size_t slash = results.rfind('/');
  size_t dot = results.rfind('.');
  if (dot != std::string::npos && (slash == std::string::npos || dot > slash))
    return results.substr(0, dot) + tag + results.substr(dot);
  return results + tag;
}

// cmd/muscato/main.go:94-150 + cmd/muscato_genestats/main.go: sort -k5, count runs of column 5
inline std::string genestats_text(const std::string& results) {
  struct Ln {
    std::string_view line, key;  // key: GNU sort -k5 = from the blank before field 5 to the end
  };
  std::vector<Ln> lines;
  for_each_line(results, [&](std::string_view l) {
    size_t p = 0;
    for (int f = 0; f < 4; f++) {
      while (p < l.size() && (l[p] == ' ' || l[p] == '\t')) p++;
      while (p < l.size() && l[p] != ' ' && l[p] != '\t') p++;
    }
    lines.push_back(Ln{l, l.substr(p)});
  });
  std::sort(lines.begin(), lines.end(), [](const Ln& a, const Ln& b) {
    const int c = a.key.compare(b.key);
    if (c) return c < 0;
    return a.line < b.line;
  });
  std::string out;
  std::string_view old;
  size_t n = 0;
  bool first = true;
  auto flush = [&]() {
    out.append(old.data(), old.size());
    out += "\t" + std::to_string(n) + "\t\n";
  };
  for (auto& l : lines) {
    std::string_view f[5];
    if (fields_sv(l.line, f, 5) < 5) continue;
    if (first) { old = f[4]; first = false; }
    if (f[4] != old) { flush(); old = f[4]; n = 0; }
    n++;
  }
  if (!first) flush();
  return out;
}

// cmd/muscato_readstats/main.go: per run of equal names-column tokens, the set of gene names.
// The reference prints the set in Go map order (random); here it is sorted.
inline std::string readstats_text(const std::string& results) {
  std::string out;
  std::string_view old;
  std::set<std::string_view> genes;
  bool first = true;
  auto flush = [&]() {
    out.append(old.data(), old.size());
    out += '\t';
    for (auto& g : genes) { out.append(g.data(), g.size()); out += ';'; }
    out += '\n';
  };
  for_each_line(results, [&](std::string_view l) {
    std::string_view f[8];
    if (fields_sv(l, f, 8) < 8) return;
    if (first) { old = f[7]; first = false; }
    if (f[7] != old) { flush(); old = f[7]; genes.clear(); }
    genes.insert(f[4]);
  });
  if (!first) flush();
  return out;
}

}  // namespace musc
