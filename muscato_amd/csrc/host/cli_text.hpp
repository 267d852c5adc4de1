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
#include "../cov_plan.hpp"
#include "../sam_plan.hpp"

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
struct ResultsLine {
  std::string six;  // the first six columns
  musc_hit hit;
};
inline std::vector<ResultsLine> results_lines(const musc_hit* hits, size_t nhits, const std::vector<UniqueRead>& reads,
                                              const std::vector<std::string>& targets,
                                              const std::map<uint64_t, std::string>& id_rest) {
  std::vector<ResultsLine> lines;
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
    lines.push_back(ResultsLine{std::move(six), h});
  }
  std::sort(lines.begin(), lines.end(), [](const ResultsLine& a, const ResultsLine& b) { return a.six < b.six; });
  return lines;
}

inline std::string results_text(const std::vector<ResultsLine>& lines, const std::vector<UniqueRead>& reads) {
  std::string out;
  for (auto& l : lines) {
    out += l.six;
    out += '\t';
    out += std::to_string(reads[l.hit.read_idx].count);
    out += '\t';
    out += reads[l.hit.read_idx].names;
    out += '\n';
  }
  return out;
}

inline std::string results_text(const musc_hit* hits, size_t nhits, const std::vector<UniqueRead>& reads,
                                const std::vector<std::string>& targets,
                                const std::map<uint64_t, std::string>& id_rest) {
  return results_text(results_lines(hits, nhits, reads, targets, id_rest), reads);
}

// ---- SAM: the format's C++ copy, and what the CLI writes when the device does not.  One record per
// tuple of `ordered`, the tuples of results.txt in its line order (results_lines, or musc_results_hits); tails[r] is
// read r's count\tnames, tails == nullptr: no read text.  The sizes, the name rules and the refusals are sam_plan.hpp's,
// which the device shares.  False: refused (what musc_sam_prepare answers with code 12), *why says which rule.
inline char sam_base(char c, bool rev) {
  switch (c) {
    case 'A': return rev ? 'T' : 'A';
    case 'C': return rev ? 'G' : 'C';
    case 'G': return rev ? 'C' : 'G';
    case 'T': return rev ? 'A' : 'T';
  }
  return 'N';
}

// seq(r) -> the bases of read r (a const std::string&), tail(r) -> its count\tnames (a std::string), asked only when have_tails
template <class Seq, class Tail>
inline bool sam_text_of(const musc_hit* ordered, size_t n, Seq seq, Tail tail_of, bool have_tails, const std::vector<std::string>& targets,
                        const std::map<uint64_t, std::string>& id_rest, bool rev_pairs, std::string* out, std::string* why) {
  auto u = [](const std::string& s) { return reinterpret_cast<const unsigned char*>(s.data()); };
  const size_t nt = targets.size();
  auto rest = [&](size_t g) -> const std::string* {
    auto it = id_rest.find(g);
    return it == id_rest.end() ? nullptr : &it->second;
  };
  // ---- the refusals
  if (rev_pairs && (nt & 1)) return *why = "rev_pairs with an odd number of targets", false;
  for (size_t g = 0; rev_pairs && g + 1 < nt; g += 2)
    if (targets[g].size() != targets[g + 1].size()) return *why = "rev_pairs, and the two targets of a pair differ in length", false;
  std::vector<musc_sam::NameSpan> name(nt, musc_sam::NameSpan{0, 0});
  for (size_t g = 0; g < nt; g++)
    if (const std::string* r = rest(g)) name[g] = musc_sam::rname_span(u(*r), r->size());
  for (size_t g = 0; g < nt; g++) {
    if (!rest(g)) continue;
    const size_t f = rev_pairs && (g & 1) ? g - 1 : g;
    if (!rest(f) || name[f].len == 0) return *why = "the gene text of a target with an id line (or of its even partner) has an empty first token", false;
  }
  // ---- the header
  std::string& o = *out;
  o = musc_sam::HD_LINE;
  for (size_t t = 0; t < nt; t++) {
    if (!rest(t) || (rev_pairs && (t & 1))) continue;
    o += "@SQ\tSN:";
    o.append(*rest(t), name[t].n0, name[t].len);
    o += "\tLN:" + std::to_string(targets[t].size()) + "\n";
  }
  o += musc_sam::PG_LINE;
  // ---- the records: NH from the runs of equal reads (the list is read-major)
  for (size_t i = 0, run0 = 0, run1 = 0; i < n; i++) {
    if (i == run1) {
      run0 = i;
      while (run1 < n && ordered[run1].read_idx == ordered[i].read_idx) run1++;
    }
    const musc_hit& h = ordered[i];
    const std::string &read = seq(h.read_idx), &t = targets[h.gene_idx];
    const size_t L = read.size(), S = std::min(L, t.size() - h.pos);
    const bool rev = rev_pairs && (h.gene_idx & 1);
    const size_t f = rev ? h.gene_idx - 1 : h.gene_idx;
    const std::string tail_text = have_tails ? tail_of(h.read_idx) : std::string();
    const std::string* tail = &tail_text;
    const musc_sam::TailSpans ts = have_tails ? musc_sam::tail_spans(u(*tail), tail->size()) : musc_sam::TailSpans{0, 0, 0, 0};
    const size_t before = o.size();
    if (ts.qlen) o.append(*tail, ts.q0, ts.qlen);
    else o += '*';
    o += '\t' + std::to_string(musc_sam::flag(rev, i == run0)) + '\t';
    o.append(*rest(f), name[f].n0, name[f].len);
    const uint64_t p1 = musc_sam::pos1(rev, t.size(), h.pos, S);
    o += '\t' + std::to_string(p1) + "\t255\t";
    const std::string clip = L > S ? std::to_string(L - S) + "S" : "", m = std::to_string(S) + "M";
    o += S == 0 ? "*" : rev ? clip + m : m + clip;
    o += "\t*\t0\t0\t";
    if (L == 0) o += '*';
    for (size_t j = 0; j < L; j++) o += sam_base(read[rev ? L - 1 - j : j], rev);
    // NM and MD, walked in forward-strand order
    std::string md;
    size_t d = 0, run = 0;
    for (size_t w = 0; w < S; w++) {
      const size_t j = rev ? S - 1 - w : w;
      const char a = read[j], b = t[h.pos + j];
      auto code = [](char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T' ? c : 'X'; };
      if (code(a) == code(b)) {
        run++;
        continue;
      }
      d++;
      md += std::to_string(run);
      md += sam_base(b, rev);
      run = 0;
    }
    md += std::to_string(run);
    o += "\t*\tNM:i:" + std::to_string(d) + "\tMD:Z:" + md + "\tNH:i:" + std::to_string(run1 - run0) + "\tHI:i:" + std::to_string(i - run0 + 1) +
         "\tXM:i:" + std::to_string(h.nmiss);
    if (ts.count_len) o += "\tXC:i:" + tail->substr(0, ts.count_len);
    o += '\n';
    // (the size rule the device lays its records out by)
    musc_sam::RecordSizes z{ts.qlen ? ts.qlen : 1u, musc_sam::flag(rev, i == run0), name[f].len, p1, (uint32_t)L, (uint32_t)S, (uint32_t)d,
                            (uint32_t)md.size(), (uint32_t)(run1 - run0), (uint32_t)(i - run0 + 1), h.nmiss, ts.count_len};
    if (musc_sam::record_bytes(z) != o.size() - before) return *why = "sam_plan.hpp's size rule and sam_text disagree", false;
  }
  return true;
}

// ... over reads and tails given as strings (tails == nullptr: no read text)
inline bool sam_text(const musc_hit* ordered, size_t n, const std::vector<std::string>& read_seqs, const std::vector<std::string>& targets,
                     const std::map<uint64_t, std::string>& id_rest, const std::vector<std::string>* tails, bool rev_pairs,
                     std::string* out, std::string* why) {
  return sam_text_of(ordered, n, [&](uint32_t r) -> const std::string& { return read_seqs[r]; },
                     [&](uint32_t r) { return (*tails)[r]; }, tails != nullptr, targets, id_rest, rev_pairs, out, why);
}

// ... over the unique reads of a run: the tail of a read is its count, a tab and its names, as in results.txt
inline bool sam_text(const musc_hit* ordered, size_t n, const std::vector<UniqueRead>& reads, const std::vector<std::string>& targets,
                     const std::map<uint64_t, std::string>& id_rest, bool rev_pairs, std::string* out, std::string* why) {
  return sam_text_of(ordered, n, [&](uint32_t r) -> const std::string& { return reads[r].seq; },
                     [&](uint32_t r) { return std::to_string(reads[r].count) + "\t" + reads[r].names; }, true, targets, id_rest, rev_pairs, out,
                     why);
}

// ---- coverage: the stage's C++ copy, and what the CLI writes when the device does not.  `ordered` as for
// sam_text; len_of(r) -> the bases of read r, tail_of(r) -> its count\tnames, asked only when have_tails.  *bed gets the
// bedGraph and *summary the per-target records.  The rules and the sizes are cov_plan.hpp's and sam_plan.hpp's, which
// the device shares; like the device it sorts events, so its memory goes with the lines and not with the database.
// False: refused (what musc_cov_prepare answers with code 12), *why says which rule.
template <class Len, class Tail>
inline bool coverage_text_of(const musc_hit* ordered, size_t n, Len len_of, Tail tail_of, bool have_tails, const std::vector<std::string>& targets,
                             const std::map<uint64_t, std::string>& id_rest, uint32_t flags, std::string* bed, std::string* summary,
                             std::string* why) {
  auto u = [](const std::string& s) { return reinterpret_cast<const unsigned char*>(s.data()); };
  const size_t nt = targets.size();
  const bool rev_pairs = (flags & MUSC_COV_REV_PAIRS) != 0, weighted = (flags & MUSC_COV_WEIGHTED) != 0, unique = (flags & MUSC_COV_UNIQUE) != 0;
  auto rest = [&](size_t g) -> const std::string* {
    auto it = id_rest.find(g);
    return it == id_rest.end() ? nullptr : &it->second;
  };
  // ---- the refusals
  if (musc_cov::lines_refused(n)) return *why = "the list has 2^31 lines or more", false;
  if (rev_pairs && (nt & 1)) return *why = "rev_pairs with an odd number of targets", false;
  for (size_t g = 0; rev_pairs && g + 1 < nt; g += 2)
    if (targets[g].size() != targets[g + 1].size()) return *why = "rev_pairs, and the two targets of a pair differ in length", false;
  std::vector<musc_sam::NameSpan> name(nt, musc_sam::NameSpan{0, 0});
  for (size_t g = 0; g < nt; g++)
    if (const std::string* r = rest(g)) name[g] = musc_sam::rname_span(u(*r), r->size());
  for (size_t g = 0; g < nt; g++) {
    if (!rest(g)) continue;
    const size_t f = rev_pairs && (g & 1) ? g - 1 : g;
    if (!rest(f) || name[f].len == 0) return *why = "the gene text of a target with an id line (or of its even partner) has an empty first token", false;
  }
  // ---- the events of the contributing lines, their weights per target and in all
  struct Event { uint64_t slot; uint32_t delta; };
  std::vector<Event> ev;
  ev.reserve(2 * n);
  std::vector<uint64_t> seq_off(nt + 1, 0), numreads(nt, 0);
  for (size_t g = 0; g < nt; g++) seq_off[g + 1] = seq_off[g] + targets[g].size();
  uint64_t total = 0;
  for (size_t i = 0, run1 = 0; i < n; i++) {
    if (i == run1)
      while (run1 < n && ordered[run1].read_idx == ordered[i].read_idx) run1++;  // (the list is read-major)
    const musc_hit& h = ordered[i];
    if (unique && !((i == 0 || ordered[i - 1].read_idx != h.read_idx) && run1 == i + 1)) continue;
    uint64_t w = 1;
    if (weighted && have_tails) {
      const std::string tail = tail_of(h.read_idx);
      w = musc_cov::weight(u(tail), tail.size());
    }
    // (musc_results_order and results_lines drop the lines of targets without an id line; one that comes here all the
    // same has no name to be written under)
    if (h.gene_idx >= nt || !rest(h.gene_idx) || h.pos > targets[h.gene_idx].size())
      return *why = "a line of the ordered list is on a target without an id line, or past its target's end", false;
    const musc_cov::Interval v = musc_cov::interval(rev_pairs, h.gene_idx, h.pos, targets[h.gene_idx].size(), len_of(h.read_idx));
    total += w;
    if (musc_cov::total_refused(total)) return *why = "the weights of the contributing lines add up to 2^32 or more", false;
    numreads[v.f] += w;
    if (w == 0 || v.S == 0) continue;
    ev.push_back(Event{musc_cov::slot(seq_off[v.f], v.f, v.a), (uint32_t)w});
    ev.push_back(Event{musc_cov::slot(seq_off[v.f], v.f, v.a + v.S), 0u - (uint32_t)w});
  }
  std::sort(ev.begin(), ev.end(), [](const Event& a, const Event& b) { return a.slot < b.slot; });
  // ---- the runs, target by target (the slots of a target are consecutive), and the summary
  bed->clear(), summary->clear();
  size_t e = 0;
  for (size_t t = 0; t < nt; t++) {
    const uint64_t base = seq_off[t] + t, len = targets[t].size();
    uint64_t covbases = 0, sumdepth = 0, start = 0;
    uint32_t depth = 0, maxdepth = 0;
    while (e < ev.size() && ev[e].slot <= base + len) {
      const uint64_t x = ev[e].slot - base;
      uint32_t d = depth;
      for (; e < ev.size() && ev[e].slot == base + x; e++) d += ev[e].delta;
      if (d == depth) continue;
      if (depth) {
        const size_t before = bed->size();
        bed->append(*rest(t), name[t].n0, name[t].len);
        *bed += '\t' + std::to_string(start) + '\t' + std::to_string(x) + '\t' + std::to_string(depth) + '\n';
        if (musc_cov::run_bytes(name[t].len, start, x, depth) != bed->size() - before) return *why = "cov_plan.hpp's size rule and coverage_text disagree", false;
        covbases += x - start, sumdepth += (x - start) * depth;
        if (depth > maxdepth) maxdepth = depth;
      }
      depth = d, start = x;
    }
    if (depth) return *why = "coverage_text: a run does not end within its target", false;
    if (!rest(t) || (rev_pairs && (t & 1))) continue;
    const size_t before = summary->size();
    summary->append(*rest(t), name[t].n0, name[t].len);
    *summary += '\t' + std::to_string(len) + '\t' + std::to_string(numreads[t]) + '\t' + std::to_string(covbases) + '\t' + std::to_string(sumdepth) +
                '\t' + std::to_string(maxdepth) + '\n';
    if (musc_cov::summary_bytes(name[t].len, len, (uint32_t)numreads[t], covbases, sumdepth, maxdepth) != summary->size() - before)
      return *why = "cov_plan.hpp's size rule and coverage_text disagree", false;
  }
  return true;
}

// ... over reads and tails given as strings (tails == nullptr: no read text)
inline bool coverage_text(const musc_hit* ordered, size_t n, const std::vector<std::string>& read_seqs, const std::vector<std::string>& targets,
                          const std::map<uint64_t, std::string>& id_rest, const std::vector<std::string>* tails, uint32_t flags, std::string* bed,
                          std::string* summary, std::string* why) {
  return coverage_text_of(ordered, n, [&](uint32_t r) { return read_seqs[r].size(); }, [&](uint32_t r) { return (*tails)[r]; }, tails != nullptr,
                          targets, id_rest, flags, bed, summary, why);
}

// ... over the unique reads of a run: the tail of a read is its count, a tab and its names, as in results.txt
inline bool coverage_text(const musc_hit* ordered, size_t n, const std::vector<UniqueRead>& reads, const std::vector<std::string>& targets,
                          const std::map<uint64_t, std::string>& id_rest, uint32_t flags, std::string* bed, std::string* summary, std::string* why) {
  return coverage_text_of(ordered, n, [&](uint32_t r) { return reads[r].seq.size(); },
                          [&](uint32_t r) { return std::to_string(reads[r].count) + "\t" + reads[r].names; }, true, targets, id_rest, flags, bed,
                          summary, why);
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
